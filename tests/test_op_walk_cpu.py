"""The rows of tests/op_walk_cases.py on the host: every case reaches its edge; the three host rules -- the scalar count
lrm_aln_summary_host, and lrm_aln_diff_host and lrm_pileup_add_host, which walk a row through op_rows.h's host walk and the
kernels' own word steps -- equal the Python references (tests/aln_summary_ref.py, tests/md_ref.py, tests/pileup_ref.py)."""
import numpy as np

import aln_summary_ref
import md_ref
import op_walk_cases as W
import pileup_cases as K
import pileup_ref
from longreadmapper_amd import capi, mapper
from longreadmapper_amd.capi import lib

TEXT = bytes(np.random.default_rng(11).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=W.HI + 50))


def test_cases_reach_their_edges():
    names = [c.name for c in W.CASES]
    assert len(set(names)) == len(names) and 36 <= len(names) <= 100
    missed = [c.name for c in W.CASES if not c.reaches()]
    assert not missed, missed
    assert {len(c.ops) for c in W.CASES} == set(W.LENGTHS)
    assert [W.steps_of(m) for m in W.LENGTHS] == [(1, 2), (2, 0), (2, 1), (3, 1)]
    # every kind of run at every edge in every relation, and every row inside the window
    for e in W.EDGES:
        for kind in "XDI":
            assert {"%s-run-%s-%d" % (kind, rel, e) for rel in ("ends-on", "starts-on", "straddles")} <= set(names)
    assert all(W.LO <= c.loc and c.loc + K.span(c.ops) <= W.HI for c in W.CASES)
    assert any(c.meta_r == 0 for c in W.CASES) and any(c.n_ops is not None and 0 < c.n_ops < len(c.ops) for c in W.CASES)


def test_summary_host_rule():
    for c in W.CASES:
        ops = K.effective_ops(c)
        assert mapper.aln_summary_host(ops) == aln_summary_ref.summary(ops), c.name


def test_diff_host_rule():
    total = 0
    for c in W.CASES:
        ops = K.effective_ops(c)
        want = md_ref.events(ops, TEXT, c.loc)
        assert mapper.aln_diff_host(ops, TEXT[c.loc:]).tolist() == want, c.name
        total += len(want)
    assert total > 20000


def test_pileup_host_rule():
    lo, hi, width = W.LO, W.HI, W.HI - W.LO
    total = pileup_ref.Pileup(lo, hi)
    planes_all = np.zeros(8 * width + 1, dtype=np.uint32)
    out = np.zeros(width, dtype=capi.PILEUP_COL_DT)
    for c in W.CASES:
        ops = K.effective_ops(c)
        if not pileup_ref.aligned(ops, c.score, c.meta_r):
            continue
        ref = pileup_ref.Pileup(lo, hi)
        planes = np.zeros(8 * width + 1, dtype=np.uint32)
        o, r = np.frombuffer(ops, dtype=np.uint8).copy(), np.frombuffer(c.read, dtype=np.uint8).copy()
        for p, acc in ((planes, ref), (planes_all, total)):
            lib.lrm_pileup_add_host(o.ctypes.data, len(ops), r.ctypes.data, len(r), c.loc, lo, hi, p.ctypes.data)
            acc.add(ops, c.read, c.loc)
        capi.check(lib.lrm_pileup_cols_host(planes.ctypes.data, lo, hi, 0, width, out.ctypes.data), "lrm_pileup_cols_host")
        assert pileup_ref.same(out, ref.columns()), (c.name, pileup_ref.first_difference(out, ref.columns()))
    capi.check(lib.lrm_pileup_cols_host(planes_all.ctypes.data, lo, hi, 0, width, out.ctypes.data), "lrm_pileup_cols_host")
    want = total.columns()
    assert pileup_ref.same(out, want), pileup_ref.first_difference(out, want)
    assert all(want[f].any() for f in pileup_ref.COL_FIELDS)
