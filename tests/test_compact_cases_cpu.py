"""The constructed inputs of tests/compact_cases.py without a GPU: each builder has the edges it claims, and the host plans
(lrm_split_plan, lrm_secondary_plan) over them equal the Python rules (split_ref.plan, rival_ref.plan) -- the same tables the
GPU tests of tests/test_gpu_compact_rows.py demand of the device stages."""
import ctypes as C

import numpy as np
import pytest

import compact_cases as cc
import rival_ref
import split_ref
from longreadmapper_amd import mapper
from longreadmapper_amd.capi import lib


@pytest.fixture(scope="module")
def split_order():
    return cc.split_order_case()


def test_order_pattern_has_its_edges():
    p = cc.order_pattern()
    per = cc.check_order_pattern(p)
    assert p.dtype == np.bool_ and len(p) == 65_829
    print("order pattern: %d rows of %d reads; workgroups 254..257 hold %s; %d workgroups empty, %d full" %
          (p.sum(), len(p), per[254:258].tolist(), (per == 0).sum(), (per[:-1] == 256).sum()))
    # the prefix at the second scan tile's first workgroup is what the carry holds there
    assert per[:256].sum() == p[:65_536].sum() > 0
    with pytest.raises(AssertionError):
        cc.check_order_pattern(np.zeros(cc.N_ORDER, dtype=bool))


def test_split_order_case_has_every_kind(split_order):
    c = split_order
    lens, cl, cr, kind, p = c["lens"], c["cl"], c["cr"], c["kind"], c["pattern"]
    assert sorted(set(kind.tolist())) == [-1, 0, 1, 2, 3, 4, 5, 6]
    assert all(kind[i] == 2 for i in cc.TWO_AT)
    assert ((cl == lens) & (kind == 5)).any() and ((cl == lens + 5) & (kind == 6)).any()
    assert c["reads"].shape == (cc.N_ORDER, 401)
    filled = c["reads"] != 0
    assert np.array_equal(filled.sum(axis=1), lens) and filled[np.arange(len(lens)), lens - 1].all()
    table = split_ref.plan(lens, cl, cr, cc.M)
    reads_of = np.array([t[0] for t in table])
    assert np.array_equal(np.unique(reads_of), np.flatnonzero(p))
    # a two-segment read in the last lane of workgroup 0, of scan tile 0 and of the batch: its second record is the next
    # workgroup's / tile's first index
    first = {r: int(np.searchsorted(reads_of, r)) for r in (256, 65_536)}
    assert reads_of[first[256] - 1] == reads_of[first[256] - 2] == 255
    assert reads_of[first[65_536] - 1] == reads_of[first[65_536] - 2] == 65_535
    assert reads_of[-1] == reads_of[-2] == cc.N_ORDER - 1
    print("split order case: %d segments of %d reads, kinds %s" % (len(table), p.sum(), np.bincount(kind[kind >= 0]).tolist()))


def test_split_plan_over_the_order_pattern(split_order):
    c = split_order
    want = split_ref.plan(c["lens"], c["cl"], c["cr"], cc.M)
    got = mapper.split_plan(c["lens"], cc.clip_records(c["cl"], c["cr"]), cc.M)
    assert len(got) == len(want) and len(want) % 256 != 0
    w = np.array(want, dtype=np.uint32)
    for col, f in enumerate(("read", "start", "len", "flags")):
        assert np.array_equal(got[f], w[:, col]), f


def test_secondary_plan_over_the_order_pattern():
    p = cc.order_pattern()
    rec = cc.secondary_records(p)
    want = rival_ref.plan(rec)
    assert np.array_equal(want, np.flatnonzero(p))
    table = np.zeros(len(want), dtype=mapper.SECONDARY_DT)
    k = C.c_uint64()
    assert lib.lrm_secondary_plan(rec.ctypes.data, len(rec), 0, 0, table.ctypes.data, len(table), C.byref(k)) == 0
    assert k.value == len(want) and np.array_equal(table["read"], want)
    # every kind of record that is no candidate occurs
    none = rec[~p]
    assert (none["n2"] == 7).any() and ((none["n2"] == 9) & (none["n1"] == 19)).any() and (none["flags"] != 0).any() and \
        ((none["n1"] == 0) & (none["n2"] == 0)).any()
    assert (rec["n1"][p] == 20).all() and (rec["n2"][p] == 12).all() and not rec["flags"][p].any()


def test_gather_cases_have_their_edges():
    assert len(cc.gather_lengths) == 13
    g = cc.split_gather_case()                                     # (asserts lengths, the tight stride and the 16 phases)
    table = split_ref.plan(g["lens"], g["cl"], g["cr"], cc.M)
    got = mapper.split_plan(g["lens"], cc.clip_records(g["cl"], g["cr"]), cc.M)
    assert [tuple(int(x) for x in s) for s in got] == table
    seg_len = np.array([t[2] for t in table])
    assert seg_len.max() == cc.MAX_LEN == g["lens"].max() and (seg_len > cc.SP_CHUNK).sum() >= 16
    assert (g["reads"] != 0).sum(axis=1).tolist() == g["lens"].tolist()
    s = cc.secondary_gather_case()
    assert s["reads"].shape[1] == cc.MAX_LEN + 1 and sorted(set(s["lens"].tolist())) == sorted(cc.gather_lengths)
    assert (s["reads"] != 0).sum(axis=1).tolist() == s["lens"].tolist()
    assert np.array_equal(s["base"][cc.A0:cc.A0 + cc.LN], s["base"][cc.B0:cc.B0 + cc.LN])
    short = s["lens"] <= 8191
    assert int(cc.round16(int(s["lens"][short].max()) + 1)) == 2 * cc.SP_CHUNK and short.sum() >= 4 * 7
    reads, lens = cc.long_chimeras(g["ref"])
    assert lens.max() <= cc.MAX_LEN and lens.min() > 4096 + 2500
