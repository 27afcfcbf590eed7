"""The shared row walk of the stream kernels over op bytes (op_rows.h) on the GPU: aln_summary_kernel, aln_diff_kernel and
pileup_add_kernel on the rows of tests/op_walk_cases.py -- more than two step pairs, runs over the pair edge, the step edge
inside a pair and the edge between the last pair and the tail -- at a row stride that is a multiple of 4 and one that is
not, from a base pointer moved by 0 and by 1; every output against the Python references for equality, outputs in guard
fill.  The store layouts, the launches and the guard checks are the helpers of the three stages' own GPU tests."""
import numpy as np
import pytest

import op_walk_cases as W
import pileup_cases as K
import test_gpu_aln_diff as D
import test_gpu_aln_summary as S
import test_gpu_pileup as P
import workloads
from longreadmapper_amd import index

pytestmark = pytest.mark.gpu
LAYOUTS = [(6148, 0), (6148, 1), (6149, 0), (6149, 1)]                  # (row stride, bytes the base pointer is moved by)


@pytest.fixture(scope="module")
def ont(gpu):
    sc = workloads.scenario("ont-2k")
    di = index.DeviceIndex.upload(sc["hi"], gpu, **P.SMALL)
    yield di, bytes(sc["hi"].content())
    di.close()


@pytest.fixture(scope="module")
def want_columns():
    """the pileup reference over all rows, computed once and left unchanged"""
    ref = P._ref(W.CASES, W.LO, W.HI)
    return ref, ref.columns()


@pytest.mark.parametrize("stride,base_off", LAYOUTS)
def test_summary_records(ont, stride, base_off):
    di, _ = ont
    got = S._kernel_records(di, [(c.ops, c.score, c.meta_r, c.n_ops) for c in W.CASES], stride, base_off)      # (checks the fill behind the records)
    S._same_records(got, [(K.effective_ops(c), c.score, c.meta_r) for c in W.CASES], (stride, base_off))


@pytest.mark.parametrize("stride,base_off", LAYOUTS)
def test_difference_events(ont, stride, base_off):
    di, content = ont
    rows = [(c.ops, c.score, c.meta_r, c.loc, c.n_ops) for c in W.CASES]
    off, buf, want = D._kernel_events(di, content, rows, stride, base_off)
    total = int(off[-1])
    assert (buf[total:] == D.FILL).all()                              # nothing at or beyond off[n]
    bad = [c.name for i, c in enumerate(W.CASES) if buf[int(off[i]):int(off[i + 1])].tolist() != want[i]]
    assert not bad, (stride, base_off, len(bad), bad[:5])
    assert total > 20000 and not want[[c.name for c in W.CASES].index("dead-meta_r-0")]


@pytest.mark.parametrize("stride,base_off", LAYOUTS)
def test_pileup_counts(ont, want_columns, stride, base_off):
    di, _ = ont
    ref, want = want_columns
    width = W.HI - W.LO
    acc = P.Acc(di, W.LO, W.HI)
    try:
        acc.add(P._batch(W.CASES, stride, base_off, 6160 + stride % 5, base_off))
        P._assert_same(acc.read(), want, (stride, base_off))             # (checks the fill either side of the records)
        raw = acc.raw()
        assert (raw[-16:] == P.GUARD).all() and raw[width] == 0          # no row ends at hi: nothing in the last depth word
        assert np.array_equal(raw[width + 1 + 4 * width:width + 1 + 5 * width].astype(np.int64), ref.other())
    finally:
        acc.close()
