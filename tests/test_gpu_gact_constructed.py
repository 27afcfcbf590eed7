"""The extension kernels on constructed alignments (tests/gact_cases.py).  Expected values come from tests/gact_ref.py,
the specification in executable form; tests/test_gact_constructed_cpu.py shows on the CPU that they are also the
oracle's.  One process, one device, sequential calls.

Per pair through lrm_debug_gact_impl (one job, so the case's own tile decides everything its wavefront decides; the
same cases beside live neighbours, m != n included, are in tests/test_gpu_gact_company.py through the job-table tap
lrm_debug_gact_jobs), and in batches through lrm_extend_batch on an index of a text the test built, with best[] rows
the test wrote: the path the product takes, where the bit-sliced kernel reads its target window out of the index's
planar text at whatever locus and strand the key names."""
import ctypes as C

import numpy as np
import pytest

import constructed
import gact_cases
import gact_ref
from longreadmapper_amd import capi, index, mapper

pytestmark = pytest.mark.gpu

BYTE, BYTE3, BITSLICED = 1, 3, 4                     # lrm_map_options.gact_impl


def _gpu_gact(q, d, T, O, W, impl):
    qa = np.frombuffer(q, dtype=np.uint8)
    da = np.frombuffer(d, dtype=np.uint8)
    ops = np.zeros(len(q) + len(d) + 16, dtype=np.uint8)
    n_ops, score = C.c_int(), C.c_int()
    capi.check(capi.lib.lrm_debug_gact_impl(qa.ctypes.data, len(q), da.ctypes.data, len(d), capi.GactParams(T, O, W), impl,
                                            ops.ctypes.data, C.byref(n_ops), C.byref(score), 0), "lrm_debug_gact_impl")
    return score.value, bytes(ops[:n_ops.value])


@pytest.fixture(scope="module")
def named():
    return [(c, gact_ref.align(c["q"], c["d"], c["T"], c["O"], c["W"])[:2]) for c in gact_cases.cases()]


@pytest.mark.parametrize("impl", [BYTE, BYTE3, BITSLICED])
def test_named_cases_per_kernel(gpu, named, impl):
    """Bands above 128 diagonals run on gact_wide_kernel whatever is asked for: they are in the impl = 1 pass only."""
    n = 0
    for c, want in named:
        if c["W"] > 128 and impl != BYTE:
            continue
        assert _gpu_gact(c["q"], c["d"], c["T"], c["O"], c["W"], impl) == want, c["name"]
        n += 1
    assert n > 600


@pytest.mark.parametrize("impl", [BYTE, BYTE3, BITSLICED])
def test_ragged_exhaustive_sample_per_kernel(gpu, impl):
    pairs = gact_cases.exhaustive_ragged()
    rng = np.random.default_rng(17)
    for p in gact_cases.EXHAUSTIVE_PARAMS:
        pick = [pairs[k] for k in rng.choice(len(pairs), size=80, replace=False)]
        for (q, d), want in zip(pick, gact_ref.align_many(pick, *p)):
            assert _gpu_gact(q, d, *p, impl) == want[:2], (p, q, d)


# ---------------------------------------------------------------------------------------------------------------------
# batches through lrm_extend_batch
# ---------------------------------------------------------------------------------------------------------------------
def _extend(di, reads, keys, gact, stride=None):
    arr, lens = gact_cases.read_matrix(reads, stride)
    best = np.zeros(len(lens), dtype=mapper.ENTRY_DT)
    best["key"] = np.array(keys, dtype=np.uint64)
    got = mapper.extend_batch(di, arr, lens, best, gact)
    return got, arr, lens


def _same(got, k, want):
    return int(got["score"][k]) == want[0] and int(got["n_ops"][k]) == len(want[1]) and \
        bytes(got["ops"][k, :len(want[1])]) == want[1]


@pytest.fixture(scope="module")
def square(gpu):
    pairs = gact_cases.exhaustive_square()
    b = gact_cases.batch_of(pairs)
    hi = index.HostIndex.build(b["seqs"], hlen=8)
    di = index.DeviceIndex.upload(hi, gpu)
    yield pairs, b, di
    di.close()


@pytest.mark.parametrize("T,O,W", gact_cases.EXHAUSTIVE_PARAMS)
def test_square_exhaustive_batch(square, map_options, T, O, W):
    """26 212 reads in one call: above LRM_BS_MIN_READS, so gact_impl = 0 is the bit-sliced kernel by the automatic choice."""
    pairs, b, di = square
    want = gact_ref.align_many(pairs, T, O, W)
    for impl in (0, BYTE3):
        map_options(di, gact_impl=impl)
        got, arr, lens = _extend(di, b["reads"], b["keys"], (T, O, W))
        assert (got["meta_r"] == 1).all() and (got["meta"]["strand"] == 0).all()
        assert np.array_equal(got["meta"]["off"], np.array(b["keys"], dtype=np.uint64))
        bad = [k for k in range(len(pairs)) if not _same(got, k, want[k])]
        assert not bad, (impl, len(bad), pairs[bad[0]])


def test_automatic_dispatch_takes_the_bitsliced_kernel(square, gpu):
    """The same batch device-resident with launch timing: at >= 16 384 reads and gact_impl = 0 the record shows
    gact_bs_kernel, and not the byte kernel."""
    import torch
    pairs, b, di = square
    di.set_map_options()
    arr, lens = gact_cases.read_matrix(b["reads"], 9)
    n = len(lens)
    assert n >= 16384
    dm = mapper.DeviceMapper(di, n, 8, device=gpu)
    dm.set_timing(True)
    dm.best[:, 0] = torch.from_numpy(np.array(b["keys"], dtype=np.int64)).cuda()
    d_reads = torch.from_numpy(arr).cuda()
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    dm.extend(d_reads, d_lens)
    torch.cuda.synchronize()
    t = dm.timing()
    assert t["gact_bs_kernel"][1] == 1 and t["bs_pack_reads_kernel"][1] == 1 and t["gact_kernel"][1] == 0
    res = dm.results(n)
    want = gact_ref.align_many(pairs, 320, 120, 128)
    assert all(_same(res, k, want[k]) for k in range(n))
    dm.close()


@pytest.fixture(scope="module")
def ragged(gpu):
    """The long named cases made square (the window is as long as the read) among thousands of 1 .. 6 base reads, fixed
    shuffle; every 53rd read carries an N or a lower-case base, which sends it to the byte kernel."""
    rng = np.random.default_rng(23)
    long_ = [c for c in gact_cases.cases() if 1000 <= len(c["q"]) <= 2600 and c["W"] <= 128][:40]
    pairs = []
    for c in long_:
        q, d = c["q"], c["d"]
        d = (d + gact_cases.rnd(len(q), "pad", c["name"]))[:len(q)]
        pairs.append((q, d))
    small = [p for p in gact_cases.exhaustive_square() if len(p[0]) <= 6]
    pairs += [small[k] for k in rng.choice(len(small), size=4000, replace=False)]
    pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    marked = []
    for k in range(5, len(pairs), 53):
        q = bytearray(pairs[k][0])
        at = int(rng.integers(0, len(q)))
        q[at] = ord("N") if (k // 53) % 2 else q[at] | 0x20
        pairs[k] = (bytes(q), pairs[k][1])
        marked.append(k)
    b = gact_cases.batch_of(pairs)
    hi = index.HostIndex.build(b["seqs"], hlen=8)
    di = index.DeviceIndex.upload(hi, gpu)
    yield pairs, b, di, marked
    di.close()


@pytest.mark.parametrize("T,O,W", [(320, 120, 128), (64, 16, 32)])
def test_ragged_batch_refills_lanes(ragged, map_options, T, O, W):
    pairs, b, di, marked = ragged
    want = gact_ref.align_many(pairs, T, O, W)
    assert len(marked) > 60 and sum(len(q) >= 1000 for q, _ in pairs) >= 20
    runs = {}
    for name, opts in (("byte", dict(gact_impl=BYTE3)), ("bs-1", dict(gact_impl=BITSLICED, bs_waves=1)),
                       ("bs-2", dict(gact_impl=BITSLICED, bs_waves=2)), ("bs", dict(gact_impl=BITSLICED))):
        map_options(di, **opts)
        got, arr, lens = _extend(di, b["reads"], b["keys"], (T, O, W))
        runs[name] = got
        assert (got["meta_r"] == 1).all()
        bad = [k for k in range(len(pairs)) if not _same(got, k, want[k])]
        assert not bad, (name, len(bad), bad[:5], [k in marked for k in bad[:5]])
    for k in marked:            # the reads the bit-sliced kernel hands to the byte kernel: the byte kernel's own answer
        for name in ("bs-1", "bs-2", "bs"):
            assert bytes(runs[name]["ops"][k]) == bytes(runs["byte"]["ops"][k])


@pytest.fixture(scope="module")
def packing(gpu):
    pb = gact_cases.packing_batch()
    hi = index.HostIndex.build(pb["seqs"], hlen=8)
    assert bytes(hi.content()) == constructed.index_text(pb["seqs"])
    di = index.DeviceIndex.upload(hi, gpu)
    yield pb, di
    di.close()


@pytest.mark.parametrize("impl", [0, BYTE3, BITSLICED])
@pytest.mark.parametrize("T,O,W", [(320, 120, 128), (64, 16, 32)])
def test_packing_edges(packing, map_options, impl, T, O, W):
    """Every locus residue mod 64 on both strands, windows on the first and last base of each sequence, and windows one
    base beyond: fenced (no extension, score -1, n_ops 0, meta_r 0) without touching their neighbours in the wavefront."""
    pb, di = packing
    map_options(di, gact_impl=impl)
    live = [k for k, w in enumerate(pb["windows"]) if w is not None]
    want = iter(gact_ref.align_many([(constructed.revcomp(pb["reads"][k]) if pb["strand"][k] else pb["reads"][k],
                                      pb["windows"][k]) for k in live], T, O, W))
    got, arr, lens = _extend(di, pb["reads"], pb["keys"], (T, O, W))
    off = np.concatenate([[0], np.cumsum([2 * len(s) for s in pb["seqs"]])])
    n_fenced = 0
    for k in range(len(lens)):
        m = got["meta"][k]
        if pb["windows"][k] is None:
            n_fenced += 1
            assert (int(got["meta_r"][k]), int(got["score"][k]), int(got["n_ops"][k])) == (0, -1, 0), k
            assert (int(m["seq_id"]), int(m["loc"]), int(m["off"]), int(m["strand"])) == (-1, 0, 0, 0), k
            assert bytes(arr[k, :lens[k]]) == pb["reads"][k]
            continue
        assert int(got["meta_r"][k]) == 1 and _same(got, k, next(want)), (k, pb["seq_id"][k], pb["pos"][k], pb["strand"][k])
        assert (int(m["seq_id"]), int(m["strand"]), int(m["off"]), int(m["loc"])) == \
            (pb["seq_id"][k], pb["strand"][k], pb["pos"][k], int(off[pb["seq_id"][k]]) + pb["pos"][k]), k
        assert bytes(arr[k, :lens[k]]) == (constructed.revcomp(pb["reads"][k]) if pb["strand"][k] else pb["reads"][k])
    assert n_fenced == 36
