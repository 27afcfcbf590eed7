"""The pileup on the GPU (docs/GACT_SPEC.md, "Pileup"): pileup_add_kernel and the read-back on the constructed cases of
tests/pileup_cases.py, every record against tests/pileup_ref.py for equality; contention, accumulation, reset; windows either
side of a read-back tile and beyond one round of the tile scan; what must stay untouched; the stage behind the three
extension modes of DeviceMapper, the MAPQ filter, the refusals."""
import ctypes as C

import numpy as np
import pytest

import pileup_cases as K
import pileup_ref
import workloads
from longreadmapper_amd import capi, index, mapper, synth
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu
SMALL = dict(lc_long_max=13)
LO, HI, W = K.LO, K.HI, K.HI - K.LO
TILE = capi.PILEUP_TILE
FILL = 0xABABABAB
GUARD = 0xC5C5C5C5
OUT_PAD = 4                       # records of fill in front of and behind the requested ones


@pytest.fixture(scope="module")
def ont(gpu):
    sc = workloads.scenario("ont-2k")
    di = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL)
    yield sc, di, bytes(sc["hi"].content())
    di.close()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Acc:
    """An lrm_pileup over [lo, hi) of a device index."""

    def __init__(self, di, lo, hi):
        self.h = C.c_void_p()
        capi.check(lib.lrm_pileup_create(C.byref(self.h), di.handle, lo, hi), "lrm_pileup_create")
        self.lo, self.hi, self.W = lo, hi, hi - lo

    def add(self, batch, min_mapq=K.MIN_MAPQ, mapq=True, n=None):
        b = batch
        capi.check(lib.lrm_pileup_add_dev(self.h, b["reads"].data_ptr() + b["read_off"], b["read_stride"], b["lens"].data_ptr(),
                                          b["store"].data_ptr() + b["store_off"], b["stride"], b["n_ops"].data_ptr(), b["score"].data_ptr(),
                                          b["meta_r"].data_ptr(), b["meta"].data_ptr(), b["n"] if n is None else n,
                                          b["mapq"].data_ptr() if mapq else None, min_mapq, _stream()), "lrm_pileup_add_dev")

    def read(self, first=0, count=None):
        """-> the records, after checking that the fill either side of them is untouched"""
        import torch
        count = self.W - first if count is None else count
        buf = torch.from_numpy(np.full((count + 2 * OUT_PAD) * 8, FILL, dtype=np.uint32).view(np.int32)).cuda()
        capi.check(lib.lrm_pileup_read_dev(self.h, first, count, buf.data_ptr() + 32 * OUT_PAD, _stream()), "lrm_pileup_read_dev")
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint32)
        assert (got[:8 * OUT_PAD] == FILL).all() and (got[8 * (OUT_PAD + count):] == FILL).all(), (first, count)
        return got[8 * OUT_PAD:8 * (OUT_PAD + count)].view(capi.PILEUP_COL_DT)

    def raw(self):
        """the counter words and the 16 guard words behind them"""
        out = np.zeros(8 * self.W + 1 + 16, dtype=np.uint32)
        capi.check(lib.lrm_debug_pileup_raw(self.h, out.ctypes.data, len(out), _stream()), "lrm_debug_pileup_raw")
        return out

    def reset(self):
        capi.check(lib.lrm_pileup_reset(self.h, _stream()), "lrm_pileup_reset")

    def close(self):
        if self.h:
            lib.lrm_pileup_free(self.h)
            self.h = None


def _batch(cases, stride=8016, store_off=0, read_stride=8000, read_off=0):
    """The device arrays of a batch of cases.  Store rows at `stride` from a base moved by store_off, every byte that is not
    an op byte of a row is 'X'; read rows at read_stride from a base moved by read_off, every byte that is not a read byte is
    'A', and the buffer ends on the last byte of the last row's read."""
    import torch
    n = len(cases)
    flat = np.full(n * stride + store_off + 64, ord("X"), dtype=np.uint8)
    rd = np.full(read_off + (n - 1) * read_stride + len(cases[-1].read), ord("A"), dtype=np.uint8)
    n_ops, lens = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
    meta, mq = np.zeros(n, dtype=mapper.META_DT), np.zeros(n, dtype=capi.MAPQ_DT)
    for i, c in enumerate(cases):
        assert len(c.ops) <= stride and len(c.read) <= read_stride
        flat[store_off + i * stride:store_off + i * stride + len(c.ops)] = np.frombuffer(c.ops, dtype=np.uint8)
        rd[read_off + i * read_stride:read_off + i * read_stride + len(c.read)] = np.frombuffer(c.read, dtype=np.uint8)
        n_ops[i] = len(c.ops) if c.n_ops is None else c.n_ops
        lens[i], meta["loc"][i], mq["mapq"][i] = len(c.read), c.loc, c.mapq
    mq["n1"], mq["n2"] = 9, 3                                          # (not read by the filter)
    dev = lambda a: torch.from_numpy(a).cuda()
    return dict(n=n, stride=stride, store_off=store_off, read_stride=read_stride, read_off=read_off, store=dev(flat), reads=dev(rd),
                n_ops=dev(n_ops), lens=dev(lens.view(np.int32)), score=dev(np.array([c.score for c in cases], dtype=np.int32)),
                meta_r=dev(np.array([c.meta_r for c in cases], dtype=np.int32)), meta=dev(meta.view(np.uint8).reshape(n, -1).copy()),
                mapq=dev(mq.view(np.uint8).reshape(n, -1).copy()))


def _ref(cases, lo=LO, hi=HI, min_mapq=K.MIN_MAPQ, mapq=True):
    ref = pileup_ref.Pileup(lo, hi)
    for c in cases:
        ref.add(K.effective_ops(c), c.read, c.loc, c.score, c.meta_r, c.mapq if mapq else None, min_mapq)
    return ref


@pytest.fixture(scope="module")
def want_cases():
    """the reference over all constructed cases, computed once and left unchanged"""
    ref = _ref(K.CASES)
    return ref, ref.columns()


def _assert_same(got, want, what=""):
    assert pileup_ref.same(got, want), (what, pileup_ref.first_difference(got, want))


SUB_RANGES = [(0, 1), (W - 1, 1), (1, 17), (TILE - 1, 3), (TILE, TILE), (333, 2 * TILE), (W // 2, 0), (W, 0)]


@pytest.mark.parametrize("read_off", range(16))
def test_cases_on_the_kernel(ont, want_cases, read_off):
    """every case in one launch; read rows at a base moved by 0..15 bytes, store rows at strides of every residue mod 4"""
    _, di, _ = ont
    ref, want = want_cases
    stride, store_off = 8016 + (read_off % 4) * 5, (5 * read_off) % 16
    acc = Acc(di, LO, HI)
    try:
        assert lib.lrm_pileup_bytes(acc.h) == 32 * W + 4 + 64 + 8 * ((W + TILE - 1) // TILE)
        acc.add(_batch(K.CASES, stride, store_off, 8000 + read_off, read_off))
        raw = acc.raw()
        _assert_same(acc.read(), want, read_off)
        for first, count in SUB_RANGES[read_off % 2::2]:
            _assert_same(acc.read(first, count), ref.columns(first, count), (read_off, first, count))
        after = acc.raw()
        assert np.array_equal(raw, after)                              # the read-back leaves the planes as they are
        assert (after[-16:] == GUARD).all() and after[W] == np.uint32(-1 * sum(1 for c in K.CASES if _ends_at_hi(c)) & 0xFFFFFFFF)
        assert np.array_equal(after[W + 1 + 4 * W:W + 1 + 5 * W].astype(np.int64), ref.other())
    finally:
        acc.close()


def _ends_at_hi(c):
    """the case's covered interval, clipped to the window, is not empty and ends at hi: its -1 lies in word W"""
    ops = K.effective_ops(c)
    if not pileup_ref.aligned(ops, c.score, c.meta_r) or c.mapq < K.MIN_MAPQ:
        return False
    return max(c.loc, LO) < min(c.loc + K.span(ops), HI) == HI


def test_without_mapq_records_nothing_is_filtered(ont):
    _, di, _ = ont
    acc = Acc(di, LO, HI)
    try:
        acc.add(_batch(K.CASES), mapq=False)
        _assert_same(acc.read(), _ref(K.CASES, mapq=False).columns())
        acc.reset()
        acc.add(_batch(K.CASES), min_mapq=0)
        _assert_same(acc.read(), _ref(K.CASES, min_mapq=0).columns())
    finally:
        acc.close()


def test_contention_accumulation_and_reset(ont, want_cases):
    _, di, _ = ont
    ref, want = want_cases
    hot = next(c for c in K.CASES if c.name == "n_ops-2049-uniform")
    one = _ref([hot]).columns()
    assert one["n_del"].sum() > 300 and one["n_ins"].sum() > 100 and (one["x_a"].sum() + one["x_c"].sum()) > 100
    acc = Acc(di, LO, HI)
    try:
        acc.add(_batch([hot] * 300))                                   # 300 wavefronts add to the same words in one launch
        got = acc.read()
        for f in pileup_ref.COL_FIELDS:
            assert np.array_equal(got[f].astype(np.int64), 300 * one[f].astype(np.int64)), f
        # two adds equal the sum, and a read-back between them changes nothing
        acc.reset()
        assert not acc.read().view(np.uint32).any() and not acc.raw()[:8 * W + 1].any()
        half = len(K.CASES) // 2
        last = [c._replace(last=False) for c in K.CASES[:half]]
        acc.add(_batch(last))
        _assert_same(acc.read(), _ref(K.CASES[:half]).columns(), "first half")
        acc.add(_batch(K.CASES[half:]))
        _assert_same(acc.read(), want, "both halves")
        acc.add(_batch(K.CASES), n=0)                                  # an empty batch
        _assert_same(acc.read(), want, "an empty batch")
        acc.reset()
        assert not acc.read().view(np.uint32).any() and (acc.raw()[-16:] == GUARD).all()
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# the read-back's tiles
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_text(gpu):
    """a text of 2.2 M positions: room for one tile more than one round of the tile scan holds (1024 tiles)"""
    hi = index.HostIndex.build([synth.reference(1_100_000, seed=77)], hlen=8)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    yield di, int(hi.h.con_len)
    di.close()
    hi.close()


def _sparse_cases(lo, width):
    """short alignments with every kind of event over the window's ends, over every tile edge of a few tiles, and in the last tile"""
    rng = np.random.default_rng(width)
    ops = b"=" * 6 + b"X" + b"==" + b"DD" + b"=" + b"II" + b"=" * 6 + b"X" + b"=" * 10 + b"D" + b"=" * 8
    n_tiles = (width + TILE - 1) // TILE
    at = {lo - 20, lo, lo + width - 20, lo + width - K.span(ops), lo + width, lo + (n_tiles - 1) * TILE + 3}
    for k in sorted({1, 2, 3, n_tiles // 2, 1023, 1024, n_tiles - 1} & set(range(1, n_tiles))):
        at |= {lo + k * TILE - 20, lo + k * TILE - K.span(ops), lo + k * TILE, lo + k * TILE - 1}
    cases = []
    for loc in sorted(a for a in at if a >= 0):
        read = bytes(rng.choice(np.frombuffer(b"ACGTn", dtype=np.uint8), size=K.qlen(ops)))
        cases.append(K.Case("sparse-%d" % loc, ops, read, loc, 5, 1, 60, None, False, None))
    return cases


@pytest.mark.parametrize("width", [TILE - 1, TILE, TILE + 1, 1025 * TILE])
def test_windows_around_the_tiles(long_text, width):
    di, con_len = long_text
    lo = 40_000
    assert lo + width <= con_len
    cases = _sparse_cases(lo, width)
    ref = _ref(cases, lo, lo + width)
    acc = Acc(di, lo, lo + width)
    try:
        acc.add(_batch(cases, stride=64, read_stride=48))
        want = ref.columns()
        _assert_same(acc.read(), want, width)
        # the alignments leave something to see at both ends of the window and of every kind
        assert want["depth"][0] == 2 and want["depth"][-1] >= 2 and want["n_del"].any() and want["n_ins"].any() and (want["depth"] - want["n_eq"] - want["n_del"]).any()
        subs = [(5, width - 9), (width - 100, 100), (width - 1, 1)]
        if width > 2 * TILE:                                           # ranges that start and end inside tiles, in both rounds of the scan
            subs += [(1000, 3000), (1023 * TILE + 5, 2 * TILE - 7 - 5), (1024 * TILE - 1, 2), (1024 * TILE + 77, 100)]
        for first, count in subs:
            _assert_same(acc.read(first, count), ref.columns(first, count), (width, first, count))
        assert (acc.raw()[-16:] == GUARD).all()
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# the stage behind the extension modes
# ---------------------------------------------------------------------------------------------------------
MODES = {"classic": {}, "anchored": dict(anchored=True), "clip": dict(clip=True)}


def _device_run(di, gpu, sc, window, **kw):
    import torch
    n, stride = sc["reads"].shape
    dm = mapper.DeviceMapper(di, n, stride - 1, sc["seed_len"], sc["thres"], device=gpu, pileup=window, **kw)
    d_reads = torch.from_numpy(sc["reads"]).cuda()
    d_lens = torch.from_numpy(sc["lens"].astype(np.int32)).cuda()
    dm.seed(d_reads, d_lens)
    dm.extend(d_reads, d_lens)
    torch.cuda.synchronize()
    res = dm.results(n)
    cols = dm.pileup_columns() if window is not None else None
    return dm, res, d_reads.cpu().numpy(), cols, (d_reads, d_lens)


def _ref_of_results(res, reads_after, lens, lo, hi, min_mapq=None):
    ref = pileup_ref.Pileup(lo, hi)
    for i in range(len(lens)):
        ops = bytes(res["ops"][i, :max(int(res["n_ops"][i]), 0)])
        ref.add(ops, bytes(reads_after[i, :lens[i]]), int(res["meta"]["loc"][i]), int(res["score"][i]), int(res["meta_r"][i]),
                int(res["mapq"]["mapq"][i]) if min_mapq is not None else None, min_mapq or 0)
    return ref


@pytest.mark.parametrize("mode", list(MODES))
def test_device_mapper_pileup(ont, gpu, mode):
    sc, di, content = ont
    di.set_map_options()
    lens = sc["lens"]
    window = (0, len(content))
    dm, res, reads_after, cols, (d_reads, d_lens) = _device_run(di, gpu, sc, window, **MODES[mode])
    try:
        ref = _ref_of_results(res, reads_after, lens, *window)
        want = ref.columns()
        _assert_same(cols, want, mode)
        assert want["depth"].max() >= 2 and want["n_del"].sum() > 100 and want["n_ins"].sum() > 100 and want["x_a"].sum() > 50
        # the rule's premise on the same data: '=' columns agree with the text, 'X' columns differ
        mapped, text = 0, content.upper()
        for i in range(len(lens)):
            ops = bytes(res["ops"][i, :max(int(res["n_ops"][i]), 0)])
            if not pileup_ref.aligned(ops, int(res["score"][i]), int(res["meta_r"][i])):
                continue
            mapped += 1
            loc, read = int(res["meta"]["loc"][i]), bytes(reads_after[i, :lens[i]]).upper()
            for o, (t, q) in zip(ops, K.walk(ops)):
                if o == ord("="):
                    assert read[q] == text[loc + t], (mode, i, t, q)
                elif o == ord("X"):
                    assert read[q] != text[loc + t], (mode, i, t, q)
        assert mapped > 50
        # a sub-range through the Python layer; a second batch adds on top; reset clears
        _assert_same(dm.pileup_columns(1000, 5000), ref.columns(1000, 5000), mode)
        assert dm.pileup_bytes() >= 32 * len(content) + 4
        # (the extension reverse-complements in place: the second pass maps the batch as it was sequenced again)
        import torch
        d_reads.copy_(torch.from_numpy(sc["reads"]).cuda())
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        twice = dm.pileup_columns()
        for f in pileup_ref.COL_FIELDS:
            assert np.array_equal(twice[f].astype(np.int64), 2 * want[f].astype(np.int64)), (mode, f)
        dm.pileup_reset()
        assert not dm.pileup_columns().view(np.uint32).any()
    finally:
        dm.close()
    # a mapper without the accumulator: the same bytes in every other output
    plain_dm, plain, plain_reads, _, _ = _device_run(di, gpu, sc, None, **MODES[mode])
    plain_dm.close()
    assert set(plain) == set(res)
    for key in plain:
        assert np.array_equal(plain[key], res[key]), (mode, key)
    assert np.array_equal(plain_reads, reads_after)


def test_mapq_filter_on_the_two_copy_repeat(gpu):
    """The planted two-copy repeat of the mapping-quality tests: with pileup_min_mapq=1 the reads the vote could not place
    (MAPQ 0) are absent from the pileup."""
    base = synth.reference(400_000, seed=61).copy()
    a0, b0, ln = 50_000, 250_000, 30_000
    base[b0:b0 + ln] = base[a0:a0 + ln]
    hi = index.HostIndex.build([base], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    try:
        r = synth.reads([base], 160, 10_000, synth.ONT, seed=62)
        sc = dict(reads=r["reads"], lens=r["lens"], seed_len=20, thres=300)
        window = (0, int(hi.h.con_len))
        dm, res, reads_after, cols, _ = _device_run(di, gpu, sc, window, mapq=True, pileup_min_mapq=1)
        dm.close()
    finally:
        di.close()
    mq = res["mapq"]["mapq"]
    live = (res["meta_r"] != 0) & (res["score"] != -1) & (res["n_ops"] > 0)
    dropped = np.flatnonzero(live & (mq == 0))
    assert len(dropped) >= 3 and (live & (mq >= 1)).sum() >= 50
    want = _ref_of_results(res, reads_after, sc["lens"], *window, min_mapq=1).columns()
    _assert_same(cols, want)
    # what the filter kept out would have been seen: the MAPQ-0 reads alone cover positions
    only = {k: (v[dropped] if isinstance(v, np.ndarray) else v) for k, v in res.items() if k != "split"}
    assert _ref_of_results(only, reads_after[dropped], sc["lens"][dropped], *window).columns()["depth"].sum() > 10_000 * len(dropped) // 2
    hi.close()


def test_refusals(ont, gpu):
    sc, di, content = ont
    h = C.c_void_p()
    L = len(content)
    assert lib.lrm_pileup_create(C.byref(h), di.handle, 10, L + 1) < 0 and b"ends behind the text" in lib.lrm_last_error() and not h
    assert lib.lrm_pileup_create(C.byref(h), di.handle, 10, 10) < 0 and b"is empty" in lib.lrm_last_error()
    assert lib.lrm_pileup_create(C.byref(h), di.handle, 11, 10) < 0 and b"is empty" in lib.lrm_last_error() and not h
    dg = index.DeviceIndex.upload_multi(sc["hi"], [gpu, gpu], **SMALL)
    try:
        assert lib.lrm_pileup_create(C.byref(h), dg.handle, 0, 100) < 0 and b"group handle" in lib.lrm_last_error() and not h
    finally:
        dg.close()
    acc = Acc(di, L - 100, L)                                           # hi == con_len is allowed
    try:
        b = _batch(K.CASES[:4])
        b["stride"] = (1 << 31) + 1
        with pytest.raises(capi.LrmError, match="store_stride .* above 2\\^31"):
            acc.add(b, n=0)
        import torch
        out = torch.zeros(64, dtype=torch.int32).cuda()
        assert lib.lrm_pileup_read_dev(acc.h, 99, 2, out.data_ptr(), _stream()) < 0 and b"outside a window" in lib.lrm_last_error()
        assert lib.lrm_pileup_read_dev(acc.h, 0, 1, out.data_ptr() + 4, _stream()) < 0 and b"16-byte aligned" in lib.lrm_last_error()
        assert not acc.read().view(np.uint32).any()
    finally:
        acc.close()
