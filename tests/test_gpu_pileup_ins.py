"""The insertion columns of the pileup on the GPU (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus"):
pileup_add_ins_kernel on the constructed rows of tests/pileup_ins_cases.py against tests/pileup_ins_ref.py, next to a plain
accumulator fed the same batches; accumulation and reset; the insertion read-back and the polish kernels around the tiles,
for every cap, inside fill; the site alleles against the host rule; the planted workload through DeviceMapper.  Everything
is compared for equality."""
import ctypes as C

import numpy as np
import pytest

import pileup_call_cases as KC
import pileup_call_ref as R
import pileup_cases as PC
import pileup_ins_cases as K
import pileup_ins_ref as IR
import test_gpu_pileup as P
import test_gpu_pileup_sites as S
import test_pileup_ins_cpu as H
import workloads
from longreadmapper_amd import capi, index, mapper, textio
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu
SMALL = dict(lc_long_max=13)
LO, HI, W = K.LO, K.HI, K.HI - K.LO
TILE = capi.PILEUP_TILE
FILL8, FILL32, GUARD = 0xAB, 0xABABABAB, 0xC5C5C5C5
LOOSE = (1, 1, 1, 0)              # one read is a depth, and one inserting read of one is a majority


class Acc(S.Acc):
    """S.Acc over an accumulator with ins_cols insertion columns: the insertion words, the polish and the site alleles, every
    output inside fill that is checked."""

    def __init__(self, di, lo, hi, ins_cols):
        self.h = C.c_void_p()
        capi.check(lib.lrm_pileup_create_ins(C.byref(self.h), di.handle, lo, hi, ins_cols), "lrm_pileup_create_ins")
        self.lo, self.hi, self.W, self.K = lo, hi, hi - lo, ins_cols
        assert lib.lrm_pileup_ins_cols(self.h) == ins_cols

    def ins_raw(self):
        """the insertion planes and the 16 guard words behind them"""
        out = np.zeros(4 * self.K * self.W + 16, dtype=np.uint32)
        capi.check(lib.lrm_debug_pileup_ins_raw(self.h, out.ctypes.data, len(out), P._stream()), "lrm_debug_pileup_ins_raw")
        return out

    def ins_words(self, first=0, count=None):
        """-> (count, K, 4), after checking that the fill either side is untouched"""
        import torch
        count = self.W - first if count is None else count
        pad = 8
        buf = torch.from_numpy(np.full(4 * self.K * count + 2 * pad, FILL32, dtype=np.uint32).view(np.int32)).cuda()
        capi.check(lib.lrm_pileup_ins_read_dev(self.h, first, count, buf.data_ptr() + 4 * pad, P._stream()), "lrm_pileup_ins_read_dev")
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint32)
        assert (got[:pad] == FILL32).all() and (got[pad + 4 * self.K * count:] == FILL32).all(), (first, count)
        return got[pad:pad + 4 * self.K * count].reshape(count, self.K, 4)

    def polish(self, first=0, count=None, opt=None, cap=None, pad=16):
        """-> (the bytes written, the total); nothing from cap on, nothing outside, the length word between two words of fill"""
        import torch
        count = self.W - first if count is None else count
        cap = (self.K + 1) * count + 1 if cap is None else cap
        buf = torch.from_numpy(np.full(cap + 2 * pad, FILL8, dtype=np.uint8)).cuda()
        total = torch.from_numpy(np.full(3, -1, dtype=np.int64)).cuda()
        o = capi.PileupCallOptions(*opt) if opt is not None else None
        capi.check(lib.lrm_pileup_polish_dev(self.h, C.byref(o) if o is not None else None, first, count, buf.data_ptr() + pad if cap else None, cap,
                                             total.data_ptr() + 8, P._stream()), "lrm_pileup_polish_dev")
        torch.cuda.synchronize()
        t, b = total.cpu().numpy(), buf.cpu().numpy()
        assert t[0] == -1 and t[2] == -1, (first, count)
        k = min(int(t[1]), cap)
        assert (b[:pad] == FILL8).all() and (b[pad + k:] == FILL8).all(), (first, count, cap, int(t[1]))
        return bytes(b[pad:pad + k]), int(t[1])

    def alleles(self, sites, opt=None):
        """sites: PILEUP_SITE_DT records -> PILEUP_INS_ALLELE_DT records, the fill either side checked"""
        import torch
        n, pad = len(sites), 2
        d_sites = torch.from_numpy(np.ascontiguousarray(sites).view(np.uint8).copy()).cuda() if n else torch.zeros(32, dtype=torch.uint8).cuda()
        out = torch.from_numpy(np.full(16 * (n + 2 * pad), FILL8, dtype=np.uint8)).cuda()
        o = capi.PileupCallOptions(*opt) if opt is not None else None
        capi.check(lib.lrm_pileup_site_alleles_dev(self.h, C.byref(o) if o is not None else None, d_sites.data_ptr(), n, out.data_ptr() + 16 * pad,
                                                   P._stream()), "lrm_pileup_site_alleles_dev")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:16 * pad] == FILL8).all() and (got[16 * (pad + n):] == FILL8).all()
        return got[16 * pad:16 * (pad + n)].view(capi.PILEUP_INS_ALLELE_DT)


@pytest.fixture(scope="module")
def ont(gpu):
    sc = workloads.scenario("ont-2k")
    di = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL)
    yield di, bytes(sc["hi"].content())
    di.close()


@pytest.fixture(scope="module")
def want_rows():
    """the reference over all constructed rows for every K, computed once and left unchanged"""
    return {ins_cols: H.ref_ins(K.ROWS, ins_cols) for ins_cols in K.KS}


# ---------------------------------------------------------------------------------------------------------
# the add
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ins_cols,read_off", [(1, 0), (1, 7), (4, 1), (4, 14), (8, 3), (8, 9), (8, 15)])
def test_rows_on_the_kernel(ont, want_rows, ins_cols, read_off):
    """every constructed row in one launch; read rows at a base moved by read_off, store rows at strides of every residue mod 4"""
    di, _ = ont
    ref = want_rows[ins_cols]
    stride, store_off = 3201 + read_off % 4 + 4 * (read_off % 3), (5 * read_off) % 16
    acc, plain = Acc(di, LO, HI, ins_cols), P.Acc(di, LO, HI)
    try:
        n_tiles = (W + TILE - 1) // TILE
        assert lib.lrm_pileup_bytes(plain.h) == 32 * W + 4 + 64 + 8 * n_tiles
        assert lib.lrm_pileup_bytes(acc.h) == lib.lrm_pileup_bytes(plain.h) + 16 * ins_cols * W + 64
        for a in (acc, plain):
            a.add(P._batch(K.ROWS, stride, store_off, 3200 + read_off, read_off))
        raw = acc.ins_raw()
        assert np.array_equal(raw[:-16], ref.planes()) and (raw[-16:] == GUARD).all(), (ins_cols, read_off)
        assert np.array_equal(acc.ins_words(), ref.words())
        for first, count in ((0, 1), (W - 1, 1), (TILE - 1, 3), (333, 2 * TILE), (W, 0)):
            assert np.array_equal(acc.ins_words(first, count), ref.words(first, count)), (first, count)
        # everything else is what a plain accumulator holds, guard words included
        first_alloc = acc.raw()
        assert np.array_equal(first_alloc, plain.raw()) and (first_alloc[-16:] == GUARD).all() and first_alloc[W + 1:-16].any()
        assert np.array_equal(acc.ins_raw(), raw)                      # the read-backs leave the planes as they are
        # the invariant on column 0
        n_ins = first_alloc[W + 1 + 6 * W:W + 1 + 7 * W].astype(np.int64)
        assert np.array_equal(ref.words()[:, 0, :].astype(np.int64).sum(axis=1) + ref.col0_other, n_ins)
    finally:
        acc.close()
        plain.close()


def test_contention_accumulation_and_reset(ont, want_rows):
    di, _ = ont
    by = {c.name: c for c in K.ROWS}
    hot = by["random-3199"]._replace(loc=LO + 50)
    one = H.ref_ins([hot], 8).words().astype(np.int64)
    assert one.sum() > 200
    acc = Acc(di, LO, HI, 8)
    try:
        acc.add(P._batch([hot] * 64, stride=3200, read_stride=3200))     # 64 wavefronts add to the same words in one launch
        assert np.array_equal(acc.ins_words().astype(np.int64), 64 * one)
        acc.add(P._batch([by["run-of-9"]._replace(loc=LO + 50)] * 64, stride=64, read_stride=64))      # 64 rows onto one position
        spot = H.ref_ins([by["run-of-9"]._replace(loc=LO + 50)], 8).words().astype(np.int64)
        assert spot.sum() == 8 and np.array_equal(acc.ins_words().astype(np.int64), 64 * (one + spot))
        acc.reset()
        assert not acc.ins_raw()[:-16].any() and not acc.raw()[:-16].any() and (acc.ins_raw()[-16:] == GUARD).all() and (acc.raw()[-16:] == GUARD).all()
        # two adds equal the sum; an empty batch adds nothing
        half = len(K.ROWS) // 2
        acc.add(P._batch([c._replace(last=False) for c in K.ROWS[:half]], stride=3216, read_stride=3200))
        assert np.array_equal(acc.ins_words(), H.ref_ins(K.ROWS[:half], 8).words())
        acc.add(P._batch(K.ROWS[half:], stride=3216, read_stride=3200))
        acc.add(P._batch(K.ROWS, stride=3216, read_stride=3200), n=0)
        assert np.array_equal(acc.ins_words(), want_rows[8].words())
        # without mapq records nothing is filtered
        acc.reset()
        acc.add(P._batch(K.ROWS, stride=3216, read_stride=3200), mapq=False)
        ref = IR.InsPileup(LO, HI, 8)
        for c in K.ROWS:
            ref.add(PC.effective_ops(c), c.read, c.loc, c.score, c.meta_r)
        assert np.array_equal(acc.ins_words(), ref.words()) and ref.c.sum() > want_rows[8].c.sum()
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# the polish and the insertion read-back around the tiles
# ---------------------------------------------------------------------------------------------------------
PW = 2 * TILE + 5


def _ins_row(p, bases):
    """one row whose 'I' run of len(bases) opens behind position p, the row's last target column"""
    return PC.Case("I*%d@%d" % (len(bases), p), b"===" + b"I" * len(bases), b"AAA" + bases, p - 2, 5, 1, 60, None, False, None)


def _polish_rows(lo, ins_cols):
    """rows over the window [lo, lo + PW): -> (rows, what they are meant to produce)"""
    rng = np.random.default_rng(31)
    letters = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))
    rows = []
    # tile 0: covered by '=' from position 100 to ten short of its end; an insertion on the tile's last position; three deleted
    # positions, the last of them with an insertion behind it ('-' next to a position of K bytes), at positions 42 .. 44
    rows.append(PC.Case("eq", b"=" * (TILE - 110), letters(TILE - 110), lo + 100, 5, 1, 60, None, False, None))
    rows.append(_ins_row(lo + TILE - 1, letters(9)))
    rows.append(PC.Case("D-then-I", b"==" + b"DDD" + b"I" * 8 + b"==", letters(12), lo + 40, 5, 1, 60, None, False, None))
    # tile 1: a whole round of deletions (positions 256 .. 511 of the tile); a round where every position is followed by a
    # run of ins_cols + 2 inserted bases (positions 768 .. 1023): every thread emits K + 1 bytes
    rows.append(S._run_of_d(lo + TILE + 256, 256))
    n = ins_cols + 2
    rows.append(PC.Case("every-position-inserts", (b"=" + b"I" * n) * 256, letters((n + 1) * 256), lo + TILE + 768, 5, 1, 60, None, False, None))
    # the last tile (5 positions): an insertion on the range's last position
    rows.append(_ins_row(lo + PW - 1, letters(3)))
    rows.append(_ins_row(lo + PW - 1, b"ACG"))
    return rows


@pytest.mark.parametrize("ins_cols", [8, 4, 1, 0])
def test_polish_around_the_tiles(ont, ins_cols):
    di, content = ont
    lo = LO
    rows = _polish_rows(lo, max(ins_cols, 1))
    acc = Acc(di, lo, lo + PW, ins_cols)
    try:
        acc.add(P._batch(rows, stride=3205, read_stride=3201, read_off=3))
        cols = acc.read()
        words = acc.ins_words() if ins_cols else None
        text = content[lo:lo + PW]
        if ins_cols:
            ref = IR.InsPileup(lo, lo + PW, ins_cols)
            for c in rows:
                ref.add(c.ops, c.read, c.loc)
            assert np.array_equal(words, ref.words())
        for opt in (LOOSE, None):
            o = R.options(*(opt or (0, 0, 0, 0)))
            want = IR.polish(cols, words, text, o)
            per = [len(IR.polish(cols[g:g + 1], None if words is None else words[g:g + 1], text[g:g + 1], o)) for g in range(PW)]
            starts = np.concatenate([[0], np.cumsum(per)])
            if opt == LOOSE:
                # the rows produced what the test is about
                assert per[TILE - 1] == 1 + ins_cols and per[PW - 1] == 1 + min(ins_cols, 3) and per[:40] == [1] * 40      # 'N' stays
                assert per[TILE + 256:TILE + 512] == [0] * 256 and per[TILE + 768:TILE + 1024] == [ins_cols + 1] * 256
                assert per[42:45] == [0, 0, ins_cols] and want[:40] == b"N" * 40
            got, total = acc.polish(opt=opt)
            assert total == len(want) and got == want, (ins_cols, opt)
            for first, count in ((0, PW), (TILE - 1, 2), (TILE, TILE), (TILE + 300, 700), (TILE + 800, 1), (PW - 1, 1), (17, 0), (PW, 0)):
                sub = want[starts[first]:starts[first + count]]
                got, total = acc.polish(first, count, opt)
                assert total == len(sub) and got == sub, (ins_cols, opt, first, count)
                if ins_cols:
                    assert np.array_equal(acc.ins_words(first, count), words[first:first + count]), (first, count)
            for first, count in ((0, PW), (TILE + 700, 600)):
                sub = want[starts[first]:starts[first + count]]
                in_tile = starts[min(((first // TILE) + 1) * TILE, first + count)] - starts[first]      # the bytes of the range's first tile
                for cap in sorted({c for c in (0, 1, in_tile - 1, in_tile, in_tile + 1, len(sub) - 1, len(sub), len(sub) + 1, len(sub) + 300) if c >= 0}):
                    got, total = acc.polish(first, count, opt, cap=cap)
                    assert total == len(sub) and got == sub[:cap], (ins_cols, opt, first, count, cap)
        # the counters are not modified, and the host rule says the same
        assert np.array_equal(acc.read().view(np.uint32), cols.view(np.uint32)) and (acc.raw()[-16:] == GUARD).all()
        if ins_cols:
            assert np.array_equal(acc.ins_words(), words) and (acc.ins_raw()[-16:] == GUARD).all()
        assert H.host_polish(cols, words, text, LOOSE)[0] == IR.polish(cols, words, text, R.options(*LOOSE))
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# the site alleles
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ins_cols", [8, 4, 1])
def test_site_alleles(ont, ins_cols):
    di, content = ont
    acc = Acc(di, LO, HI, ins_cols)
    try:
        rows = [c for c in K.ROWS if c.name.startswith(("run-of-", "random-", "run-cut-by", "read-"))] + _polish_rows(LO + 4000, ins_cols)
        acc.add(P._batch(rows, stride=3205, read_stride=3201))
        words = acc.ins_words()
        for opt in (LOOSE, (2, 1, 30, 0)):
            sites, total, _ = acc.sites(opt=opt, cons=False)
            assert total == len(sites) > (300 if opt == LOOSE else 0)
            recs = np.zeros(total + 3, dtype=capi.PILEUP_SITE_DT)
            for k, s in enumerate(sites):
                recs[k] = s
            # records whose pos lies outside the window: all-zero alleles
            recs[total:] = recs[:3]
            recs["pos"][total:] = [LO - 1, HI, 2**40]
            got = acc.alleles(recs, opt)
            o = R.options(*opt)
            want, host = [], []
            for s in sites:
                w = words[s[0] - LO]
                want.append(IR.allele(s[1], s[5], w, o))
                host.append(H.host_allele(s[1], s[5], w, opt))
            assert [IR.allele_tuple(r) for r in got[:total]] == want == host, (ins_cols, opt)
            assert not got[total:].view(np.uint8).any()
            if opt == LOOSE:
                assert {t[1] for t in want} >= {0, 1, ins_cols} and {t[2] for t in want} >= {0, IR.ENTERS | IR.FULL}
        assert len(acc.alleles(recs[:0])) == 0
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# through DeviceMapper: the planted workload
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(P.MODES))
def test_device_mapper_polish(gpu, mode, tmp_path):
    import torch
    w = KC.planted()
    hi = index.HostIndex.build([w["text"]], names=["planted"], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    n, stride = w["reads"].shape
    window = index.text_window(hi, 0)
    lo = window[0]
    dm = mapper.DeviceMapper(di, n, stride - 1, 20, 300, device=gpu, pileup=window, pileup_ins_cols=8, **P.MODES[mode])
    try:
        d_reads = torch.from_numpy(w["reads"]).cuda()
        d_lens = torch.from_numpy(w["lens"].astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        torch.cuda.synchronize()
        cols, words = dm.pileup_columns(), dm.pileup_ins_columns()
        assert words.shape == (window[1] - window[0], 8, 4) and words.dtype == np.uint32
        content = bytes(hi.content()[window[0]:window[1]])
        got = dm.pileup_polish()
        want, total, _ = H.host_polish(cols, words, content)
        assert got.dtype == np.uint8 and bytes(got) == want and total == len(want), mode
        a, b = 6000, 194000
        part = bytes(dm.pileup_polish(a, b - a, cap=1000))                 # a first buffer that is too small: the retry path
        assert part == H.host_polish(cols[a:b], words[a:b], content[a:b])[0]
        copy = H.copy_slice(w, a, b)
        if mode == "classic":
            assert part == copy and len(part) == 187_995
        # the 80-base slices around the 60 planted variants
        same = 0
        for p in sorted(p for p, _ in w["snv"] + w["dels"] + w["ins"]):
            same += H.host_polish(cols[p - 40:p + 40], words[p - 40:p + 40], content[p - 40:p + 40])[0] == H.copy_slice(w, p - 40, p + 40)
        print("%s: %d of the 60 planted variants' 80-base slices reproduce the copy; whole slice equal: %s" % (mode, same, part == copy))
        # the alleles of the sites, against the host rule; the writers
        sites, n_sites, _ = dm.pileup_sites()
        alleles = dm.pileup_site_alleles(sites)
        assert alleles.dtype == capi.PILEUP_INS_ALLELE_DT and len(alleles) == n_sites
        assert [IR.allele_tuple(r) for r in alleles] == [H.host_allele(int(s["depth"]), int(s["n_ins"]), words[int(s["pos"]) - lo], None) for s in sites]
        assert textio.write_sites(str(tmp_path / "s.tsv"), hi, sites, alleles=alleles) == n_sites
        back = [l.split("\t") for l in open(tmp_path / "s.tsv").read().splitlines()]
        assert [f[11] for f in back] == [bytes(r["bases"][:int(r["len"])]).decode() or "." for r in alleles]
        if mode == "classic":                                              # no insertion is called away from a planted one
            called = [int(s["pos"]) - lo for s, r in zip(sites, alleles) if int(r["flags"]) & capi.INS_ENTERS and int(r["len"])]
            assert len(called) >= len(w["ins"]) and all(min(abs(q - p) for p, _ in w["ins"]) <= 10 for q in called), called
    finally:
        dm.close()
        di.close()
        hi.close()


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------
def test_refusals(ont):
    import torch
    di, content = ont
    h = C.c_void_p()
    assert lib.lrm_pileup_create_ins(C.byref(h), di.handle, LO, HI, 9) < 0 and b"insertion columns" in lib.lrm_last_error() and not h
    assert lib.lrm_pileup_create_ins(C.byref(h), di.handle, HI, HI, 4) < 0 and b"is empty" in lib.lrm_last_error() and not h
    zero, plain = Acc(di, LO, HI, 0), P.Acc(di, LO, HI)
    acc = Acc(di, LO, HI, 4)
    try:
        # ins_cols == 0 is lrm_pileup_create exactly
        assert lib.lrm_pileup_bytes(zero.h) == lib.lrm_pileup_bytes(plain.h) == 32 * W + 4 + 64 + 8 * ((W + TILE - 1) // TILE)
        buf = torch.from_numpy(np.full(4096, FILL8, dtype=np.uint8)).cuda()
        n_out = torch.from_numpy(np.full(2, -1, dtype=np.int64)).cuda()
        st = P._stream()
        for a in (zero, plain):
            assert lib.lrm_pileup_ins_cols(a.h) == 0
            assert lib.lrm_pileup_ins_read_dev(a.h, 0, 10, buf.data_ptr(), st) < 0 and b"no insertion planes" in lib.lrm_last_error()
            assert lib.lrm_pileup_site_alleles_dev(a.h, None, buf.data_ptr(), 1, buf.data_ptr() + 64, st) < 0 and b"no insertion planes" in lib.lrm_last_error()
            assert lib.lrm_debug_pileup_ins_raw(a.h, buf.data_ptr(), 1, st) < 0
        assert lib.lrm_pileup_ins_read_dev(acc.h, W - 1, 2, buf.data_ptr(), st) < 0 and b"outside a window" in lib.lrm_last_error()
        assert lib.lrm_pileup_ins_read_dev(acc.h, 0, 2, buf.data_ptr() + 8, st) < 0 and b"16-byte aligned" in lib.lrm_last_error()
        assert lib.lrm_pileup_ins_read_dev(acc.h, 0, 2, None, st) < 0 and b"null argument" in lib.lrm_last_error()
        polish = lambda **kw: lib.lrm_pileup_polish_dev(acc.h, kw.get("opt"), kw.get("first", 0), kw.get("count", 10), kw.get("seq", buf.data_ptr()),
                                                        kw.get("cap", 100), kw.get("total", n_out.data_ptr()), st)
        assert polish(first=W, count=1) < 0 and b"outside a window" in lib.lrm_last_error()
        assert polish(opt=C.byref(capi.PileupCallOptions(0, 0, 101, 0))) < 0 and b"min_pct" in lib.lrm_last_error()
        assert polish(opt=C.byref(capi.PileupCallOptions(0, 0, 0, 5))) < 0 and b"reserved" in lib.lrm_last_error()
        assert polish(total=None) < 0 and polish(seq=None) < 0 and b"null argument" in lib.lrm_last_error()
        assert polish(total=n_out.data_ptr() + 4) < 0 and b"8-byte aligned" in lib.lrm_last_error()
        assert lib.lrm_pileup_site_alleles_dev(acc.h, None, buf.data_ptr() + 8, 1, buf.data_ptr() + 64, st) < 0 and b"16-byte aligned" in lib.lrm_last_error()
        assert lib.lrm_pileup_site_alleles_dev(acc.h, None, None, 1, buf.data_ptr(), st) < 0
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == FILL8).all() and (n_out.cpu().numpy() == -1).all()      # no kernel ran
        created = acc.bytes()
        assert acc.polish(0, 0)[1] == 0 and acc.bytes() == created                            # count == 0: no scratch either
        assert acc.polish()[0] == b"N" * W and acc.bytes() == created + 8 * ((W + TILE - 1) // TILE)
        assert zero.polish()[0] == b"N" * W
    finally:
        for a in (zero, plain, acc):
            a.close()
