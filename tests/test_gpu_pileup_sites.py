"""The call stage of the pileup on the GPU (docs/GACT_SPEC.md, "Pileup calls"): pileup_call_kernel, the site-count scan and
pileup_sites_kernel.  The accumulator is filled through lrm_pileup_add_dev with batches of tiny hand-made rows stacked to the
wanted depth and counts; the expected sites are tests/pileup_call_ref.py applied to lrm_pileup_read_dev's records -- which
tests/test_gpu_pileup.py pins -- and the text.  Sites, totals and cons bytes are compared for equality."""
import ctypes as C

import numpy as np
import pytest

import pileup_call_cases as KC
import pileup_call_ref as R
import pileup_cases as K
import test_gpu_pileup as P
import workloads
from longreadmapper_amd import capi, index, mapper, synth, textio
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu
SMALL = dict(lc_long_max=13)
LO, HI, W = K.LO, K.HI, K.HI - K.LO
TILE = capi.PILEUP_TILE
FILL8 = 0xAB
PAD = 4                           # records of fill in front of and behind the table
LOOSE = (1, 1, 1, 0)              # options under which one 'X', 'D' or opening 'I' column makes a site


class Acc(P.Acc):
    """P.Acc with the call stage: the table lies in 0xAB fill with PAD records of fill either side, the cons buffer with 16
    bytes either side, the count word between two words of fill; everything that must stay untouched is checked."""

    def sites(self, first=0, count=None, opt=None, cap=None, cons=True, null_table=False):
        import torch
        count = self.W - first if count is None else count
        cap = count if cap is None else cap
        table = torch.from_numpy(np.full((cap + 2 * PAD) * 32, FILL8, dtype=np.uint8)).cuda()
        cbuf = torch.from_numpy(np.full(count + 32, FILL8, dtype=np.uint8)).cuda()
        total = torch.from_numpy(np.full(3, -1, dtype=np.int64)).cuda()
        o = capi.PileupCallOptions(*opt) if opt is not None else None
        capi.check(lib.lrm_pileup_sites_dev(self.h, C.byref(o) if o is not None else None, first, count,
                                            None if null_table else table.data_ptr() + 32 * PAD, cap, total.data_ptr() + 8,
                                            cbuf.data_ptr() + 16 if cons else None, P._stream()), "lrm_pileup_sites_dev")
        torch.cuda.synchronize()
        t, tb, cb = total.cpu().numpy(), table.cpu().numpy(), cbuf.cpu().numpy()
        assert t[0] == -1 and t[2] == -1, (first, count)
        n = int(t[1])
        k = min(n, cap)
        assert (tb[:32 * PAD] == FILL8).all() and (tb[32 * (PAD + k):] == FILL8).all(), (first, count, cap, n)    # from cap on, and the fill
        assert (cb[:16] == FILL8).all() and (cb[16 + count:] == FILL8).all(), (first, count)
        if not cons:
            assert (cb == FILL8).all()
        return R.as_tuples(tb[32 * PAD:32 * (PAD + k)].view(capi.PILEUP_SITE_DT)), n, bytes(cb[16:16 + count]) if cons else None

    def bytes(self):
        return int(lib.lrm_pileup_bytes(self.h))


def row(kind, p, byte=b"N"):
    """one tiny row over position p: 'e' "=====", 'x' "==X==" with read byte `byte` on p, 'd' "==D==", 'i' "===I==" whose run
    opens behind p"""
    ops, read = {"e": (b"=====", b"AAAAA"), "x": (b"==X==", b"AA" + byte + b"AA"), "d": (b"==D==", b"AAAA"), "i": (b"===I==", b"AAAAAA")}[kind]
    return K.Case("%s@%d" % (kind, p), ops, read, p - 2, 5, 1, 60, None, False, None)


def stack(c, p):
    """the rows that give position p the record of a constructed case"""
    depth, n_eq, xa, xc, xg, xt, n_del, n_ins = c.col
    rows = []
    for base, n in zip(b"ACGT", (xa, xc, xg, xt)):
        rows += [row("x", p, bytes([base]))] * n
    rows += [row("x", p, b"N")] * c.other + [row("d", p)] * n_del + [row("i", p)] * n_ins + [row("e", p)] * (n_eq - n_ins)
    assert len(rows) == depth
    return rows


def place(cases, content, lo, hi, gap=16):
    """a position for every case: its text byte, residue k mod 16 for case k, `gap` positions from its neighbours"""
    at, p = [], lo + gap
    for k, c in enumerate(cases):
        while content[p] != c.byte or p % 16 != k % 16:
            p += 1
        assert p + gap < hi, "the window is too short for the cases"
        at.append(p)
        p += gap
    return at


def want_of(acc, content, opt=None, sparse=False):
    """the reference over the whole window, from the records the read-back returns"""
    cols = acc.read()
    text = bytes(content[acc.lo:acc.hi])
    return (R.sites_sparse if sparse else R.sites)(cols, text, acc.lo, R.options(*(opt or (0, 0, 0, 0)))), cols


@pytest.fixture(scope="module")
def ont(gpu):
    sc = workloads.scenario("ont-2k")
    di = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL)
    yield di, bytes(sc["hi"].content())
    di.close()


@pytest.fixture(scope="module")
def planted_cases(ont):
    """every plantable constructed case stacked on a position of the window [5000, 12000), in one accumulator that the tests
    read and do not change"""
    di, content = ont
    cases = [c for c in KC.CASES if KC.plantable(c)]
    at = place(cases, content, LO, HI)
    assert {p % 16 for p in at} == set(range(16)) and len(cases) >= 50
    rows = [r for c, p in zip(cases, at) for r in stack(c, p)]
    acc = Acc(di, LO, HI)
    acc.add(P._batch(rows, stride=16, read_stride=16))
    yield acc, cases, at, content
    acc.close()


def test_constructed_cases(planted_cases):
    acc, cases, at, content = planted_cases
    cols = acc.read()
    for c, p in zip(cases, at):                                        # the rows gave every case its record
        assert tuple(int(v) for v in cols[p - LO]) == c.col, c.name
    for opt in sorted({KC_opt(c) for c in cases}):
        (want, want_cons), _ = want_of(acc, content, opt)
        got, total, cons = acc.sites(opt=opt)
        assert total == len(want) and got == want and cons == want_cons, opt
        here = {c.name: R.call(c.col, c.byte, R.options(*opt)) for c in cases if KC_opt(c) == opt}
        by_pos = {s[0]: s for s in got}
        for c, p in zip(cases, at):                                    # ... and the case's own edge is in the device's answer
            if KC_opt(c) == opt:
                kinds, alt, n_alt, letter = here[c.name]
                assert cons[p - LO] == letter and (by_pos[p][6:] == (c.byte, alt, letter, kinds) if kinds else p not in by_pos), c.name
    (want, _), _ = want_of(acc, content)
    assert {s[9] for s in want} == {1, 2, 3, 4, 5, 6, 7} and len(want) > 20
    assert acc.sites(opt=None)[0] == want                              # opt == NULL: the defaults


def KC_opt(c):
    return (c.opt.get("min_depth", 0), c.opt.get("min_count", 0), c.opt.get("min_pct", 0), 0)


# ---------------------------------------------------------------------------------------------------------
# the tiles
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_text(gpu):
    """the 2.2 M-position text of test_gpu_pileup.test_windows_around_the_tiles"""
    hi = index.HostIndex.build([synth.reference(1_100_000, seed=77)], hlen=8)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    yield di, bytes(hi.content())
    di.close()
    hi.close()


def _other_base(b):
    return bytes([b"ACGT"[(b"ACGT".index(b) + 1) % 4]])


def _run_of_d(first, n):
    """one row whose n 'D' columns fall on positions first .. first + n - 1"""
    ops = b"=" + b"D" * n + b"="
    return K.Case("D*%d@%d" % (n, first), ops, b"AA", first - 1, 5, 1, 60, None, False, None)


def _tile_rows(lo, width, content):
    """-> (rows, what they are meant to produce).  Single sites alternate between the three kinds."""
    n_tiles = (width + TILE - 1) // TILE
    singles, runs = {lo, lo + width - 1}, []
    if n_tiles <= 2:
        singles.add(lo + 300)
        if width >= TILE:
            runs.append((lo, TILE))                                    # tile 0: 2048 sites, the window's first position among them
        else:
            runs.append((lo + 512, 256))                               # every position of one round of tile 0
    else:
        for k in (1, 2, 1023, 1024, n_tiles - 1):
            singles |= {lo + k * TILE - 1, lo + k * TILE}
        runs += [(lo + 4 * TILE + 512, 256), (lo + 6 * TILE, TILE), (lo + 1024 * TILE + 1000, 300)]      # tile 3: no site; tile 5: none
        singles |= {lo + 1023 * TILE + 700, lo + 7 * TILE + 255, lo + 7 * TILE + 256}
    rows = []
    for k, p in enumerate(sorted(singles)):
        kind = "xdi"[k % 3]
        rows.append(row(kind, p, _other_base(content[p])))
    rows += [_run_of_d(a, n) for a, n in runs]
    return rows, singles, runs


@pytest.mark.parametrize("width", [TILE - 1, TILE, TILE + 1, 1025 * TILE])
def test_sites_around_the_tiles(long_text, width):
    di, content = long_text
    lo = 40_000
    assert lo + width + 8 <= len(content)
    rows, singles, runs = _tile_rows(lo, width, content)
    acc = Acc(di, lo, lo + width)
    try:
        acc.add(P._batch(rows, stride=2064, read_stride=16))
        ((want, want_cons), cols) = want_of(acc, content, LOOSE, sparse=True)
        room = lambda count: min(count, 4096)                          # (more than the sites of any range here: the table stays small)
        got, total, cons = acc.sites(opt=LOOSE, cap=room(width))
        assert total == len(want) <= 4096 and got == want and cons == want_cons, width
        # the rows produced what the test is about
        at = np.array([s[0] for s in want]) - lo
        per_tile = np.bincount(at // TILE, minlength=(width + TILE - 1) // TILE)
        assert at[0] == 0 and at[-1] == width - 1 and {p - lo for p in singles} <= set(at.tolist())
        assert {bit for s in want for bit in (1, 2, 4) if s[9] & bit} == {1, 2, 4}
        for a, n in runs:
            assert set(range(a - lo, min(a - lo + n, width))) <= set(at.tolist())
        if width >= TILE:
            assert per_tile.max() == TILE
        else:
            assert set(range(512, 768)) <= set(at.tolist())
        subs = [(5, width - 9), (width - 100, 100), (width - 1, 1), (0, 1), (width // 2, 0), (width, 0), (0, 0)]
        if width > 2 * TILE:
            assert per_tile[3] == 0 and per_tile[2] > 0 and per_tile[4] >= 256 and per_tile[5] == 0 and per_tile[6] == TILE
            assert {TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 1023 * TILE - 1, 1023 * TILE, 1024 * TILE - 1, 1024 * TILE} <= set(at.tolist())
            # ranges that start and end inside tiles, in both rounds of the tile scan
            subs += [(1000, 3000), (6 * TILE + 100, TILE), (1023 * TILE + 5, 2 * TILE - 7 - 5), (1024 * TILE - 1, 2), (1024 * TILE + 77, 1500),
                     (4 * TILE + 600, 3 * TILE)]
        for first, count in subs:
            sub = [s for s in want if lo + first <= s[0] < lo + first + count]
            got, total, cons = acc.sites(first, count, LOOSE, cap=room(count))
            assert total == len(sub) and got == sub and cons == want_cons[first:first + count], (width, first, count)
        assert (acc.raw()[-16:] == P.GUARD).all()
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# cap, and what must stay untouched
# ---------------------------------------------------------------------------------------------------------
def test_cap_and_fill(planted_cases):
    acc, cases, at, content = planted_cases
    (want, want_cons), _ = want_of(acc, content)
    total = len(want)
    in_tile0 = sum(1 for s in want if s[0] - LO < TILE)
    assert 2 < in_tile0 < total - 2
    for cap in (total, total - 1, in_tile0 - 1, in_tile0, in_tile0 + 2, 1, total + 5):      # (the fill from cap on is checked by Acc.sites)
        got, n, cons = acc.sites(cap=cap)
        assert n == total and got == want[:cap] and cons == want_cons, cap
    for cons_on in (True, False):
        got, n, cons = acc.sites(cap=0, null_table=True, cons=cons_on)
        assert n == total and got == [] and cons == (want_cons if cons_on else None)
    # the cons buffer for `first` of every residue mod 16, ends off every boundary
    for first in range(16):
        count = W - first - (3 * first) % 16 - 1
        sub = [s for s in want if LO + first <= s[0] < LO + first + count]
        got, n, cons = acc.sites(first, count)
        assert n == len(sub) and got == sub and cons == want_cons[first:first + count], first
    for first, count in ((at[3] - LO, 1), (at[3] - LO - 1, 3), (TILE - 1, 2), (TILE, 1)):
        got, n, cons = acc.sites(first, count)
        assert cons == want_cons[first:first + count] and got == [s for s in want if LO + first <= s[0] < LO + first + count]


def test_counters_and_scratch(ont):
    di, content = ont
    cases = [c for c in KC.CASES if KC.plantable(c)]
    at = place(cases, content, LO, HI)
    half = len(cases) // 2
    first_rows = [r for c, p in zip(cases[:half], at) for r in stack(c, p)]
    second_rows = [r for c, p in zip(cases[half:], at[half:]) for r in stack(c, p)]
    acc = Acc(di, LO, HI)
    try:
        n_tiles = (W + TILE - 1) // TILE
        created = acc.bytes()
        assert created == 32 * W + 4 + 64 + 8 * n_tiles
        acc.add(P._batch(first_rows, stride=16, read_stride=16))
        raw, cols = acc.raw(), acc.read().copy()
        assert acc.bytes() == created                                  # the read-back needs nothing more
        (want, want_cons), _ = want_of(acc, content)
        got, total, cons = acc.sites()
        assert acc.bytes() == created + 8 * n_tiles                    # the stage's scratch, booked by the first sites call
        assert (got, total, cons) == (want, len(want), want_cons) and total > 5
        assert np.array_equal(acc.raw(), raw) and (raw[-16:] == P.GUARD).all()      # the counters, guard words included
        assert np.array_equal(acc.read().view(np.uint32), cols.view(np.uint32))
        acc.add(P._batch(second_rows, stride=16, read_stride=16))      # a second batch: the sites follow the new records
        (want2, want_cons2), _ = want_of(acc, content)
        got, total, cons = acc.sites()
        assert (got, total, cons) == (want2, len(want2), want_cons2) and len(want2) > len(want) and want2[:len(want)] == want
        assert acc.bytes() == created + 8 * n_tiles                    # ... and not again
        acc.reset()
        got, total, cons = acc.sites()
        assert got == [] and total == 0 and cons == b"N" * W
        got, total, cons = acc.sites(opt=LOOSE)
        assert got == [] and total == 0 and cons == b"N" * W
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# through DeviceMapper: reads from a copy of the text that carries planted variants
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_index(gpu):
    w = KC.planted()
    hi = index.HostIndex.build([w["text"]], names=["planted"], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    yield w, hi, di
    di.close()
    hi.close()


@pytest.mark.parametrize("mode", list(P.MODES))
def test_device_mapper_sites(planted_index, gpu, mode, tmp_path):
    import torch
    w, hi, di = planted_index
    di.set_map_options()
    n, stride = w["reads"].shape
    window = index.text_window(hi, 0)
    lo = window[0]
    dm = mapper.DeviceMapper(di, n, stride - 1, 20, 300, device=gpu, pileup=window, **P.MODES[mode])
    try:
        d_reads = torch.from_numpy(w["reads"]).cuda()
        d_lens = torch.from_numpy(w["lens"].astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        torch.cuda.synchronize()
        before, reads_before = dm.results(n), d_reads.cpu().numpy()
        cols = dm.pileup_columns()
        sites, total, cons = dm.pileup_sites(consensus=True)
        content = hi.content()
        want, want_cons = R.sites(cols, bytes(content[window[0]:window[1]]), lo, R.options())
        assert total == len(sites) == len(want) and R.as_tuples(sites) == want and bytes(cons) == want_cons, mode
        assert sites.dtype == capi.PILEUP_SITE_DT and cons.dtype == np.uint8 and len(cons) == window[1] - window[0]
        missing, away = KC.planted_conditions(w, sites, lo)
        print("%s: %d sites, %d of them more than 10 positions from every planted variant; missing %s" % (mode, total, away, missing))
        if mode == "classic":
            assert not missing, missing
        # every per-read output is the same bytes after the sites call as before it, the accumulator's records too
        after = dm.results(n)
        assert set(after) == set(before)
        for key in before:
            assert np.array_equal(before[key], after[key]), (mode, key)
        assert np.array_equal(d_reads.cpu().numpy(), reads_before)
        assert np.array_equal(dm.pileup_columns().view(np.uint32), cols.view(np.uint32))
        # a first table that is too small: the retry path; no consensus asked: none returned; a sub-range; other options
        again, total2, none = dm.pileup_sites(cap=3)
        assert total2 == total and none is None and np.array_equal(again.view(np.uint8), sites.view(np.uint8))
        assert dm.pileup_sites(cap=0)[1] == total
        sub, n_sub, cons_sub = dm.pileup_sites(50_001, 70_000, consensus=True)
        assert R.as_tuples(sub) == [s for s in want if lo + 50_001 <= s[0] < lo + 120_001] and n_sub == len(sub) and bytes(cons_sub) == want_cons[50_001:120_001]
        strict, n_strict, _ = dm.pileup_sites(min_depth=20, min_count=10, min_pct=60)
        sel = slice(60_000, 100_000)
        want_strict = R.sites(cols[sel], bytes(content[lo + 60_000:lo + 100_000]), lo + 60_000, R.options(20, 10, 60))[0]
        assert [s for s in R.as_tuples(strict) if lo + 60_000 <= s[0] < lo + 100_000] == want_strict and 0 < n_strict < total
        # the text writers: files that parse back to the same sites and bases
        assert textio.write_sites(str(tmp_path / "s.tsv"), hi, sites) == total
        back = [l.split("\t") for l in open(tmp_path / "s.tsv").read().splitlines()]
        kinds_of = lambda t: sum(bit for bit, ch in ((1, "S"), (2, "D"), (4, "I")) if ch in t)
        assert [(int(f[1]) - 1 + lo, int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9]), ord(f[2]), ord(f[3]), ord(f[10]), kinds_of(f[4])) for f in back] == want
        assert {f[0] for f in back} == {"planted"}
        wrote = textio.write_consensus(str(tmp_path / "c.fa"), hi, 0, cons, lo)
        fa = open(tmp_path / "c.fa").read().splitlines()
        assert fa[0] == ">planted" and "".join(fa[1:]) == want_cons.decode().replace("-", "") and wrote == len(want_cons) - want_cons.count(b"-")
    finally:
        dm.close()


def test_refusals(ont):
    import torch
    di, content = ont
    acc = Acc(di, LO, HI)
    try:
        sdi = next(c for c in KC.CASES if c.name == "kinds-SDI")
        where = place([sdi], content, LO + 100, HI)[0]
        acc.add(P._batch(stack(sdi, where), stride=16, read_stride=16))
        created = acc.bytes()
        table = torch.from_numpy(np.full(64 * 32, FILL8, dtype=np.uint8)).cuda()
        n_sites = torch.from_numpy(np.full(2, -1, dtype=np.int64)).cuda()
        cons = torch.from_numpy(np.full(W, FILL8, dtype=np.uint8)).cuda()

        def refused(message, opt=(0, 0, 0, 0), first=0, count=W, sites=table.data_ptr(), cap=64, total=n_sites.data_ptr()):
            o = capi.PileupCallOptions(*opt)
            assert lib.lrm_pileup_sites_dev(acc.h, C.byref(o), first, count, sites, cap, total, cons.data_ptr(), P._stream()) < 0, message
            assert message in lib.lrm_last_error(), (message, lib.lrm_last_error())

        refused(b"outside a window", first=1)
        refused(b"outside a window", first=W + 1, count=0)
        refused(b"min_pct", opt=(0, 0, 101, 0))
        refused(b"reserved", opt=(0, 0, 0, 1))
        refused(b"16-byte aligned", sites=table.data_ptr() + 8)
        refused(b"null argument", total=None)
        refused(b"null argument", sites=None)
        refused(b"8-byte aligned", total=n_sites.data_ptr() + 4)
        assert lib.lrm_pileup_sites_dev(None, None, 0, 0, None, 0, n_sites.data_ptr(), None, P._stream()) < 0
        torch.cuda.synchronize()
        # no kernel ran: nothing was written, and the stage's scratch was never allocated
        assert (table.cpu().numpy() == FILL8).all() and (n_sites.cpu().numpy() == -1).all() and (cons.cpu().numpy() == FILL8).all()
        assert acc.bytes() == created
        got, total, _ = acc.sites()
        assert total == 1 and got[0][0] == where and got[0][9] == 7
    finally:
        acc.close()
