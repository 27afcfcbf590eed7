"""The variant stage of the pileup on the GPU (docs/GACT_SPEC.md, "Pileup variants and VCF"): pileup_var_count_kernel, the two
scans and pileup_var_write_kernel.  The accumulator is filled through lrm_pileup_add_dev with hand-made rows; the expected
table is lrm_pileup_variants_host -- which tests/test_pileup_var_cpu.py pins against the Python reference -- over
lrm_pileup_read_dev and lrm_pileup_ins_read_dev of the same accumulator.  Tables and totals are compared for equality; the
table lies in 0xA5 fill with 48 guard bytes either side that must stay fill."""
import ctypes as C

import numpy as np
import pytest

import pileup_call_cases as KC
import pileup_cases as PC
import pileup_host_cases as HC
import pileup_var_ref as V
import test_gpu_pileup as P
import test_gpu_pileup_ins as I
import test_pileup_var_cpu as H
from test_gpu_pileup_sites import _run_of_d, _tile_rows, place, row, stack
from longreadmapper_amd import capi, index, mapper, textio
from longreadmapper_amd.capi import lib
from longreadmapper_amd.pileup import Pileup

pytestmark = pytest.mark.gpu
SMALL = dict(lc_long_max=13)
TILE = capi.PILEUP_TILE
LO = PC.LO
FILL8 = 0xA5
LOOSE = (1, 1, 1, 0, 0)           # options under which one 'X', 'D' or opening 'I' column makes a record
DEF = (0, 0, 0, 0, 0)
SNV, DEL, INS = V.SNV, V.DEL, V.INS


class Acc(I.Acc):
    """I.Acc with the variant stage: the table lies in 0xA5 fill with one record of fill (48 guard bytes) either side, the
    count word between two words of fill; everything that must stay untouched is checked."""

    def variants(self, first=0, count=None, opt=None, cap=None, null_table=False):
        import torch
        count = self.W - first if count is None else count
        cap = 3 * count if cap is None else cap
        table = torch.from_numpy(np.full((cap + 2) * 48, FILL8, dtype=np.uint8)).cuda()
        total = torch.from_numpy(np.full(3, -1, dtype=np.int64)).cuda()
        o = H.variant_options(opt) if opt is not None else None
        capi.check(lib.lrm_pileup_variants_dev(self.h, C.byref(o) if o is not None else None, first, count, None if null_table else table.data_ptr() + 48,
                                               cap, total.data_ptr() + 8, P._stream()), "lrm_pileup_variants_dev")
        torch.cuda.synchronize()
        t, tb = total.cpu().numpy(), table.cpu().numpy()
        assert t[0] == -1 and t[2] == -1, (first, count)
        n = int(t[1])
        k = min(n, cap)
        assert (tb[:48] == FILL8).all() and (tb[48 * (1 + k):] == FILL8).all(), (first, count, cap, n)         # from cap on, and the guard bytes
        return V.as_tuples(tb[48:48 * (1 + k)].view(capi.PILEUP_VARIANT_DT)), n                             # (as_tuples: the padding is zero)

    def want(self, content, first=0, count=None, opt=None):
        """lrm_pileup_variants_host over the read-back of the same positions"""
        count = self.W - first if count is None else count
        cols = self.read(first, count)
        words = self.ins_words(first, count) if self.K and count else None
        got, total, _ = H.host_variants(cols, words, content[self.lo + first:self.lo + first + count], self.lo + first, opt)
        assert total == len(got)
        return V.as_tuples(got)

    def check(self, content, first=0, count=None, opt=LOOSE, cap=None):
        want = self.want(content, first, count, opt)
        got, total = self.variants(first, count, opt, cap)
        assert total == len(want) and got == (want if cap is None else want[:cap]), (first, count, cap, total, len(want))
        return want


@pytest.fixture(scope="module")
def ont(gpu):
    import workloads
    sc = workloads.scenario("ont-2k")
    di = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL)
    yield di, bytes(sc["hi"].content())
    di.close()


def other_base(content, p):
    """a read byte that differs from the text byte of position p"""
    return b"C" if content[p:p + 1] == b"A" else b"A"


def runs_of(want, lo):
    return [(r[0] - lo, r[1]) for r in want if r[6] == DEL]


# ---------------------------------------------------------------------------------------------------------
# window widths
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_window_widths(ont, width):
    di, content = ont
    lo = LO
    rows, singles, runs = _tile_rows(lo, min(width, 2 * TILE), content)       # (at most two tiles of rows: the long form is for longer texts)
    if width > 2 * TILE:
        rows.append(row("d", lo + width - 1))
    acc = Acc(di, lo, lo + width, 0)
    try:
        acc.add(P._batch(rows, stride=2064, read_stride=16))
        want = acc.check(content)
        # the rows produced what the test is about: a record on the window's first and last position, every kind, and at a
        # width of a tile or more the run that is the whole of tile 0
        at = [r[0] - lo for r in want]
        assert at[0] == 0 and at[-1] == width - 1
        if width >= TILE:
            assert (0, TILE) in runs_of(want, lo) and {r[6] for r in want} == {SNV, DEL, INS}
        elif width > 1:
            assert (512, 256) in runs_of(want, lo)
        for first, count in ((0, 1), (width - 1, 1), (width // 2, 0), (width, 0), (5, max(width - 9, 0)), (width // 3, width // 2)):
            if first <= width and first + count <= width:
                acc.check(content, first, count)
        assert (acc.raw()[-16:] == P.GUARD).all()
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# runs across tiles and scan rounds, and ranges that cut them
# ---------------------------------------------------------------------------------------------------------
W3 = 3 * TILE + 12
SCENES = {
    # a run across a tile edge, one across a scan round, one from position 0, one ending on the window's last position, two
    # runs that meet a tile edge from either side with one clean position between them (the tile's last, then its first)
    "edges": [(TILE - 2, 4), (255, 3), (0, 3), (W3 - 5, 5), (2 * TILE - 4, 3), (2 * TILE, 3), (3 * TILE - 3, 3), (3 * TILE + 1, 2)],
    # a whole tile inside the run: the run's length comes through a wholly deleted tile
    "whole-tile": [(TILE - 1, TILE + 2), (2 * TILE + 2, 3), (0, 5)],
    # two whole tiles inside one run that ends on the window's last position; the range cuts decide its length
    "two-tiles": [(TILE - 3, 2 * TILE + 15)],
}


@pytest.mark.parametrize("scene,ins_cols", [("edges", 0), ("edges", 8), ("whole-tile", 0), ("whole-tile", 4), ("two-tiles", 0)])
def test_runs_and_range_cuts(ont, scene, ins_cols):
    di, content = ont
    lo = LO
    runs = SCENES[scene]
    rows = [_run_of_d(lo + a, n) for a, n in runs]
    # an SNV and an insertion inside the cross-tile run, on either side of the edge, and away from every run
    extra = [TILE - 1, TILE, 700]
    for p in extra:
        rows += [row("x", lo + p, other_base(content, lo + p)), I._ins_row(lo + p, b"GATTACAGATT")]
    acc = Acc(di, lo, lo + W3, ins_cols)
    try:
        acc.add(P._batch(rows, stride=2 * TILE + 64, read_stride=32))
        want = acc.check(content)
        got_runs = runs_of(want, lo)
        assert got_runs == sorted((a, min(n, W3 - a)) for a, n in runs), scene
        by = {(r[0] - lo, r[6]): r for r in want}
        for p in extra:                                                # DEL (where a run starts), SNV, INS, in this order
            assert by[(p, SNV)][8] == other_base(content, lo + p)[0] and by[(p, INS)][10] == b"GATTACAGATT"[:ins_cols]
            assert by[(p, INS)][11] & capi.INS_FULL if ins_cols else by[(p, INS)][11] == 0
        kinds_at = [r[6] for r in want if r[0] - lo == TILE - 1]
        assert kinds_at == ([DEL, SNV, INS] if scene == "whole-tile" else [SNV, INS])
        total = len(want)
        subs = [
            (TILE - 1, 2), (TILE - 1, 1), (TILE, 5),                   # first and first + count inside the cross-tile run
            (TILE - 1, W3 - TILE + 1), (TILE - 3, 7),                  # first at a run's second position / not a multiple of 16
            (3, 2 * TILE), (250, 10), (257, 600), (TILE + 5, TILE - 10), (TILE + 1, 2 * TILE), (2 * TILE - 1, 2), (W3 - 3, 3), (W3 - 1, 1), (0, 2),
            (2 * TILE - 2, TILE + 2), (TILE, TILE), (TILE, 2 * TILE), (1, W3 - 1),
        ]
        for first, count in subs:
            sub = acc.check(content, first, count)
            # ... which is the rule on the range alone: runs cut at both of its ends and nowhere else
            cut = sorted((max(a, first), min(a + n, first + count, W3) - max(a, first)) for a, n in runs if max(a, first) < min(a + n, first + count, W3))
            assert runs_of(sub, lo) == cut, (scene, first, count)
        # cap: none with a NULL table, one short of the total, inside the first tile's records, above the total
        in_tile0 = sum(1 for r in want if r[0] - lo < TILE)
        for cap in sorted({0, 1, in_tile0 - 1, in_tile0, in_tile0 + 1, total - 1, total, total + 7}):
            acc.check(content, cap=cap)
        got, n = acc.variants(opt=LOOSE, cap=0, null_table=True)
        assert (got, n) == ([], total)
        # the default options see none of these single reads
        assert acc.variants(opt=None) == ([], 0) and acc.want(content) == []
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# one position with all three kinds; cap between its records
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ins_cols", [0, 1, 8])
def test_one_position_with_three_kinds(ont, ins_cols):
    di, content = ont
    sdi = next(c for c in KC.CASES if c.name == "kinds-SDI")
    lo, hi = LO, LO + TILE + 300
    where = place([sdi], content, lo + TILE, hi)[0]                    # in the window's second tile
    acc = Acc(di, lo, hi, ins_cols)
    try:
        acc.add(P._batch(stack(sdi, where), stride=16, read_stride=16))
        want = acc.check(content, opt=DEF)
        assert [(r[0], r[6], r[1]) for r in want] == [(where, DEL, 1), (where, SNV, 1), (where, INS, min(ins_cols, 1))]
        assert want[2][10] == b"A"[:ins_cols] and want[2][5] == (want[2][4] if ins_cols else 0)      # the rows insert one A each
        assert acc.variants(opt=None)[0] == want                       # opt == NULL: the defaults
        for cap in (0, 1, 2, 3, 4):                                    # between the records of one position
            acc.check(content, opt=DEF, cap=cap)
        assert acc.variants(opt=DEF, cap=0, null_table=True) == ([], 3)
        for first, count in ((where - lo, 1), (where - lo - 1, 2), (where - lo + 1, 5), (0, where - lo)):
            acc.check(content, first, count, DEF)
        # the genotype follows hom_pct
        gts = {hom: [r[9] for r in acc.check(content, opt=(0, 0, 0, 0, hom))] for hom in (1, 100)}
        assert gts[1] == [2, 2, 2] and gts[100] == [1, 1, 1]
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# what must stay untouched
# ---------------------------------------------------------------------------------------------------------
def test_state_is_not_modified(ont):
    di, content = ont
    lo, W = LO, 2 * TILE + 100
    n_tiles = 3
    rows = [_run_of_d(lo + TILE - 2, 4), row("x", lo + 9, other_base(content, lo + 9)), I._ins_row(lo + TILE + 5, b"ACGT"), row("d", lo + W - 1)]
    acc = Acc(di, lo, lo + W, 4)
    try:
        acc.add(P._batch(rows, stride=32, read_stride=32))
        created = acc.bytes()
        sites, polish = acc.sites(opt=LOOSE[:4]), acc.polish(opt=LOOSE[:4])
        assert acc.bytes() == created + 8 * n_tiles                    # the call stage's scratch
        raw, ins_raw = acc.raw(), acc.ins_raw()
        want = acc.check(content)
        assert len(want) == 4 and acc.bytes() == created + 16 * n_tiles       # 8 more bytes per tile, booked by the first call
        acc.check(content, 5, TILE)
        acc.check(content, cap=1)
        assert acc.bytes() == created + 16 * n_tiles                   # ... and not again
        assert np.array_equal(acc.raw(), raw) and np.array_equal(acc.ins_raw(), ins_raw)           # both allocations, guard words included
        assert (raw[-16:] == P.GUARD).all() and (ins_raw[-16:] == P.GUARD).all()
        assert acc.sites(opt=LOOSE[:4]) == sites and acc.polish(opt=LOOSE[:4]) == polish
        acc.reset()
        assert acc.variants(opt=LOOSE) == ([], 0)
    finally:
        acc.close()


def test_refusals(ont, gpu):
    import torch
    di, content = ont
    W = 500
    acc = Acc(di, LO, LO + W, 0)
    try:
        acc.add(P._batch([row("d", LO + 7)], stride=16, read_stride=16))
        created = acc.bytes()
        table = torch.from_numpy(np.full(64 * 48, FILL8, dtype=np.uint8)).cuda()
        n_vars = torch.from_numpy(np.full(2, -1, dtype=np.int64)).cuda()

        def refused(message, opt=DEF, first=0, count=W, table_at=table.data_ptr(), cap=64, total=n_vars.data_ptr(), handle=acc.h):
            o = H.variant_options(opt)
            assert lib.lrm_pileup_variants_dev(handle, C.byref(o), first, count, table_at, cap, total, P._stream()) < 0, message
            assert message in lib.lrm_last_error(), (message, lib.lrm_last_error())

        refused(b"outside a window", first=1)
        refused(b"outside a window", first=W + 1, count=0)
        refused(b"ranks are 32-bit", count=(2**32 + 2) // 3)           # 3 * count >= 2^32
        refused(b"min_pct", opt=(0, 0, 101, 0, 0))
        refused(b"reserved", opt=(0, 0, 0, 1, 0))
        refused(b"hom_pct", opt=(0, 0, 0, 0, 101))
        refused(b"reserved", opt=(0, 0, 0, 0, 0, (0, 1, 0)))
        refused(b"16-byte aligned", table_at=table.data_ptr() + 8)
        refused(b"8-byte aligned", total=n_vars.data_ptr() + 4)
        refused(b"null argument", total=None)
        refused(b"null argument", table_at=None)
        refused(b"null argument", handle=None)
        torch.cuda.synchronize()
        assert (table.cpu().numpy() == FILL8).all() and (n_vars.cpu().numpy() == -1).all()
        assert acc.bytes() == created                                  # no kernel ran, no scratch was allocated
        assert acc.variants(opt=LOOSE)[1] == 1
        assert 3 * ((2**32 + 2) // 3) >= 2**32 > 3 * ((2**32 + 2) // 3 - 1)
    finally:
        acc.close()
    # a group handle holds one text per replica: no accumulator is created on it, so no variants call runs on one; the
    # accumulator of its replica 0 answers like any other
    import workloads
    dg = index.DeviceIndex.upload_multi(workloads.scenario("ont-2k")["hi"], [gpu, gpu], **SMALL)
    try:
        h = C.c_void_p()
        assert lib.lrm_pileup_create_ins(C.byref(h), dg.handle, LO, LO + W, 0) < 0 and b"group handle" in lib.lrm_last_error() and not h
        rep0 = Pileup(dg, LO, LO + W, 0, replica=0, device=gpu)
        assert rep0.variants(min_depth=1, min_count=1, min_pct=1)[1] == 0
        rep0.close()
    finally:
        dg.close()


# ---------------------------------------------------------------------------------------------------------
# the planted workload: DeviceMapper, the host-buffer path, the flow
# ---------------------------------------------------------------------------------------------------------
def _device_variants(di, gpu, w, window, content, **kw):
    """DeviceMapper over the planted reads -> (variants, total, columns, insertion words, the table asked for with cap=3)"""
    import torch
    n, stride = w["reads"].shape
    dm = mapper.DeviceMapper(di, n, stride - 1, 20, 300, device=gpu, pileup=window, pileup_ins_cols=8, **kw)
    try:
        d_reads = torch.from_numpy(w["reads"].copy()).cuda()
        d_lens = torch.from_numpy(w["lens"].astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        torch.cuda.synchronize()
        cols, words = dm.pileup_columns(), dm.pileup_ins_columns()
        variants, total = dm.pileup_variants()
        again, total2 = dm.pileup_variants(cap=3)                      # a first table that is too small: the retry path
        assert total2 == total and again.tobytes() == variants.tobytes()
        assert dm.pileup_variants(cap=0)[1] == total
        sub, n_sub = dm.pileup_variants(50_001, 70_000, hom_pct=50)
        lo = window[0]
        want_sub, _, _ = H.host_variants(cols[50_001:120_001], words[50_001:120_001], content[50_001:120_001], lo + 50_001, (0, 0, 0, 0, 50))
        assert n_sub == len(sub) and sub.tobytes() == want_sub.tobytes() and n_sub > 10
        return variants, total, cols, words
    finally:
        dm.close()


@pytest.fixture(scope="module")
def planted(gpu):
    w = KC.planted()
    hi = index.HostIndex.build([w["text"]], names=["planted"], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    window = index.text_window(hi, 0)
    content = bytes(hi.content()[window[0]:window[1]])
    variants, total, cols, words = _device_variants(di, gpu, w, window, content)
    yield dict(w=w, hi=hi, di=di, window=window, variants=variants, total=total, cols=cols, words=words, content=content)
    di.close()
    hi.close()


def test_device_mapper_classic(planted):
    s = planted
    lo = s["window"][0]
    want, total, _ = H.host_variants(s["cols"], s["words"], s["content"], lo, cap=4096)
    assert s["variants"].dtype == capi.PILEUP_VARIANT_DT and s["total"] == total == len(s["variants"])
    assert s["variants"].tobytes() == want.tobytes()
    c = H.planted_conditions(s["w"], V.as_tuples(s["variants"]), lo)
    print("classic:", {k: v for k, v in c.items() if k != "missing_snv"})
    assert c["kinds"] == H.PLANTED_KINDS and not c["missing_snv"] and not c["far_not_1"] and c["del_sums_ok"] >= 9 and c["hom_snv"] == H.PLANTED_HOM_SNV
    pos1 = [int(line.split("\t")[1]) for line in textio.vcf_text(s["hi"], s["variants"]).decode().splitlines()]
    assert len(pos1) == total and all(a <= b for a, b in zip(pos1, pos1[1:]))


def test_device_mapper_anchored_clip(planted, gpu):
    s = planted
    variants, total, cols, words = _device_variants(s["di"], gpu, s["w"], s["window"], s["content"], **P.MODES["clip"])
    want, n, _ = H.host_variants(cols, words, s["content"], s["window"][0], cap=8192)
    assert total == n == len(variants) > 50 and variants.tobytes() == want.tobytes()


def test_host_buffer_path(planted, gpu):
    s = planted
    acc = Pileup(s["di"], *s["window"], 8, device=gpu)
    try:
        for reads, lens in HC.batches(s["w"]):
            mapper.map_batch(s["di"], reads, lens, 20, 300, options=HC.PIPE, pileup=acc)
        created = acc.bytes()
        variants, total = acc.variants()
        assert total == s["total"] and variants.tobytes() == s["variants"].tobytes()
        n_tiles = (s["window"][1] - s["window"][0] + TILE - 1) // TILE
        assert acc.bytes() == created + 16 * n_tiles                   # the call stage's scratch and the variant stage's, both new here
        again, total2 = acc.variants(cap=1)
        assert total2 == total and again.tobytes() == variants.tobytes() and acc.bytes() == created + 16 * n_tiles
        sub, n_sub = acc.variants(100_000, 50_000)
        lo = s["window"][0]
        assert V.as_tuples(sub) == [r for r in V.as_tuples(variants) if lo + 100_000 <= r[0] < lo + 150_000] and n_sub == len(sub)
    finally:
        acc.close()


def test_accaln_flow_writes_the_vcf(planted, gpu, tmp_path):
    s = planted
    w = s["w"]
    fa, fq = tmp_path / "planted.fa", tmp_path / "reads.fq"
    HC.write_fasta(fa, [(b"planted", w["text"])])
    assert lib.lrm_accidx(str(fa).encode(), 32, 10, 1) == 0
    HC.write_fastq(fq, w["reads"], w["lens"])
    n = len(w["lens"])
    counts = textio.accaln(str(fa), str(fq), None, 600, device=gpu, rg_id=7, mapq=1,
                           pileup=dict(seq=0, ins_cols=8, vcf=str(tmp_path / "variants.vcf"), sites=str(tmp_path / "sites.tsv"), sample="reads"))
    assert counts[0] == n and counts[1] > n * 9 // 10
    hi = index.HostIndex.read(str(fa))
    try:
        assert index.text_window(hi, 0) == s["window"]
        want = textio.vcf_header(hi, "reads") + textio.vcf_text(hi, s["variants"])
    finally:
        hi.close()
    got = open(tmp_path / "variants.vcf", "rb").read()
    assert got == want and len(got.splitlines()) == 10 - 2 + s["total"]            # one contig line here, three in the header test
    assert len(open(tmp_path / "sites.tsv", "rb").read().splitlines()) == 120
    # the sites table is what it was without the VCF file, and hom_pct reaches the records
    textio.accaln(str(fa), str(fq), None, 600, device=gpu, rg_id=7, mapq=1,
                  pileup=dict(seq=0, ins_cols=8, vcf=str(tmp_path / "v100.vcf"), hom_pct=100))
    lines = open(tmp_path / "v100.vcf").read().splitlines()
    assert lines[-1].split("\t")[-1].startswith(("0/1:", "1/1:")) and lines[7].endswith("\tSAMPLE")
    hom = lambda ls: sum(l.split("\t")[-1].startswith("1/1") for l in ls[8:])       # noqa: E731
    assert hom(lines) < hom(got.decode().splitlines()) and len(lines) == 8 + s["total"]
