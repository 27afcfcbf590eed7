"""Split reads (docs/GACT_SPEC.md, "Split reads") without a GPU: the segment table (lrm_split_plan), the clip counts of an
alignment (lrm_clip_of_cigar) and the SAM text with supplementary records (lrm_sam_format_split), against tests/split_ref.py."""
import ctypes as C

import numpy as np
import pytest

import sam_ref
import split_ref
from longreadmapper_amd import capi, mapper, textio
from longreadmapper_amd.capi import lib


def _clip(cl, cr):
    c = np.zeros(len(cl), dtype=mapper.CLIP_DT)
    c["left"], c["right"] = cl, cr
    return c


def _rows(seg):
    return [tuple(int(x) for x in s) for s in seg]


@pytest.mark.parametrize("M", [0, 50, 200, 777])
def test_plan_equals_reference_on_random_batches(M):
    rng = np.random.default_rng(7 + M)
    n = 3000
    lens = rng.integers(0, 5000, n).astype(np.uint32)
    cl = (rng.integers(0, 1200, n) * (rng.random(n) < 0.5)).astype(np.uint32)
    cr = (rng.integers(0, 1200, n) * (rng.random(n) < 0.5)).astype(np.uint32)
    cl, cr = np.minimum(cl, lens), np.minimum(cr, lens - np.minimum(cl, lens))
    want = split_ref.plan(lens, cl, cr, M)
    assert len(want) > 200
    assert _rows(mapper.split_plan(lens, _clip(cl, cr), M)) == want


def test_plan_edges():
    M = 200
    lens = np.array([1000, 1000, 1000, 1000, 400, 0, 1000], dtype=np.uint32)
    cl = np.array([M - 1, M, 0, 300, 200, 0, 0], dtype=np.uint32)
    cr = np.array([0, 0, M, 450, 200, 0, M - 1], dtype=np.uint32)
    got = _rows(mapper.split_plan(lens, _clip(cl, cr)))
    assert got == split_ref.plan(lens, cl, cr) == [(1, 0, 200, 0), (2, 800, 200, 1), (3, 0, 300, 0), (3, 550, 450, 1),
                                                    (4, 0, 200, 0), (4, 200, 200, 1)]
    # cap one too small: -3, the count, nothing written
    rc, k, seg = mapper.split_plan(lens, _clip(cl, cr), cap=5)
    assert (rc, k) == (-3, 6) and not seg["len"].any() and b"6 segments" in lib.lrm_last_error()
    rc, k, seg = mapper.split_plan(lens, _clip(cl, cr), cap=6)
    assert (rc, k) == (0, 6) and _rows(seg) == got
    # no segment, no read
    assert len(mapper.split_plan(lens, _clip(np.zeros(7), np.zeros(7)))) == 0
    assert mapper.split_plan(np.zeros(0, np.uint32), _clip([], []), cap=0)[:2] == (0, 0)
    for bad in (1, 49, (1 << 20) + 1):
        with pytest.raises(capi.LrmError, match="split_min_len"):
            mapper.split_plan(lens, _clip(cl, cr), bad)
        with pytest.raises(ValueError):
            split_ref.plan(lens, cl, cr, bad)
    assert _rows(mapper.split_plan(lens, _clip(cl, cr), 1 << 20)) == []


def test_plan_clamps_clip_counts_and_lets_sides_overlap():
    """cl > n, cr > n (each becomes n, and qualifies or not as n does), cl + cr > n with both sides qualifying"""
    M = 200
    lens = np.array([300, 300, 300, 250, 150, 199, 200], dtype=np.uint32)
    cl = np.array([301, 0, 250, 5000, 400, 0xFFFFFFFF, 200], dtype=np.uint32)
    cr = np.array([0, 1000, 200, 6000, 400, 0, 0xFFFFFFFF], dtype=np.uint32)
    got = _rows(mapper.split_plan(lens, _clip(cl, cr), M))
    assert got == split_ref.plan(lens, cl, cr, M) == [(0, 0, 300, 0), (1, 0, 300, 1), (2, 0, 250, 0), (2, 100, 200, 1),
                                                       (3, 0, 250, 0), (3, 0, 250, 1), (6, 0, 200, 0), (6, 0, 200, 1)]


@pytest.mark.parametrize("ops", [b"==X=I=D=", b"SSS==X=", b"==X=SS", b"S==DD=I=SSSS", b"=", b"", b"S" * 300 + b"=" * 20 + b"S" * 1234])
def test_clip_of_cigar_bytes_and_text(ops):
    want = split_ref.clip_of_ops(ops)
    assert mapper.clip_of_cigar(ops) == want
    text = sam_ref.rle(ops).encode()
    assert mapper.clip_of_cigar(text, is_text=True) == want
    if not ops:
        assert text == b"*"


def _batch(tmp_path, recs):
    p = tmp_path / "r.fq"
    p.write_bytes(b"".join((b"@%s\n%s\n+\n%s\n" % (nm, s, q)) if q is not None else (b">%s\n%s\n" % (nm, s)) for nm, s, q in recs))
    rd = textio.Reader(p)
    assert rd.next(100) == len(recs)
    return rd, rd.batch


def _cigars(ops_list, scores, as_text):
    return textio.cigar_array(ops_list, scores, [sam_ref.rle(o).encode() for o in ops_list] if as_text else None)


COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.mark.parametrize("as_text", [False, True])
@pytest.mark.parametrize("fasta", [False, True])
def test_sam_lines_equal_the_reference_formatter(tmp_path, as_text, fasta):
    rng = np.random.default_rng(5)
    pymta = [("chrA", 0, 100000), ("contig_two", 200000, 50000)]
    mta = textio.mta_table(pymta)

    def rnd(k):
        return bytes(b"ACGT"[x] for x in rng.integers(0, 4, k))

    # reads 0..3: one left or right segment for each (ps, ss); 4: two segments; 5: a segment that is not reported;
    # 6: no segment; 7: unmapped; net D, net I and neither among the alignments
    n_reads = 8
    lens = [900, 900, 1000, 1000, 1500, 800, 300, 250]
    seqs = [rnd(k) for k in lens]
    quals = [None if fasta else bytes(33 + (i + j) % 60 for j in range(k)) for i, k in enumerate(lens)]
    prim_ops = [b"=" * 600 + b"S" * 300, b"S" * 250 + b"=" * 300 + b"D" * 5 + b"=" * 350, b"=" * 400 + b"I" * 7 + b"X" + b"=" * 292 + b"S" * 300,
                b"S" * 400 + b"=" * 600, b"S" * 500 + b"=" * 600 + b"S" * 400, b"=" * 550 + b"S" * 250, b"=" * 300, b""]
    ps = [0, 0, 1, 1, 1, 0, 1, 0]
    prim = [dict(ops=prim_ops[i], score=i if i < 7 else -1, meta_r=1, seq_id=i % 2, off=1000 * i + 17, strand=ps[i]) for i in range(n_reads)]
    cl, cr = zip(*(split_ref.clip_of_ops(o) for o in prim_ops))
    table = split_ref.plan(lens, cl, cr)
    assert [t[0] for t in table] == [0, 1, 2, 3, 4, 4, 5]
    seg_ss = [0, 1, 0, 1, 1, 0, 0]
    seg_ops = [b"S" * 10 + b"=" * 290, b"=" * 100 + b"D" * 3 + b"=" * 150, b"=" * 200 + b"I" * 4 + b"=" * 90 + b"S" * 6, b"=" * 400,
               b"S" * 20 + b"=" * 480, b"=" * 380 + b"X" * 2 + b"S" * 18, b"=" * 250]
    k = len(table)
    row_stride = 512
    rows = np.zeros((k, row_stride), dtype=np.uint8)
    seg = np.zeros(k, dtype=mapper.SEGMENT_DT)
    smeta = np.zeros(k, dtype=mapper.META_DT)
    sscore = np.arange(40, 40 + k, dtype=np.int32)
    smeta_r = np.ones(k, dtype=np.int32)
    segs_of = {i: [] for i in range(n_reads)}
    for s, (read, start, ln, fl) in enumerate(table):
        R = seqs[read] if ps[read] == 0 else seqs[read].translate(COMP)[::-1]       # the read as the extension left it
        row = R[start:start + ln]
        if seg_ss[s]:
            row = row.translate(COMP)[::-1]
        rows[s, :ln] = np.frombuffer(row, dtype=np.uint8)
        flags = fl | (0 if read == 5 else split_ref.SEG_ALIGNED)
        seg[s] = (read, start, ln, flags)
        smeta[s]["seq_id"], smeta[s]["off"], smeta[s]["strand"] = (s + 1) % 2, 5000 + 31 * s, seg_ss[s]
        segs_of[read].append(dict(start=start, len=ln, flags=flags, row=row.decode(), ops=seg_ops[s], score=int(sscore[s]),
                                  seq_id=(s + 1) % 2, off=5000 + 31 * s, strand=seg_ss[s]))
        assert len(seg_ops[s]) - seg_ops[s].count(b"D") == ln
    # the batch as the device pass leaves it when keep_reads is off: reverse-strand reads reverse-complemented in place
    printed = [seqs[i] if ps[i] == 0 or i == 7 else seqs[i].translate(COMP)[::-1] for i in range(n_reads)]
    rd, b = _batch(tmp_path, [(b"q%d" % i, printed[i], quals[i]) for i in range(n_reads)])
    score = np.array([p["score"] for p in prim], dtype=np.int32)
    meta_r = np.array([p["meta_r"] for p in prim], dtype=np.int32)
    meta = np.zeros(n_reads, dtype=mapper.META_DT)
    meta["seq_id"], meta["off"], meta["strand"] = [p["seq_id"] for p in prim], [p["off"] for p in prim], ps
    cig, keep1 = _cigars(prim_ops, score, as_text)
    scig, keep2 = _cigars(seg_ops, sscore, as_text)
    out = capi.SplitOut(k, k, seg.ctypes.data, rows.ctypes.data, row_stride, None, None, scig.ctypes.data, None, 0,
                        sscore.ctypes.data, smeta.ctypes.data, smeta_r.ctypes.data, None, None)

    def fmt(split):
        return textio.sam_format(b, mta, cig, score, meta, meta_r, n_reads, is_text=as_text, split=split, entry="lrm_sam_format_split")

    got = fmt(out)
    want = "".join(split_ref.records("q%d" % i, printed[i].decode(), quals[i].decode() if quals[i] else None, pymta, prim[i], segs_of[i])
                   for i in range(n_reads))
    assert got == want
    lines = got.splitlines()
    assert len(lines) == n_reads + 6                                              # the unreported segment prints nothing
    f = [ln.split("\t") for ln in lines]
    assert [int(x[1]) for x in f] == [0, 2048, 0, 2048 + 16, 16, 2048 + 16, 16, 2048, 16, 2048, 2048 + 16, 0, 16, 4]
    # H lengths: read 0's right segment on its own forward strand, read 1's left segment on its own reverse strand
    assert f[1][5] == "600H10S290M" and f[3][5] == "650H100M3D150M" and f[1][9] == segs_of[0][0]["row"]
    # SA:Z: the primary names its segments left then right, a segment the primary and then the other segment
    assert f[0][-1] == "SA:Z:contig_two,5001,+,610S290M,255,40;" and f[1][-1] == "SA:Z:chrA,18,+,600M300S,255,0;"
    assert f[2][-1] == "SA:Z:chrA,5032,-,650S250M3D,255,41;" and f[3][-1] == "SA:Z:contig_two,1018,+,250S650M5D,255,1;"
    assert f[4][-1] == "SA:Z:contig_two,5063,-,700S294M4I6S,255,42;" and f[5][-1] == "SA:Z:chrA,2018,-,700M7I300S,255,2;"
    assert f[8][-1].count(";") == 2 and f[9][-1].count(";") == 2 and f[9][-1].split(";")[1] == f[8][-1][5:].split(";")[1]
    assert all(len(x[9]) == len(x[10]) or x[10] == "*" for x in f)
    if not fasta:
        assert f[1][10] == quals[0][600:].decode() and f[3][10] == quals[1][:250][::-1].decode()
        assert f[5][10] == quals[2][:300][::-1].decode() and f[7][10] == quals[3][600:].decode()
    # without segments: exactly lrm_sam_format (which takes op bytes)
    if not as_text:
        plain = textio.sam_format(b, mta, cig, score, meta, meta_r, n_reads, entry="lrm_sam_format")
        none = capi.SplitOut()
        assert fmt(None) == plain and fmt(none) == plain
        assert [ln for ln in lines if "SA:Z" not in ln] == [ln for ln in plain.splitlines() if ln.split("\t")[0] in ("q5", "q6", "q7")]
    rd.close()


def test_fields_mirrors_and_entry_points():
    assert capi.MapOptions.split.offset == 68 and capi.MapOptions.split_min_len.offset == 72 and C.sizeof(capi.MapOptions) == 76
    o = capi.map_options(split=1, split_min_len=300)
    assert (o.split, o.split_min_len) == (1, 300) and o.struct_size == 76
    assert (capi.map_options().split, capi.map_options().split_min_len) == (0, 0)
    assert C.sizeof(capi.Segment) == 16 == mapper.SEGMENT_DT.itemsize
    assert (capi.SEG_RIGHT, capi.SEG_ALIGNED, capi.SPLIT_MIN_DEFAULT) == (split_ref.SEG_RIGHT, split_ref.SEG_ALIGNED, split_ref.MIN_DEFAULT)
    for name in ("lrm_split_plan", "lrm_clip_of_cigar", "lrm_split_batch_dev", "lrm_split_batch", "lrm_sam_format_split"):
        assert getattr(lib, name) is not None
    assert lib.lrm_abi_version() == 3 and mapper.N_KERNELS == 9
