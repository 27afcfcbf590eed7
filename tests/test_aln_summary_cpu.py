"""Alignment summary records and PAF text without a GPU (docs/GACT_SPEC.md, "Alignment summary and PAF"):

  (a) lrm_aln_summary_host, the rule's statement in the library, against tests/aln_summary_ref.py;
  (b) what the records mean on real alignments: NM is the score, the clips are the end clipping's;
  (c) lrm_paf_format against the reference line; the struct sizes and the exported entry points."""
import ctypes as C
import itertools

import numpy as np
import pytest

import aln_summary_ref as ref
import anchored_cases
import clip_ref
import gact_cases
import orc
from longreadmapper_amd import capi, mapper, textio
from longreadmapper_amd.capi import lib


# ---------------------------------------------------------------------------------------------------------
# (a) the rule
# ---------------------------------------------------------------------------------------------------------
def test_every_short_row():
    checked = 0
    for m in range(7):
        for t in itertools.product(b"=XIDS", repeat=m):
            ops = bytes(t)
            assert mapper.aln_summary_host(ops) == ref.summary(ops), ops
            checked += 1
    assert checked == (5 ** 7 - 1) // 4 == 19531


def test_random_rows():
    rng = np.random.default_rng(7)
    lengths = [0, 1, 2, 3000] + [int(x) for x in rng.integers(0, 3001, 1996)]
    alphabet = np.frombuffer(b"=XIDS", dtype=np.uint8)
    all_s = 0
    for k, m in enumerate(lengths):
        p = [[0.8, 0.05, 0.05, 0.05, 0.05], [0.2] * 5, [0.3, 0.0, 0.3, 0.3, 0.1], [0.0, 0.0, 0.0, 0.0, 1.0]][k % 4 if k % 40 else 3]
        ops = bytes(rng.choice(alphabet, size=m, p=p))
        if k % 3 == 0:                                           # soft clips where the extension puts them
            ops = b"S" * int(rng.integers(0, 50)) + ops + b"S" * int(rng.integers(0, 50))
        assert mapper.aln_summary_host(ops) == ref.summary(ops), (k, m)
        all_s += bool(ops) and ops.count(b"S") == len(ops)
    assert all_s > 20
    assert mapper.aln_summary_host(b"SSSS") == dict(ref.ZERO, clip_left=4)


def test_foreign_bytes_are_counted_nowhere():
    for ops in (b"\0", b"M", b"==M==", b"IIMII", b"DD\xffDD", b"SSNSS", b"NSS==SSN", b"S" * 5 + b"H" + b"S" * 3, b"I" + bytes(range(256)) + b"I"):
        got = mapper.aln_summary_host(ops)
        assert got == ref.summary(ops), ops
    assert mapper.aln_summary_host(b"IIMII") == dict(ref.ZERO, n_ins=4, ins_runs=2)
    assert mapper.aln_summary_host(b"SSNSS") == dict(ref.ZERO, clip_left=2, clip_right=2)
    # an 'I' run right behind a 'D' run is a run of its own; the classic mode's 'I' tail is one run of insertions
    assert mapper.aln_summary_host(b"==DDII==I" + b"I" * 40) == dict(ref.ZERO, n_eq=4, n_del=2, n_ins=43, ins_runs=2, del_runs=1)


# ---------------------------------------------------------------------------------------------------------
# (b) the records on real alignments
# ---------------------------------------------------------------------------------------------------------
def test_nm_is_the_score_on_the_constructed_alignments():
    """docs/GACT_SPEC.md defines the score as the edit distance of the ops."""
    n = tails = 0
    for c in gact_cases.cases():
        score, ops, _ = orc.gact(c["q"], c["d"], c["T"], c["O"], c["W"])
        if score == -1:
            continue
        s = mapper.aln_summary_host(ops)
        assert s == ref.summary(ops), c["name"]
        assert ref.nm(s) == score, (c["name"], s, score)
        assert ref.block_len(s) == len(ops) and s["clip_left"] == s["clip_right"] == 0
        assert s["n_eq"] + s["n_x"] + s["n_ins"] == len(c["q"]) and ref.target_span(s) <= len(c["d"])
        tails += ops.endswith(b"II") and len(c["q"]) > len(c["d"])
        n += 1
    assert n > 150 and tails > 5


TEXT, MTA, CASES = anchored_cases.cases()


@pytest.mark.parametrize("P,B", [(0, 0), (1, 1), (5, 40)])
def test_clips_and_nm_after_end_clipping(P, B):
    clipped = 0
    for case in CASES:
        S, len_s = MTA[case["seq"]]
        e = clip_ref.extend_clipped(case["read"], TEXT, case["L"], S, len_s, min_len=case["min_len"], P=P, B=B)
        s = mapper.aln_summary_host(e["ops"])
        assert s == ref.summary(e["ops"]), case["name"]
        assert ref.nm(s) == e["score"], case["name"]
        assert (s["clip_left"], s["clip_right"]) == (e["clip_left"], e["clip_right"]), case["name"]
        assert s["clip_left"] + s["n_eq"] + s["n_x"] + s["n_ins"] + s["clip_right"] == len(case["read"])
        clipped += e["clip_left"] > 0 or e["clip_right"] > 0
    assert clipped > 3


# ---------------------------------------------------------------------------------------------------------
# (c) PAF text and the boundary
# ---------------------------------------------------------------------------------------------------------
def _batch(tmp_path, recs):
    p = tmp_path / "r.fq"
    p.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (nm, s, q) for nm, s, q in recs))
    rd = textio.Reader(p)
    assert rd.next(100) == len(recs)
    return rd, rd.batch


def test_paf_lines(tmp_path):
    rng = np.random.default_rng(12)
    tn = ((b"chrA", 0, 100000), (b"chrB", 200000, 50000))
    mta = textio.mta_table(tn)
    # 0: forward, clipped on the left only; 1: reverse, clipped on the left (of the ops) only; 2: unmapped (no locus);
    # 3: reverse, clipped on the right only, gaps; 4: unmapped (score -1); 5: forward, 'S' only: a zero denominator; 6: forward, gaps
    ops = [b"S" * 100 + b"=" * 500 + b"X" + b"=" * 299,
           b"S" * 30 + b"=" * 200 + b"X" + b"=" * 169,
           b"=" * 300,
           b"=" * 100 + b"DDD" + b"=" * 50 + b"II" + b"D" + b"=" * 88 + b"X" * 2 + b"=" * 8 + b"S" * 50,
           b"=" * 250,
           b"S" * 120,
           b"=" * 10 + b"I" + b"=" * 10 + b"I" * 7 + b"=" * 72]
    qlen = [900, 400, 300, 300, 250, 120, 100]
    for o, q in zip(ops, qlen):
        assert len(o) - o.count(b"D") == q
    score = np.array([1, 1, 0, 8, -1, 0, 8], dtype=np.int32)
    meta_r = np.array([1, 1, 0, 1, 1, 1, 1], dtype=np.int32)
    meta = np.zeros(7, dtype=mapper.META_DT)
    meta["seq_id"], meta["off"], meta["strand"] = [0, 1, 0, 1, 0, 0, 1], [17, 2017, 4017, 49000, 5, 77, 0], [0, 1, 0, 1, 0, 0, 0]
    seqs = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, k)) for k in qlen]
    rd, b = _batch(tmp_path, [(b"q%d" % i, seqs[i], b"F" * qlen[i]) for i in range(7)])
    sums = np.zeros(7, dtype=mapper.SUMMARY_DT)
    for i, o in enumerate(ops):
        for f, v in ref.record(o, int(score[i]), int(meta_r[i])).items():
            sums[f][i] = v
    mq = np.zeros(7, dtype=mapper.MAPQ_DT)
    mq["n1"], mq["n2"], mq["mapq"] = [31, 12, 0, 9, 5, 3, 40], [2, 12, 0, 0, 1, 3, 0], [56, 0, 0, 54, 33, 0, 60]
    texts = [ref.sam_ref.rle(o).encode() for o in ops]

    def fmt(is_text, mqp):
        cig, keep = textio.cigar_array(ops, score, texts if is_text else None)
        got = textio.paf_format(b, mta, cig, score, meta, meta_r, 7, sums, is_text=is_text, mapq=mqp)
        assert got is not None
        return got

    for with_mq in (False, True):
        want = "".join(ref.paf_line("q%d" % i, qlen[i], int(meta["strand"][i]), tn[meta["seq_id"][i]][0].decode(), tn[meta["seq_id"][i]][2],
                                    int(meta["off"][i]), ops[i], int(score[i]), int(meta_r[i]),
                                    (int(mq["mapq"][i]), int(mq["n1"][i]), int(mq["n2"][i])) if with_mq else None) for i in range(7))
        for is_text in (False, True):
            assert fmt(is_text, mq if with_mq else None) == want, (with_mq, is_text)
    lines = [l.split("\t") for l in want.splitlines()]
    assert [l[0] for l in lines] == ["q0", "q1", "q3", "q5", "q6"]                   # the unmapped reads print nothing
    # the lines by hand: a swapped qstart / qend on the reverse strand would show
    assert lines[0][1:12] == ["900", "100", "900", "+", "chrA", "100000", "17", "817", "799", "800", "56"]
    assert lines[1][1:12] == ["400", "0", "370", "-", "chrB", "50000", "2017", "2387", "369", "370", "0"]
    assert lines[2][1:12] == ["300", "50", "300", "-", "chrB", "50000", "49000", "49252", "246", "254", "54"]
    assert lines[2][12:17] == ["NM:i:8", "ED:i:8", "tp:A:P", "de:f:%.4f" % (5 / 251), "cg:Z:100M3D50M2I1D98M50S"]
    assert lines[3][1:11] == ["120", "120", "120", "+", "chrA", "100000", "77", "77", "0", "0"] and lines[3][15] == "de:f:0.0000"
    assert lines[4][12:19] == ["NM:i:8", "ED:i:8", "tp:A:P", "de:f:%.4f" % (2 / 94), "cg:Z:10M1I10M7I72M", "v1:i:40", "v2:i:0"]
    assert textio.paf_format(b, mta, None, score, meta, meta_r, 7, None) is None            # the records are required
    rd.close()


def test_struct_sizes_and_entry_points():
    assert C.sizeof(capi.AlnSummary) == 32 == mapper.SUMMARY_DT.itemsize
    assert [f for f, _ in capi.AlnSummary._fields_] == list(ref.FIELDS) == list(mapper.SUMMARY_DT.names)
    assert C.sizeof(capi.BatchExtras) == 24 and capi.BatchExtras.mapq_out.offset == 8 and capi.BatchExtras.summary_out.offset == 16
    assert C.sizeof(capi.MapOptions) == 76 and lib.lrm_abi_version() == 3          # the records are asked for per call
    for name in ("lrm_aln_summary_dev", "lrm_aln_summary_host", "lrm_map_batch_submit_ex", "lrm_paf_format", "lrm_accaln_paf"):
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
    a = capi.AlnSummary(1, 2, 3, 4, 5, 6, 7, 8)
    lib.lrm_aln_summary_host(None, 0, C.byref(a))
    assert [getattr(a, f) for f in ref.FIELDS] == [0] * 8
    lib.lrm_aln_summary_host(b"==", -3, C.byref(a))
    assert [getattr(a, f) for f in ref.FIELDS] == [0] * 8


def test_paf_flow_refuses_split_reads(tmp_path):
    """Refused before anything is opened: no index files, no device needed."""
    opt = capi.map_options(anchored=1, clip=1, split=1)
    with pytest.raises(capi.LrmError) as refused:
        textio.accaln("/nonexistent/ref.fa", "/nonexistent/reads.fq", tmp_path / "o.paf", 64, options=opt, paf=True)
    assert refused.value.rc == -1 and b"split" in lib.lrm_last_error()
    assert not (tmp_path / "o.paf").exists()
