"""lrm_sam_format_secondary without a GPU (docs/GACT_SPEC.md, "Secondary alignments"): hand-made results give one FLAG 256 line
behind the lines of every read with a reported secondary, built here field by field; every other line is unchanged; a NULL
table gives the text of lrm_sam_format_md."""
import ctypes as C

import numpy as np

import sam_ref
from longreadmapper_amd import capi, mapper, textio
from longreadmapper_amd.capi import lib


def _batch(tmp_path, recs):
    p = tmp_path / "r.fq"
    p.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (nm, s, q) for nm, s, q in recs))
    rd = textio.Reader(p)
    assert rd.next(100) == len(recs)
    return rd, rd.batch


def _secondary_out(table, ops, score, meta, texts=None):
    k = len(table)
    cig, keep = textio.cigar_array(ops, score, texts)
    meta_r = np.ones(k, dtype=np.int32)
    out = capi.SecondaryOut(k, k, table.ctypes.data, None, 0, None, None, cig.ctypes.data, None, 0, score.ctypes.data, meta.ctypes.data,
                            meta_r.ctypes.data, None, None)
    return out, (cig, keep, meta_r)


def test_flag_256_lines(tmp_path):
    rng = np.random.default_rng(17)
    mta = textio.mta_table([(b"chrA", 0, 100000), (b"chrB", 200000, 50000)])
    lens = [900, 400, 300, 250, 500]
    seqs = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, k)) for k in lens]
    quals = [bytes(33 + (i + j) % 60 for j in range(k)) for i, k in enumerate(lens)]
    # read 0: a reported right segment AND a reported secondary; 1: reverse strand, secondary on the reverse strand, soft clips;
    # 2: a duplicate (not reported); 3: unmapped, no candidate; 4: a candidate whose extension failed (flags 0)
    ops = [b"=" * 600 + b"S" * 300, b"=" * 200 + b"X" + b"=" * 199, b"=" * 300, b"", b"=" * 500]
    score = np.array([3, 1, 0, -1, 0], dtype=np.int32)
    meta_r = np.array([1, 1, 1, 1, 1], dtype=np.int32)
    meta = np.zeros(5, dtype=mapper.META_DT)
    meta["seq_id"], meta["off"], meta["strand"] = [0, 1, 0, 0, 0], [17, 2017, 4017, 0, 9000], [0, 1, 0, 0, 0]
    rd, b = _batch(tmp_path, [(b"q%d" % i, seqs[i], quals[i]) for i in range(5)])
    cig, keep1 = textio.cigar_array(ops, score)
    seg = np.zeros(1, dtype=mapper.SEGMENT_DT)
    seg[0] = (0, 600, 300, capi.SEG_RIGHT | capi.SEG_ALIGNED)
    rows = np.zeros((1, 320), dtype=np.uint8)
    rows[0, :300] = np.frombuffer(seqs[0][600:], dtype=np.uint8)
    sscore, smeta_r = np.array([7], dtype=np.int32), np.array([1], dtype=np.int32)
    smeta = np.zeros(1, dtype=mapper.META_DT)
    smeta["seq_id"], smeta["off"] = 1, 5000
    scig, keep2 = textio.cigar_array([b"=" * 300], sscore)
    split = capi.SplitOut(1, 1, seg.ctypes.data, rows.ctypes.data, 320, None, None, scig.ctypes.data, None, 0,
                          sscore.ctypes.data, smeta.ctypes.data, smeta_r.ctypes.data, None, None)
    rec = np.zeros(5, dtype=mapper.MAPQ_DT)
    rec["n1"], rec["n2"], rec["mapq"], rec["radius"] = [31, 12, 9, 5, 20], [20, 12, 9, 1, 15], [21, 0, 0, 33, 15], 512

    table = np.zeros(4, dtype=mapper.SECONDARY_DT)
    table["read"], table["hits"] = [0, 1, 2, 4], [9, 8, 8, 8]
    table["flags"] = [capi.SEC_ALIGNED, capi.SEC_ALIGNED, capi.SEC_DUPLICATE, 0]
    sec_ops = [b"=" * 450 + b"I" * 2 + b"=" * 448, b"S" * 30 + b"=" * 100 + b"D" * 3 + b"X" + b"=" * 249 + b"S" * 20, b"=" * 300, b"=" * 500]
    sec_score = np.array([2, 4, 0, -1], dtype=np.int32)
    sec_meta = np.zeros(4, dtype=mapper.META_DT)
    sec_meta["seq_id"], sec_meta["off"], sec_meta["strand"] = [1, 0, 0, 0], [30_000, 70_123, 4100, 0], [0, 1, 0, 0]
    sec, keep3 = _secondary_out(table, sec_ops, sec_score, sec_meta)

    def line(i, s):                                    # the expected line of candidate s of read i, field by field
        flag = 256 + (16 if sec_meta["strand"][s] else 0)
        rname = ("chrA", "chrB")[int(sec_meta["seq_id"][s])]
        return "\t".join(["q%d" % i, str(flag), rname, str(int(sec_meta["off"][s]) + 1), "0", sam_ref.rle(sec_ops[s]), "*", "0", "0", "*", "*",
                          "ED:I:%d" % sec_score[s], "tp:A:S"])

    assert sam_ref.rle(sec_ops[1]) == "30S100M3D250M20S"
    for split_arg in (None, split):
        for mq in (None, rec):
            kw = dict(split=split_arg, mapq=mq)
            base = textio.sam_format(b, mta, cig, score, meta, meta_r, 5, entry="lrm_sam_format_md", **kw)
            assert textio.sam_format(b, mta, cig, score, meta, meta_r, 5, entry="lrm_sam_format_secondary", **kw) == base      # NULL table
            got = textio.sam_format(b, mta, cig, score, meta, meta_r, 5, secondary=sec, **kw).splitlines()
            want = []
            for ln in base.splitlines():
                want.append(ln)
                nxt = base.splitlines()[len(want)] if len(want) < len(base.splitlines()) else ""
                i = int(ln.split("\t")[0][1:])
                if nxt.split("\t")[0] != "q%d" % i and i in (0, 1):       # behind the read's last line
                    want.append(line(i, i))
            assert got == want
            assert [x.split("\t")[1] for x in got if int(x.split("\t")[1]) & 256] == ["256", "272"]
            assert len(got) == len(base.splitlines()) + 2
    # run-length text in place of op bytes (lrm_map_options.cigar_text)
    tcig, keep4 = textio.cigar_array(ops, score, [sam_ref.rle(o).encode() if o else b"*" for o in ops])
    tsec, keep5 = _secondary_out(table, sec_ops, sec_score, sec_meta, [sam_ref.rle(o).encode() for o in sec_ops])
    text = textio.sam_format(b, mta, tcig, score, meta, meta_r, 5, is_text=1, secondary=tsec)
    assert text == textio.sam_format(b, mta, cig, score, meta, meta_r, 5, secondary=sec)
    # an empty table is no table; a table without its arrays is refused
    empty = capi.SecondaryOut(0, 0, None, None, 0, None, None, None, None, 0, None, None, None, None, None)
    assert textio.sam_format(b, mta, cig, score, meta, meta_r, 5, secondary=empty) == textio.sam_format(b, mta, cig, score, meta, meta_r, 5, entry="lrm_sam_format_md")
    bad = capi.SecondaryOut(4, 4, table.ctypes.data, None, 0, None, None, None, None, 0, None, None, None, None, None)
    assert textio.sam_format(b, mta, cig, score, meta, meta_r, 5, secondary=bad) is None and b"lrm_secondary_out" in lib.lrm_last_error()
    assert "lrm_sam_format_secondary" in capi.SYMBOLS and capi.LATER_STRUCTS[capi.SecondaryOut] == "lrm_secondary_out"
    assert C.sizeof(capi.SecondaryOut) == 15 * 8
    rd.close()
