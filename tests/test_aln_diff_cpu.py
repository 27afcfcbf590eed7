"""Difference events and MD:Z on the host (docs/GACT_SPEC.md, "Difference events and MD:Z"): lrm_aln_diff_host -- which walks a
row through the kernel's own per-word step, aln_diff_step.h -- and lrm_md_format against tests/md_ref.py and against strings
written by hand; the round trip from read, M CIGAR and MD text back to the target span; the formatter; the struct."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import md_ref
from longreadmapper_amd import capi, mapper, textio
from longreadmapper_amd.capi import lib

TEXT = b"ACGT" * 8                     # position p holds "ACGT"[p % 4]

# (ops, loc, MD by hand); None: no alignment, no tag
CASES = [
    (b"=" * 10, 0, "10"),
    (b"=" * 17, 3, "17"),
    (b"==X=X==", 0, "2G1A2"),
    (b"==XX=", 0, "2G0T1"),
    (b"==DX=", 0, "2^G0T1"),
    (b"==XD=", 0, "2G0^T1"),
    (b"=DDIDD=", 0, "1^CG0^TA1"),
    (b"=DDDIID", 1, "1^GTA0^C0"),
    (b"SS==X==SSS", 0, "2G2"),
    (b"SSS=====", 2, "5"),
    (b"==N=X=", 0, "3T1"),
    (b"=DND=", 0, "1^C0^G1"),
    (b"X===D", 0, "0A3^A0"),
    (b"D===X", 1, "0^C3C0"),
    (b"", 0, None),
    (b"X", 0, "0A0"),
    (b"=", 0, "1"),
    (b"D", 2, "0^G0"),
    (b"I", 0, "0"),
    (b"S", 0, "0"),
    (b"===X", len(TEXT) - 4, "3T0"),                # the target runs to the text's last byte
    (b"===X", len(TEXT) - 3, "3\x000"),             # ... and one beyond it: never read, its byte is 0
    (b"==DD", len(TEXT) - 3, "2^T\x000"),
]


def _host(ops, content, loc):
    return mapper.aln_diff_host(ops, content[loc:])


@pytest.mark.parametrize("ops,loc,want", CASES)
def test_events_and_md_by_hand(ops, loc, want):
    assert md_ref.md(ops, TEXT, loc) == want
    ev = _host(ops, TEXT, loc)
    assert ev.tolist() == md_ref.events(ops, TEXT, loc)
    assert len(ev) == ops.count(b"X") + ops.count(b"D")
    if want is not None:
        assert textio.md_text(ev, md_ref.n_eq(ops)) == want
    # the text as the caller holds it ends right at the last aligned base: the same events where they are inside
    span = sum(ops.count(c) for c in b"=XD")
    if loc + span <= len(TEXT):
        assert mapper.aln_diff_host(ops, TEXT[loc:loc + span]).tolist() == ev.tolist()


def test_count_only_and_no_target():
    ops = b"==XD="
    assert lib.lrm_aln_diff_host(ops, len(ops), TEXT, len(TEXT), None) == 2
    assert lib.lrm_aln_diff_host(ops, 0, TEXT, len(TEXT), None) == 0 and lib.lrm_aln_diff_host(ops, -3, TEXT, len(TEXT), None) == 0
    ev = np.zeros(2, dtype=np.uint32)
    assert lib.lrm_aln_diff_host(ops, len(ops), None, 0, ev.ctypes.data) == 2
    assert ev.tolist() == [(0 << 8) | (2 << 10), (1 << 8) | (2 << 10)]            # no text: every base 0


def _put(row, at, piece):
    assert 0 <= at and at + len(piece) <= len(row)
    return row[:at] + piece + row[at + len(piece):]


def test_per_word_step_across_lane_and_step_edges():
    """Rows whose events straddle columns 16 (the lanes of a step) and 1024 (the steps of a row), and the columns before them
    shift the target by every residue."""
    rng = np.random.default_rng(3)
    content = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4000)])
    base = b"=" * 2100
    rows = []
    for e in (16, 1024, 2048):
        for piece in (b"X", b"XX", b"D", b"DD", b"DDDD", b"XD", b"DX", b"DID", b"DDII", b"IIDD", b"XIX", b"DSD", b"X=X", b"DNX"):
            for at in range(e - len(piece), e + 1):
                rows.append(_put(base, at, piece))
        for lead in range(0, 17):                                   # 'I' columns in front: the lane's first target byte moves
            rows.append(_put(_put(base, 0, b"I" * lead), e - 2, b"XDDX"))
    rows += [bytes(rng.choice(np.frombuffer(b"=XIDS", dtype=np.uint8), size=m, p=[0.6, 0.1, 0.1, 0.1, 0.1])) for m in (15, 16, 17, 1023, 1024, 1025, 2049)]
    rows += [b"X" * 2049, b"D" * 2049, b"I" * 2049, b"S" * 2049]
    for k, ops in enumerate(rows):
        loc = k % 16 + 1
        got = _host(ops, content, loc)
        assert got.tolist() == md_ref.events(ops, content, loc), (k, ops[:40])
        assert textio.md_text(got, md_ref.n_eq(ops)) == md_ref.md(ops, content, loc), k
    assert len(rows) > 200


def test_round_trip_to_the_target_span():
    rng = np.random.default_rng(11)
    content = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 6000)])
    kinds = set()
    for k in range(200):
        span = int(rng.integers(1, 400))
        loc = int(rng.integers(0, len(content) - span + 1)) if k % 10 else len(content) - span       # (every tenth ends on the last byte)
        read, ops = md_ref.mutate(rng, content, loc, span)
        ev = _host(ops, content, loc)
        assert ev.tolist() == md_ref.events(ops, content, loc), k
        text = textio.md_text(ev, md_ref.n_eq(ops))
        assert text == md_ref.md(ops, content, loc), k
        assert md_ref.target_from_md(read, md_ref.m_cigar(ops), text) == content[loc:loc + span], k
        kinds |= set(ops)
    assert kinds == set(b"=XIDS")


def test_md_format_buffer():
    ev = np.array(md_ref.events(b"=" * 10 + b"X" + b"X" + b"=" * 5, b"A" * 10 + b"AC" + b"A" * 5, 0), dtype=np.uint32)
    want = b"10A0C5"
    buf = C.create_string_buffer(b"\xab" * 16, 16)
    assert lib.lrm_md_format(ev.ctypes.data, len(ev), 15, buf, len(want) + 1) == len(want)
    assert buf.raw[:len(want) + 1] == want + b"\0" and buf.raw[len(want) + 1] == 0xAB
    assert lib.lrm_md_format(ev.ctypes.data, len(ev), 15, buf, len(want)) < 0           # one too small: the NUL has no place
    assert lib.lrm_md_format(None, 0, 7, buf, 2) == 1 and buf.raw[:2] == b"7\0"
    assert lib.lrm_md_format(None, 0, 7, buf, 1) < 0
    assert textio.md_text(mapper.aln_diff_host(b"=====DD=", b"AAAAAACT"), 6) == "5^AC1"
    assert textio.md_text(mapper.aln_diff_host(b"=====X" + b"D" + b"===", b"AAAAAACGGG"), 8) == "5A0^C3"


def _batch(tmp_path):
    p = tmp_path / "r.fq"
    p.write_bytes(b"@q0\nACGTAC\n+\nIIIIII\n@q1\nGGGG\n+\n####\n@q2\nTT\n+\n!!\n@q3\nACG\n+\n;;;\n")
    rd = textio.Reader(p)
    assert rd.next(10) == 4
    return rd


def test_sam_format_md(tmp_path):
    pymta = [("chrA", 0, 1000), ("contig_two", 2000, 321)]
    mta = textio.mta_table(pymta)
    rd = _batch(tmp_path)
    content = b"ACGTACGTAC"
    ops = [b"==X=I=", b"=D===", b"", b"==="]
    locs = [0, 2, 0, 0]
    score = np.array([2, 1, -1, 0], dtype=np.int32)
    cig, _keep = textio.cigar_array(ops, score)
    meta_r = np.array([1, 1, 1, 0], dtype=np.int32)
    meta = np.zeros(4, dtype=mapper.META_DT)
    meta["seq_id"], meta["off"], meta["strand"] = [0, 1, 0, -1], [41, 7, 3, 0], [0, 1, 0, 0]
    mq = np.zeros(4, dtype=mapper.MAPQ_DT)
    mq["n1"], mq["n2"], mq["mapq"] = [9, 8, 0, 0], [1, 8, 0, 0], [48, 0, 0, 0]
    args = (rd.batch, mta, cig, score, meta, meta_r, 4)
    # NULL events: exactly the lines of lrm_sam_format_mapq
    for m in (None, mq):
        assert textio.sam_format(*args, mapq=m, entry="lrm_sam_format_md") == textio.sam_format(*args, mapq=m, entry="lrm_sam_format_mapq")
    summ = np.zeros(4, dtype=mapper.SUMMARY_DT)
    evs, off, cnt = [], np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint32)
    for i, o in enumerate(ops):
        s = mapper.aln_summary_host(o) if score[i] != -1 and meta_r[i] != 0 else {}
        for f, v in s.items():
            summ[f][i] = v
        e = md_ref.events(o, content, locs[i], int(score[i]), int(meta_r[i]))
        off[i], cnt[i] = len(evs), len(e)
        evs += e
    events = np.array(evs + [0], dtype=np.uint32)
    for m in (None, mq):
        plain = textio.sam_format(*args, mapq=m, entry="lrm_sam_format_mapq").splitlines()
        got = textio.sam_format(*args, mapq=m, md=(summ, off, cnt, events)).splitlines()
        assert got[0] == plain[0] + "\tNM:i:2\tMD:Z:2G2" and got[1] == plain[1] + "\tNM:i:1\tMD:Z:1^T3"
        assert got[2:] == plain[2:]                                 # no alignment, no locus: no tag at all
        assert got[0].split("\t")[-3].startswith("v2:i:" if m is not None else "ED:I:")
    off[1] = capi.DIFF_NO_ROOM                                      # a read whose events found no room prints no tag
    got = textio.sam_format(*args, md=(summ, off, cnt, events)).splitlines()
    assert got[1] == textio.sam_format(*args, entry="lrm_sam_format_mapq").splitlines()[1]
    rd.close()


def test_struct_and_abi():
    assert lib.lrm_abi_version() == 3 and capi.N_KERNELS == 9
    assert C.sizeof(capi.BatchExtras) == 24 and C.sizeof(capi.MapOptions) == 76
    d = capi.BatchDiff
    assert C.sizeof(d) == 48
    assert [(getattr(d, f).offset, getattr(d, f).size) for f, _ in d._fields_] == [(0, 4), (4, 4), (8, 8), (16, 8), (24, 8), (32, 8), (40, 8)]
    assert capi.LATER_STRUCTS[d] == "lrm_batch_diff" and d not in capi.STRUCTS
    # no Structure of records.py escapes both lists (the anonymous tail of MapOptions is part of lrm_map_options)
    from longreadmapper_amd import records
    every = {v for v in vars(records).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert every - set(records.STRUCTS) - set(records.LATER_STRUCTS) == {records._SplitWords}


def test_struct_agrees_with_the_header(tmp_path):
    """sizeof and offsetof of every member of every later struct as the host C compiler reads include/lrm_accel.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrm_accel.h"', '#include "lrm_io_host.h"', 'int main(void) {']
    for s, c_name in capi.LATER_STRUCTS.items():
        lines.append('    printf("sizeof %s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f, c_name, f) for f, _ in s._fields_]
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    says = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    for s, c_name in capi.LATER_STRUCTS.items():
        assert C.sizeof(s) == says["sizeof " + c_name]
        for f, _ in s._fields_:
            assert getattr(s, f).offset == says["%s.%s" % (c_name, f)], (c_name, f)
    assert (capi.DIFF_X, capi.DIFF_D_OPEN, capi.DIFF_D_MORE) == (0, 1, 2) and capi.DIFF_NO_ROOM == 2**64 - 1
    for name in ("lrm_aln_diff_offsets_dev", "lrm_aln_diff_dev", "lrm_aln_diff_host", "lrm_md_format", "lrm_map_batch_submit_ex2",
                 "lrm_sam_format_md", "lrm_accaln_md"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
