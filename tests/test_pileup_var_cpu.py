"""The variant rule of the pileup on the host (docs/GACT_SPEC.md, "Pileup variants and VCF"): the constructed positions reach
their edges; lrm_pileup_variants_host -- the kernels' own rule as plain C++ -- equals tests/pileup_var_ref.py on every case
and on random records, for equality; the table's bounds; the refusals; the VCF text and header; the record's layout by a
compiled C program; a stand-alone sanitizer build of the rule, run as a child process; the planted workload of the GPU test
proved on the oracle."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import orc
import pileup_call_cases as KC
import pileup_call_ref as R
import pileup_var_cases as K
import pileup_var_ref as V
from longreadmapper_amd import capi, index, textio
from longreadmapper_amd.capi import lib

FILL = 0xAB
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def as_cols(rows):
    out = np.zeros(len(rows), dtype=capi.PILEUP_COL_DT)
    ref = R.cols_array(rows)
    for f in ref.dtype.names:
        out[f] = ref[f]
    return out


def variant_options(opt):
    """(min_depth, min_count, min_pct, reserved, hom_pct[, reserved3]) -> lrm_pileup_variant_options"""
    return capi.PileupVariantOptions(capi.PileupCallOptions(*opt[:4]), opt[4], tuple(opt[5]) if len(opt) > 5 else (0, 0, 0))


def host_variants(cols, words, content, pos0, opt=None, cap=None, pad=2):
    """lrm_pileup_variants_host into a table that lies in fill -> (records, total, the bytes outside out[0 .. min(total, cap)))"""
    cols = np.ascontiguousarray(cols, dtype=capi.PILEUP_COL_DT)
    n = len(cols)
    ins_cols = 0 if words is None else words.shape[1]
    flat = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1) if ins_cols else None
    content = np.frombuffer(bytes(content), dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)
    cap = 3 * n + 1 if cap is None else cap
    buf = np.full(48 * (cap + 2 * pad), FILL, dtype=np.uint8)
    o = variant_options(opt) if opt is not None else None
    total = lib.lrm_pileup_variants_host(cols.ctypes.data if n else None, flat.ctypes.data if ins_cols and n else None, ins_cols, content.ctypes.data, pos0, n,
                                         C.byref(o) if o is not None else None, buf.ctypes.data + 48 * pad if cap else None, cap)
    if total < 0:
        return None, total, None
    k = min(total, cap)
    recs = buf[48 * pad:48 * (pad + k)].copy().view(capi.PILEUP_VARIANT_DT)
    return recs, total, np.concatenate([buf[:48 * pad], buf[48 * (pad + k):]])


def sliced(c):
    """a case's range: (rows, text, words, pos0) of [first, first + count)"""
    first = 0 if c.first is None else c.first
    count = len(c.rows) - first if c.count is None else c.count
    words = None if c.words is None else c.words[first:first + count]
    return c.rows[first:first + count], c.text[first:first + count], words, K.POS0 + first


def ref_of(c):
    rows, text, words, pos0 = sliced(c)
    return V.variants(R.cols_array(rows), words, text, pos0, V.options(*c.opt))


# ---------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------
def test_cases_reach_their_edges():
    names = [c.name for c in K.CASES]
    assert len(set(names)) == len(names) >= 30
    missed = [c.name for c in K.CASES if not c.reaches(ref_of(c))]
    assert not missed, missed
    assert all(V.options(*o) is None for o in K.REFUSED) and V.options(*K.DEF) == ((8, 4, 25), 70)


def test_host_rule_on_every_case():
    bad = []
    for c in K.CASES:
        rows, text, words, pos0 = sliced(c)
        want = ref_of(c)
        got, total, outside = host_variants(as_cols(rows), words, text, pos0, c.opt)
        if total != len(want) or V.as_tuples(got) != want or not (outside == FILL).all():
            bad.append((c.name, total, V.as_tuples(got), want))
    assert not bad, (len(bad), bad[:3])
    # options NULL: the defaults
    c = K.CASES[0]
    assert V.as_tuples(host_variants(as_cols(c.rows), None, c.text, K.POS0, None)[0]) == ref_of(c)


def test_table_bounds():
    """cap 0 with a NULL table, cap between the records of one position, cap at and above the total: nothing from cap on,
    nothing outside the table"""
    by = {c.name: c for c in K.CASES}
    c = by["all-three-kinds"]
    want = ref_of(c)
    assert len(want) == 3 and len({r[0] for r in want}) == 1
    for cap in (0, 1, 2, 3, 4, 10):
        got, total, outside = host_variants(as_cols(c.rows), c.words, c.text, K.POS0, c.opt, cap=cap)
        assert total == 3 and V.as_tuples(got) == want[:cap] and (outside == FILL).all(), cap
    rows = [K.D_, K.C_] * 20
    want = V.variants(R.cols_array(rows), None, b"A" * 40, 7, V.options())
    for cap in (0, 19, 20, 21):
        got, total, outside = host_variants(as_cols(rows), None, b"A" * 40, 7, cap=cap)
        assert total == 20 and V.as_tuples(got) == want[:cap] and (outside == FILL).all(), cap
    assert host_variants(as_cols([]), None, b"", 0)[1] == 0


def test_host_rule_on_random_records():
    n = 2000
    for ins_cols, seed in ((0, 1), (1, 2), (4, 3), (8, 4)):
        rows, text, words = K.random_records(n, ins_cols, seed)
        for opt in (K.DEF, (3, 2, 10, 0, 40)):
            want = V.variants(R.cols_array(rows), words, text, 12345, V.options(*opt))
            got, total, outside = host_variants(as_cols(rows), words, text, 12345, opt)
            kinds = [r[6] for r in want]
            assert min(kinds.count(k) for k in (V.SNV, V.DEL, V.INS)) > 50 and max(r[1] for r in want if r[6] == V.DEL) >= 8
            assert {r[9] for r in want} == {1, 2}
            assert total == len(want) and V.as_tuples(got) == want and (outside == FILL).all(), (ins_cols, opt)
        # a range cut out of the middle is the rule on that range alone
        for a, b in ((1, n), (777, 1290), (n - 1, n)):
            want = V.variants(R.cols_array(rows[a:b]), None if words is None else words[a:b], text[a:b], a, V.options())
            got, total, _ = host_variants(as_cols(rows[a:b]), None if words is None else words[a:b], text[a:b], a)
            assert total == len(want) and V.as_tuples(got) == want


def test_refusals():
    c = K.CASES[0]
    cols = as_cols(c.rows)
    for o in K.REFUSED:
        assert host_variants(cols, None, c.text, 0, o)[1] < 0, o
        assert any(w in lib.lrm_last_error() for w in (b"min_pct", b"reserved", b"hom_pct")), o
    out = np.zeros(48 * 4, dtype=np.uint8)
    one = np.zeros(4 * 9 * 3, dtype=np.uint32)
    text = np.frombuffer(c.text, dtype=np.uint8).copy()
    assert lib.lrm_pileup_variants_host(cols.ctypes.data, None, 4, text.ctypes.data, 0, 3, None, out.ctypes.data, 4) < 0 and b"null argument" in lib.lrm_last_error()
    assert lib.lrm_pileup_variants_host(cols.ctypes.data, one.ctypes.data, 9, text.ctypes.data, 0, 3, None, out.ctypes.data, 4) < 0 and b"insertion columns" in lib.lrm_last_error()
    assert lib.lrm_pileup_variants_host(cols.ctypes.data, None, 0, text.ctypes.data, 0, 3, None, None, 4) < 0
    assert lib.lrm_pileup_variants_host(None, None, 0, text.ctypes.data, 0, 3, None, out.ctypes.data, 4) < 0
    assert lib.lrm_pileup_variants_host(cols.ctypes.data, None, 0, None, 0, 3, None, out.ctypes.data, 4) < 0
    assert lib.lrm_pileup_variants_host(None, None, 0, None, 0, 0, None, None, 0) == 0


# ---------------------------------------------------------------------------------------------------------
# the text
# ---------------------------------------------------------------------------------------------------------
def three_sequences():
    seqs = [b"ACGTTGCAAC", b"ggcatTACGT", b"TTGACCA"]
    hi = index.HostIndex.build(seqs, names=["chr1", "second", "c"], hlen=3)
    return hi, seqs, [(int(hi.h.mta[s].offset), int(hi.h.mta[s].seq_len)) for s in range(3)]


def variant(pos, kind, ln=1, depth=20, n_ref=5, n_alt=15, ref=ord("A"), alt=0, gt=2, bases=b"", flags=0, n_col0=0):
    return (pos, ln, depth, n_ref, n_alt, n_col0, kind, ref, alt, gt, bases, flags)


def as_records(tuples):
    out = np.zeros(len(tuples), dtype=capi.PILEUP_VARIANT_DT)
    for k, t in enumerate(tuples):
        for f, v in zip(V.FIELDS[:10], t[:10]):
            out[k][f] = v
        out[k]["bases"][:len(t[10])] = list(t[10])
        out[k]["ins_flags"] = t[11]
    return out


def test_vcf_lines():
    hi, seqs, where = three_sequences()
    o1, o2, o3 = (w[0] for w in where)
    recs = [
        variant(o1 + 3, V.SNV, ref=ord("T"), alt=ord("G"), gt=1, n_ref=12, n_alt=8),
        variant(o1 + 4, V.DEL, ln=3, ref=ord("T")),                                     # TGC behind the T of position 4 (1-based)
        variant(o1 + 9, V.INS, ln=2, ref=ord("C"), bases=b"GT", flags=1),
        variant(o2 + 0, V.DEL, ln=2, ref=ord("g")),                                     # on the sequence's first base: lower-case text
        variant(o2 + 2, V.SNV, ref=ord("c"), alt=ord("A")),                             # a lower-case text byte prints in upper case
        variant(o2 + 2, V.INS, ln=0, ref=ord("c"), gt=1),                               # no allele: <INS>
        variant(o2 + 8, V.DEL, ln=2, ref=ord("G")),                                     # ends on the sequence's last base
        variant(o3 + 1, V.INS, ln=8, ref=ord("T"), bases=b"ACGTACGT", flags=3, depth=4000000000, n_ref=7, n_alt=3999999993),
        variant(o3 + 6, V.DEL, ln=1, ref=ord("A")),
    ]
    want = ["chr1\t4\t.\tT\tG\t.\t.\tDP=20\tGT:AD\t0/1:12,8\n", "chr1\t4\t.\tTTGC\tT\t.\t.\tDP=20\tGT:AD\t1/1:5,15\n",
            "chr1\t10\t.\tC\tCGT\t.\t.\tDP=20\tGT:AD\t1/1:5,15\n", "second\t1\t.\tGGC\tC\t.\t.\tDP=20\tGT:AD\t1/1:5,15\n",
            "second\t3\t.\tC\tA\t.\t.\tDP=20\tGT:AD\t1/1:5,15\n", "second\t3\t.\tC\t<INS>\t.\t.\tDP=20\tGT:AD\t0/1:5,15\n",
            "second\t8\t.\tCGT\tC\t.\t.\tDP=20\tGT:AD\t1/1:5,15\n",
            "c\t2\t.\tT\tTACGTACGT\t.\t.\tDP=4000000000;INSFULL\tGT:AD\t1/1:7,3999999993\n", "c\t6\t.\tCA\tC\t.\t.\tDP=20\tGT:AD\t1/1:5,15\n"]
    # the lines assembled here agree with the reference's formatter, and the library prints them
    names = ("chr1", "second", "c")
    ref_lines = []
    for r in recs:
        s = max(k for k in range(3) if where[k][0] <= r[0])
        ref_lines.append(V.vcf_line(names[s], r[0] - where[s][0], where[s][1], seqs[s], r))
    assert ref_lines == want
    assert textio.vcf_text(hi, as_records(recs)).decode() == "".join(want)
    pos1 = [int(line.split("\t")[1]) for line in want]
    assert pos1[:3] == sorted(pos1[:3]) and pos1[3:7] == sorted(pos1[3:7])                # DEL, SNV, INS of a position stay sorted
    # a buffer one byte short of a line's room is refused; a record in no sequence, a run that leaves its sequence, a bad kind
    records = as_records(recs)
    buf = C.create_string_buffer(4096)
    fmt = lambda rec, room: lib.lrm_pileup_variants_format_vcf(hi.h.mta, hi.mta_len, hi.h.content, rec.ctypes.data, len(rec), buf, room)  # noqa: E731
    assert fmt(records, 4096) == len("".join(want))
    assert fmt(records, 200) < 0 and b"too small" in lib.lrm_last_error()
    assert fmt(records[:1], len(want[0])) < 0 and fmt(records[:1], 1) < 0
    for bad in (variant(o3 + 7, V.SNV), variant(o1 + 8, V.DEL, ln=3), variant(o3 + 0, V.DEL, ln=7), variant(o1, 3), variant(o1, V.DEL, ln=0)):
        assert fmt(as_records([bad]), 4096) < 0, bad
    assert fmt(as_records([variant(o3 + 0, V.DEL, ln=6)]), 4096) > 0                      # ... the base behind it is the sequence's last
    assert lib.lrm_pileup_variants_format_vcf(hi.h.mta, hi.mta_len, hi.h.content, None, 0, buf, 16) == 0
    assert lib.lrm_pileup_variants_format_vcf(hi.h.mta, hi.mta_len, None, records.ctypes.data, 1, buf, 4096) < 0
    hi.close()


def test_vcf_header_and_file(tmp_path):
    hi, seqs, where = three_sequences()
    head = textio.vcf_header(hi, "reads-1").decode().splitlines()
    assert head[0] == "##fileformat=VCFv4.2"
    assert head[1:4] == ["##contig=<ID=chr1,length=10>", "##contig=<ID=second,length=10>", "##contig=<ID=c,length=7>"]
    assert len(head) == 1 + 3 + 6 and all(line.startswith("##") for line in head[:-1])
    assert [line.split("=<ID=")[1].split(",")[0] for line in head[4:9]] == ["DP", "INSFULL", "INS", "GT", "AD"]
    assert [line.split("=<")[0] for line in head[4:9]] == ["##INFO", "##INFO", "##ALT", "##FORMAT", "##FORMAT"]
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\treads-1"
    assert textio.vcf_header(hi).decode().splitlines()[-1].endswith("\tSAMPLE")
    buf = C.create_string_buffer(64)
    assert lib.lrm_vcf_header(hi.h.mta, hi.mta_len, None, buf, 64) < 0 and b"too small" in lib.lrm_last_error()
    big = C.create_string_buffer(4096)
    k = lib.lrm_vcf_header(hi.h.mta, hi.mta_len, None, big, 4096)
    assert big.raw[:k] == textio.vcf_header(hi) and lib.lrm_vcf_header(hi.h.mta, hi.mta_len, None, big, k) < 0
    assert lib.lrm_vcf_header(hi.h.mta, hi.mta_len, None, big, k + 1) == k
    recs = as_records([variant(where[0][0] + 3, V.SNV, ref=ord("T"), alt=ord("G")), variant(where[2][0] + 6, V.DEL, ref=ord("A"))])
    assert textio.write_vcf(str(tmp_path / "v.vcf"), hi, recs, sample="s", chunk=1) == 2
    assert open(tmp_path / "v.vcf", "rb").read() == textio.vcf_header(hi, "s") + textio.vcf_text(hi, recs)
    hi.close()


# ---------------------------------------------------------------------------------------------------------
# the record, the binding
# ---------------------------------------------------------------------------------------------------------
def test_record_layout_and_binding(tmp_path):
    """the 48-byte record and the options by the host C compiler: a small program of its own prints sizeof and offsetof"""
    fields = ("pos", "len", "depth", "n_ref", "n_alt", "n_col0", "kind", "ref", "alt", "gt", "bases", "ins_flags", "pad")
    src = tmp_path / "variant.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lrm_accel.h"\n#include "lrm_io_host.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu\\n", sizeof(lrm_pileup_variant), sizeof(lrm_pileup_variant_options), sizeof(lrm_accaln_vcf_options));\n'
                   + "".join('    printf("%%zu\\n", offsetof(lrm_pileup_variant, %s));\n' % f for f in fields) +
                   '    printf("%zu %zu\\n", offsetof(lrm_pileup_variant_options, hom_pct), offsetof(lrm_pileup_variant_options, reserved));\n    return 0;\n}\n')
    exe = tmp_path / "variant"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    says = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    dt = capi.PILEUP_VARIANT_DT
    assert says[:3] == [48, 32, 32] == [dt.itemsize, C.sizeof(capi.PileupVariantOptions), C.sizeof(capi.AccalnVcfOptions)]
    assert says[3:16] == [dt.fields[f][1] for f in fields] == [getattr(capi.PileupVariant, f).offset for f in fields]
    assert says[3:16] == [0, 8, 12, 16, 20, 24, 28, 29, 30, 31, 32, 40, 41] and says[16:] == [16, 20]
    assert dt.names == fields and dt.fields["bases"][0].shape == (8,) and dt.fields["pad"][0].shape == (7,)
    for s, name in ((capi.PileupVariant, "lrm_pileup_variant"), (capi.PileupVariantOptions, "lrm_pileup_variant_options"), (capi.AccalnVcfOptions, "lrm_accaln_vcf_options")):
        assert capi.LATER_STRUCTS[s] == name                           # compared with the header by tests/test_aln_diff_cpu.py
    assert (V.SNV, V.DEL, V.INS) == (capi.CALL_SNV, capi.CALL_DEL, capi.CALL_INS)
    assert lib.lrm_abi_version() == 3 and capi.N_KERNELS == 9 and len(capi.STRUCTS) == 25
    for name in ("lrm_pileup_variants_dev", "lrm_pileup_variants_host", "lrm_pileup_variants_format_vcf", "lrm_vcf_header", "lrm_accaln_pileup_vcf"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
    from longreadmapper_amd import mapper, pileup
    assert hasattr(mapper.DeviceMapper, "pileup_variants") and hasattr(pileup.Pileup, "variants") and hasattr(textio, "write_vcf")


def test_flow_refuses_bad_options_before_any_file(tmp_path):
    """lrm_accaln_pileup_vcf: bad options are refused before the index is read or any output file is created"""
    out = {k: str(tmp_path / k) for k in ("sam", "sites", "vcf")}
    p, gp = capi.Params(100, 20, 300), capi.GactParams(0, 0, 0)
    po = capi.AccalnPileupOptions(C.sizeof(capi.AccalnPileupOptions), 0, 0, 0, capi.PileupCallOptions(0, 0, 0, 0), -1, 0, os.fsencode(out["sites"]), None)
    total, valid = C.c_uint64(), C.c_uint64()

    def run(po_, vo_):
        return lib.lrm_accaln_pileup_vcf(b"/nonexistent/genome", b"/nonexistent/reads", os.fsencode(out["sam"]), p, gp, 0, 1, C.byref(total), C.byref(valid), None, 0,
                                         C.byref(po_) if po_ is not None else None, C.byref(vo_) if vo_ is not None else None)

    size = C.sizeof(capi.AccalnVcfOptions)
    for vo, word in ((capi.AccalnVcfOptions(size, 101, os.fsencode(out["vcf"]), None, 0), b"hom_pct"), (capi.AccalnVcfOptions(size, 0, os.fsencode(out["vcf"]), None, 5), b"reserved"),
                     (capi.AccalnVcfOptions(size - 8, 0, os.fsencode(out["vcf"]), None, 0), b"struct_size"), (capi.AccalnVcfOptions(size, 0, None, None, 0), b"vcf_path")):
        assert run(po, vo) < 0 and word in lib.lrm_last_error(), word
    assert run(None, capi.AccalnVcfOptions(size, 0, os.fsencode(out["vcf"]), None, 0)) < 0 and b"lrm_accaln_pileup_options" in lib.lrm_last_error()
    bad_po = capi.AccalnPileupOptions(C.sizeof(capi.AccalnPileupOptions), 9, 0, 0, capi.PileupCallOptions(0, 0, 0, 0), -1, 0, None, None)
    assert run(bad_po, capi.AccalnVcfOptions(size, 0, os.fsencode(out["vcf"]), None, 0)) < 0 and b"insertion columns" in lib.lrm_last_error()
    assert not any(os.path.exists(v) for v in out.values())
    with pytest.raises(AssertionError):
        textio.accaln("g", "r", None, 100, pileup=dict(hom_pct=50))                     # hom_pct belongs to vcf=


# ---------------------------------------------------------------------------------------------------------
# the sanitizer build
# ---------------------------------------------------------------------------------------------------------
def test_sanitized_host_harness(tmp_path):
    """tests/models/pileup_var_harness.cpp, with its own main, built with -fsanitize=address,undefined and run as a child
    process: the records, the words, the text and the table in heap blocks of exactly their size."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "pileup_var_harness"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "longreadmapper_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "models", "pileup_var_harness.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(rows, words, text, pos0, opt, cap):
        ins_cols = 0 if words is None else words.shape[1]
        blob = struct.pack("<IQQQIIII", ins_cols, len(rows), cap, pos0, opt[0], opt[1], opt[2], opt[4]) + as_cols(rows).tobytes()
        blob += (b"" if words is None else np.ascontiguousarray(words, dtype=np.uint32).tobytes()) + bytes(text)
        (tmp_path / "in.bin").write_bytes(blob)
        p = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        raw = (tmp_path / "out.bin").read_bytes()
        return struct.unpack("<Q", raw[:8])[0], np.frombuffer(raw[8:], dtype=capi.PILEUP_VARIANT_DT)

    for c in K.CASES:
        rows, text, words, pos0 = sliced(c)
        want = ref_of(c)
        for cap in sorted({len(want), max(len(want) - 1, 0), 0}):
            total, recs = run(rows, words, text, pos0, c.opt, cap)
            assert total == len(want) and V.as_tuples(recs) == want[:cap], (c.name, cap)
    rows, text, words = K.random_records(600, 8, 9)
    want = V.variants(R.cols_array(rows), words, text, 5, V.options())
    total, recs = run(rows, words, text, 5, K.DEF, len(want))
    assert total == len(want) > 100 and V.as_tuples(recs) == want


# ---------------------------------------------------------------------------------------------------------
# the end-to-end inputs on the oracle
# ---------------------------------------------------------------------------------------------------------
def planted_conditions(w, recs, lo):
    """The conditions on a variant table (tuples of V.FIELDS) of the planted workload whose text starts at text position lo
    -> dict(kinds, missing_snv, far_not_1, n_far, del_sums_ok, hom_snv)"""
    kinds = [r[6] for r in recs]
    snv = {r[0] - lo: r for r in recs if r[6] == V.SNV}
    runs = [(r[0] - lo, r[1]) for r in recs if r[6] == V.DEL]
    missing = [(p, chr(b)) for p, b in w["snv"] if p not in snv or snv[p][8] != b]
    far = [(q, ln) for q, ln in runs if all(abs(q - p) > 10 for p, _ in w["dels"])]
    sums = [sum(ln for q, ln in runs if q < p + pl + 10 and q + ln > p - 10) for p, pl in w["dels"]]
    return dict(kinds=(len(recs), kinds.count(V.DEL), kinds.count(V.SNV), kinds.count(V.INS)), missing_snv=missing,
                far_not_1=[r for r in far if r[1] != 1], n_far=len(far),
                del_sums_ok=sum(1 for s, (_, pl) in zip(sums, w["dels"]) if s == pl),
                hom_snv=sum(1 for p, _ in w["snv"] if p in snv and snv[p][9] == 2))


PLANTED_KINDS = (104, 46, 41, 17)
PLANTED_HOM_SNV = 38


def test_planted_variants_on_the_oracle():
    """The end-to-end inputs of tests/test_gpu_pileup_variants.py, proved where no GPU is needed: the oracle maps the reads of
    the copy against the original text (classic mode), their op bytes go through the host rules with K = 8 and the default
    options, and the variant table of the whole text holds what was planted.  The classic aligner splits a planted deletion
    by a matching column in some cases (DD=DDD): one planted deletion may be two or three adjacent records -- the aligner's
    doing, not the merge's -- so the deleted lengths are summed around every planted deletion.  A condition on the input."""
    w = KC.planted()
    hi = index.HostIndex.build([w["text"]], hlen=10)
    oi = orc.OracleIndex.from_host_index(hi)
    best, _ = oi.seed_batch(w["reads"], w["lens"], nthreads=8)
    reads = w["reads"].copy()
    ext = oi.extend_batch(reads, w["lens"], best, nthreads=8)
    lo, hi_ = index.text_window(hi, 0)
    W_ = hi_ - lo
    ins_cols = 8
    planes, ins = np.zeros(8 * W_ + 1, dtype=np.uint32), np.zeros(4 * ins_cols * W_, dtype=np.uint32)
    for i in range(len(reads)):
        n = int(ext["n_ops"][i])
        if n > 0 and ext["meta_r"][i] != 0 and ext["score"][i] != -1:
            args = (ext["ops"][i].ctypes.data, n, reads[i].ctypes.data, int(w["lens"][i]), int(ext["meta"]["loc"][i]), lo, hi_)
            lib.lrm_pileup_add_host(*args, planes.ctypes.data)
            lib.lrm_pileup_ins_add_host(*args, ins_cols, ins.ctypes.data)
    cols = np.zeros(W_, dtype=capi.PILEUP_COL_DT)
    capi.check(lib.lrm_pileup_cols_host(planes.ctypes.data, lo, hi_, 0, W_, cols.ctypes.data), "lrm_pileup_cols_host")
    words = np.ascontiguousarray(ins.reshape(ins_cols, 4, W_).transpose(2, 0, 1))
    content = bytes(hi.content()[lo:hi_])
    got, total, _ = host_variants(cols, words, content, lo, cap=4096)
    recs = V.as_tuples(got)
    # the reference's reading of the same records: only the positions with any count go through it (sites_sparse's argument)
    live = np.flatnonzero(cols["n_del"].astype(bool) | cols["n_ins"].astype(bool) | (cols["n_eq"] != cols["depth"]))
    blocks, want = np.split(live, np.flatnonzero(np.diff(live) > 1) + 1), []
    for b in blocks:                                                   # maximal stretches: a run never crosses a clean position
        a, e = int(b[0]), int(b[-1]) + 1
        want += V.variants(cols[a:e], words[a:e], content[a:e], lo + a, V.options())
    assert total == len(recs) and recs == want
    c = planted_conditions(w, recs, lo)
    print("planted:", {k: v for k, v in c.items() if k != "missing_snv"})
    assert c["kinds"] == PLANTED_KINDS
    assert not c["missing_snv"], c["missing_snv"]
    assert not c["far_not_1"] and c["n_far"] == 28
    assert c["del_sums_ok"] >= 9
    assert c["hom_snv"] == PLANTED_HOM_SNV
    # the sites table of the same records: 63 deleted positions merge into the 46 runs
    sites = np.zeros(256, dtype=capi.PILEUP_SITE_DT)
    n_sites = lib.lrm_pileup_sites_host(cols.ctypes.data, content, lo, W_, None, sites.ctypes.data, 256, None)
    k = sites["kinds"][:n_sites]
    assert n_sites == 120 and [int(((k & b) != 0).sum()) for b in (2, 1, 4)] == [63, 41, 17]
    assert sum(r[1] for r in recs if r[6] == V.DEL) == 63
    # the VCF text: POS does not decrease
    pos1 = [int(line.split("\t")[1]) for line in textio.vcf_text(hi, got).decode().splitlines()]
    assert len(pos1) == 104 and all(a <= b for a, b in zip(pos1, pos1[1:]))
    hi.close()
