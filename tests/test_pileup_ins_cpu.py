"""The insertion columns of the pileup on the host (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus"): the
constructed rows and records reach their edges; lrm_pileup_ins_add_host, lrm_pileup_ins_allele_host and
lrm_pileup_polish_host -- the kernels' own rules as plain C++ -- equal tests/pileup_ins_ref.py on every case and on random
inputs, for equality; the invariant on column 0; the refusals; the record's layout by a compiled C program; a stand-alone
sanitizer build of the rules, run as a child process; the planted workload of the GPU test proved on the oracle."""
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
import pileup_cases as P
import pileup_ins_cases as K
import pileup_ins_ref as IR
import pileup_ref
from longreadmapper_amd import capi, index, textio
from longreadmapper_amd.capi import lib

FILL = 0xAB
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LO, HI, W = K.LO, K.HI, K.HI - K.LO


def live(c, min_mapq=K.MIN_MAPQ):
    return pileup_ref.aligned(P.effective_ops(c), c.score, c.meta_r) and c.mapq >= min_mapq


def host_ins_add(cases, ins_cols, lo=LO, hi=HI, planes=None):
    """lrm_pileup_ins_add_host over the rows that are aligned and pass the filter -> the planes (4 * K * W words).  Every
    row's op bytes and read bytes sit in arrays of exactly their length."""
    planes = np.zeros(4 * ins_cols * (hi - lo), dtype=np.uint32) if planes is None else planes
    for c in cases:
        if not live(c):
            continue
        ops, read = np.frombuffer(P.effective_ops(c), dtype=np.uint8).copy(), np.frombuffer(c.read, dtype=np.uint8).copy()
        lib.lrm_pileup_ins_add_host(ops.ctypes.data, len(ops), read.ctypes.data if len(read) else None, len(read), c.loc, lo, hi, ins_cols, planes.ctypes.data)
    return planes


def ref_ins(cases, ins_cols, lo=LO, hi=HI):
    ref = IR.InsPileup(lo, hi, ins_cols)
    for c in cases:
        ref.add(P.effective_ops(c), c.read, c.loc, c.score, c.meta_r, c.mapq, K.MIN_MAPQ)
    return ref


def host_allele(depth, n_ins, s, opt=None):
    """lrm_pileup_ins_allele_host on words and a record that lie in fill -> (n_col0, len, flags, bases) or None when refused"""
    s = np.asarray(s, dtype=np.uint32)
    words = np.concatenate([np.full(4, 0xABABABAB, dtype=np.uint32), s.reshape(-1), np.full(4, 0xABABABAB, dtype=np.uint32)])
    out = np.full(48, FILL, dtype=np.uint8)
    o = capi.PileupCallOptions(*opt) if opt is not None else None
    rc = lib.lrm_pileup_ins_allele_host(depth, n_ins, words.ctypes.data + 16, len(s), C.byref(o) if o is not None else None, out.ctypes.data + 16)
    if rc < 0:
        return None
    assert (out[:16] == FILL).all() and (out[32:] == FILL).all()
    return IR.allele_tuple(out[16:32].view(capi.PILEUP_INS_ALLELE_DT)[0])


def as_cols(rows):
    out = np.zeros(len(rows), dtype=capi.PILEUP_COL_DT)
    ref = R.cols_array(rows)
    for f in ref.dtype.names:
        out[f] = ref[f]
    return out


def host_polish(cols, words, content, opt=None, cap=None, pad=16):
    """lrm_pileup_polish_host into a buffer that lies in fill -> (bytes written, total, the bytes outside out[0 .. min(total, cap)))"""
    cols = np.ascontiguousarray(cols, dtype=capi.PILEUP_COL_DT)
    n = len(cols)
    ins_cols = 0 if words is None else words.shape[1]
    flat = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1) if ins_cols else None
    content = np.frombuffer(bytes(content), dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)
    cap = 9 * n + 1 if cap is None else cap
    buf = np.full(cap + 2 * pad, FILL, dtype=np.uint8)
    o = capi.PileupCallOptions(*opt) if opt is not None else None
    total = lib.lrm_pileup_polish_host(cols.ctypes.data if n else None, flat.ctypes.data if ins_cols and n else None, ins_cols, content.ctypes.data, n,
                                       C.byref(o) if o is not None else None, buf.ctypes.data + pad if cap else None, cap)
    if total < 0:
        return None, total, None
    k = min(total, cap)
    return bytes(buf[pad:pad + k]), total, np.concatenate([buf[:pad], buf[pad + k:]])


# ---------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------
def test_cases_reach_their_edges():
    names = [c.name for c in K.ROWS]
    assert len(set(names)) == len(names) >= 70 and max(len(c.ops) for c in K.ROWS) <= K.MAX_ROW and K.ROWS[-1].last
    missed = [c.name for c in K.ROWS if not c.reaches()]
    assert not missed, missed
    assert K.RUN_LENGTHS == [1, 2, 3, 4, 5, 7, 8, 9, 17, 40]
    by = {c.name: c for c in K.ROWS}
    # by the reference's own reading: what is counted nowhere, what stops at K, what the window cuts
    for name in ("row-is-one-I", "run-at-column-0", "run-behind-S-only", "read-only-N", "dead-meta_r-0", "dead-score--1", "dead-n_ops-0", "mapq-below",
                 "run-at-lo-1", "run-at-hi+0", "starts-at-hi"):
        assert not ref_ins([by[name]], 8).c.any(), name
    for name in ("run-at-lo+0", "run-at-hi-1", "mapq-at", "starts-left-of-the-window", "read-lower-case", "run-on-the-last-read-bytes"):
        assert ref_ins([by[name]], 8).c.any(), name
    for ins_cols in K.KS:
        for n in K.RUN_LENGTHS:
            assert ref_ins([by["run-of-%d" % n]], ins_cols).c.sum() == min(n, ins_cols)
        assert ref_ins([by["run-over-lanes-1-to-3"]], ins_cols).c.sum() == ins_cols
    assert ref_ins([by["read-ends-inside-the-run"]], 8).c.sum() == 4              # the read's 24 bytes end behind the run's fourth column
    assert ref_ins([by["starts-left-of-the-window"]], 8).c.sum() == 5             # the run left of lo is not counted
    assert ref_ins([by["run-behind-D"]], 8).c[by["run-behind-D"].loc + 10 - LO].sum() == 3
    missed = [a.name for a in K.ALLELES if not a.reaches()]
    assert not missed, missed
    assert len(K.ALLELES) >= 50 and {len(a.s) for a in K.ALLELES} >= set(K.KS)


@pytest.mark.parametrize("ins_cols", K.KS)
def test_host_add_on_every_row(ins_cols):
    bad = []
    for c in K.ROWS:
        got, want = host_ins_add([c], ins_cols), ref_ins([c], ins_cols).planes()
        if not np.array_equal(got, want):
            bad.append((c.name, int(got.sum()), int(want.sum())))
    assert not bad, (len(bad), bad[:8])
    # all rows into one set of planes, and every row twice: the counts add up
    want = ref_ins(K.ROWS, ins_cols).planes()
    got = host_ins_add(K.ROWS, ins_cols)
    assert np.array_equal(got, want) and want.sum() > 1000
    assert np.array_equal(host_ins_add(K.ROWS, ins_cols, planes=got), 2 * want)


def test_windows_that_cut_the_rows():
    by = {c.name: c for c in K.ROWS}
    c = by["random-3100"]
    for lo, hi in ((c.loc + 100, c.loc + 101), (c.loc - 50, c.loc + 1), (c.loc + 1500, c.loc + 9000), (c.loc + P.span(c.ops) - 1, c.loc + P.span(c.ops) + 5)):
        want = ref_ins([c], 4, lo, hi)
        assert np.array_equal(host_ins_add([c], 4, lo, hi), want.planes()), (lo, hi)
    assert ref_ins([c], 4, c.loc + 1500, c.loc + 9000).c.any()


def test_counters_wrap():
    by = {c.name: c for c in K.ROWS}
    c = by["run-of-4"]
    planes = np.full(4 * 4 * W, 0xFFFFFFFF, dtype=np.uint32)
    host_ins_add([c], 4, planes=planes)
    want = ref_ins([c], 4).planes()
    assert want.sum() == 4 and np.array_equal(planes, (want.astype(np.int64) - 1) & 0xFFFFFFFF)


def test_column_0_sums_to_the_ins_plane():
    """the four words of column 0 at a position, plus the column-0 bytes that are no base, are the existing `ins` plane there"""
    for ins_cols in K.KS:
        ins = host_ins_add(K.ROWS, ins_cols).reshape(ins_cols, 4, W)
        planes = np.zeros(8 * W + 1, dtype=np.uint32)
        ref = ref_ins(K.ROWS, ins_cols)
        for c in K.ROWS:
            if live(c):
                ops, read = np.frombuffer(P.effective_ops(c), dtype=np.uint8).copy(), np.frombuffer(c.read, dtype=np.uint8).copy()
                lib.lrm_pileup_add_host(ops.ctypes.data, len(ops), read.ctypes.data if len(read) else None, len(read), c.loc, LO, HI, planes.ctypes.data)
        n_ins = planes[W + 1 + 6 * W:W + 1 + 7 * W].astype(np.int64)
        assert n_ins.sum() > 300 and ref.col0_other.sum() > 20
        assert np.array_equal(ins[0].astype(np.int64).sum(axis=0) + ref.col0_other, n_ins), ins_cols


# ---------------------------------------------------------------------------------------------------------
# the allele rule
# ---------------------------------------------------------------------------------------------------------
def test_allele_rule_on_every_case():
    bad = []
    for a in K.ALLELES:
        want = IR.allele(a.depth, a.n_ins, a.s, a.opt)
        got = host_allele(a.depth, a.n_ins, a.s, a.opt + (0,))
        if got != want:
            bad.append((a.name, got, want))
    assert not bad, (len(bad), bad[:5])
    got = {a.name: IR.allele(a.depth, a.n_ins, a.s, a.opt) for a in K.ALLELES}
    # the case list holds what the rule's edges ask for, by the reference's own reading of each case
    for ins_cols in K.KS:
        for j in range(ins_cols):
            assert got["K%d-col%d-sup-on" % (ins_cols, j)][1] == j and got["K%d-col%d-sup-above" % (ins_cols, j)][1] == ins_cols
        assert got["K%d-full" % ins_cols][1:3] == (ins_cols, IR.ENTERS | IR.FULL)
    assert [got[n][2] & IR.ENTERS for n in ("enters-on", "enters-above", "depth-below-min", "depth-at-min", "depth-below-min-20", "depth-at-min-20",
                                            "64-bit-enters-on", "64-bit-enters-above", "64-bit-enters-product-past-2^32")] == [0, 1, 0, 1, 0, 1, 0, 1, 1]
    assert {got["tie-%s" % t][3] for t in ("AC", "AG", "AT", "ACGT")} == {b"AAAA"} and got["tie-CG"][3] == b"CCCC" and got["tie-GT"][3] == b"GGGG"
    assert got["tie-T"][3] == b"TTTT" and got["later-letter-larger"][3] == b"TTTT"
    assert got["gap-in-column-2"][1] == 2 and got["column-0-fails"][1] == 0 and got["all-words-zero"][1] == 0 and got["n_ins-zero"][1:3] == (0, 0)
    assert (got["64-bit-sup-on"][1], got["64-bit-sup-above"][1]) == (0, 1) and got["sup-wraps"] == (9, 1, IR.ENTERS | IR.FULL, b"A")
    # options NULL: the defaults
    a = K.ALLELES[0]
    assert host_allele(a.depth, a.n_ins, a.s, None) == IR.allele(a.depth, a.n_ins, a.s, K.DEF)


def test_allele_rule_on_random_words():
    rng = np.random.default_rng(99)
    bad = 0
    for n in range(4000):
        ins_cols = int(rng.integers(1, 9))
        hi = (3, 12, 40, 2**31)[n % 4]
        s = rng.integers(0, hi, (ins_cols, 4)) * (rng.random((ins_cols, 4)) < 0.7)
        depth, n_ins = int(rng.integers(0, min(3 * hi, 2**32))), int(rng.integers(0, 2 * hi))
        opt = ((0, 0, 0), (3, 2, 10), (30, 1, 100))[n % 3]
        bad += host_allele(depth, n_ins, s, opt + (0,)) != IR.allele(depth, n_ins, s, R.options(*opt))
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------
# the polished sequence
# ---------------------------------------------------------------------------------------------------------
def test_polish_on_the_constructed_positions():
    cols, text, words = K.polish_positions()
    want = IR.polish(R.cols_array(cols), words, text, K.DEF)
    assert want == b"AAA" + b"T" + b"G" * 8 + b"G" * 8 + b"N" + b"N" + b"G" + b"A" + b"AC" + b"N" + b"T"
    for ins_cols in (8, 4, 1):
        w = np.ascontiguousarray(words[:, :ins_cols])
        want_k = IR.polish(R.cols_array(cols), w, text, K.DEF)
        got, total, outside = host_polish(as_cols(cols), w, text)
        assert (got, total) == (want_k, len(want_k)) and (outside == FILL).all(), ins_cols
    plain = IR.polish(R.cols_array(cols), None, text, K.DEF)
    assert plain == b"AAATNNGANT" and host_polish(as_cols(cols), None, text)[:2] == (plain, len(plain))
    # cap below, at and above the total: nothing from cap on, nothing outside
    for cap in (0, 1, 3, 4, 5, 11, 12, 13, len(want) - 1, len(want), len(want) + 1, len(want) + 50):
        got, total, outside = host_polish(as_cols(cols), words, text, cap=cap)
        assert total == len(want) and got == want[:cap] and (outside == FILL).all(), cap
    # other options: min_depth 2 lets the shallow positions speak
    opt = (2, 0, 0, 0)
    want2 = IR.polish(R.cols_array(cols), words, text, R.options(*opt))
    assert want2 != want and host_polish(as_cols(cols), words, text, opt)[:2] == (want2, len(want2))
    assert host_polish(as_cols([]), words[:0], b"")[:2] == (b"", 0)


def test_polish_on_random_records():
    rng = np.random.default_rng(5)
    n = 3000
    rows = []
    for k in range(n):
        hi = (3, 12, 40)[k % 3]
        x = rng.integers(0, hi, 4) * (rng.random(4) < 0.5)
        n_eq, n_del = int(rng.integers(0, 2 * hi)), int(rng.integers(0, 2 * hi) * (rng.random() < 0.3))
        rows.append((n_eq + int(x.sum()) + n_del, n_eq, *(int(v) for v in x), n_del, int(rng.integers(0, 2 * hi) * (rng.random() < 0.5))))
    content = bytes(rng.choice(np.frombuffer(b"ACGTACGTacgtNn", dtype=np.uint8), size=n))
    for ins_cols in K.KS:
        words = (rng.integers(0, 30, (n, ins_cols, 4)) * (rng.random((n, ins_cols, 4)) < 0.6)).astype(np.uint32)
        for opt in ((0, 0, 0, 0), (3, 2, 10, 0)):
            want = IR.polish(R.cols_array(rows), words, content, R.options(*opt))
            got, total, outside = host_polish(as_cols(rows), words, content, opt)
            assert n // 2 < len(want) and (got, total) == (want, len(want)) and (outside == FILL).all(), (ins_cols, opt)
            assert len(want) > len(IR.polish(R.cols_array(rows), None, content, R.options(*opt)))


# ---------------------------------------------------------------------------------------------------------
# refusals, the record, the binding
# ---------------------------------------------------------------------------------------------------------
def test_refusals():
    cols, text, words = K.polish_positions()
    for o in K.REFUSED:
        assert host_polish(as_cols(cols), words, text, o)[1] < 0 and (b"min_pct" in lib.lrm_last_error() or b"reserved" in lib.lrm_last_error()), o
        assert host_allele(20, 12, words[4], o) is None
    one = np.zeros(4 * 9, dtype=np.uint32)
    out = np.zeros(16, dtype=np.uint8)
    assert lib.lrm_pileup_ins_allele_host(20, 12, one.ctypes.data, 9, None, out.ctypes.data) < 0 and b"insertion columns" in lib.lrm_last_error()
    assert lib.lrm_pileup_ins_allele_host(20, 12, one.ctypes.data, 0, None, out.ctypes.data) < 0
    assert lib.lrm_pileup_ins_allele_host(20, 12, None, 4, None, out.ctypes.data) < 0 and b"null argument" in lib.lrm_last_error()
    assert lib.lrm_pileup_ins_allele_host(20, 12, one.ctypes.data, 4, None, None) < 0
    c = as_cols(cols)
    assert lib.lrm_pileup_polish_host(c.ctypes.data, None, 4, text, len(c), None, out.ctypes.data, 16) < 0 and b"null argument" in lib.lrm_last_error()
    assert lib.lrm_pileup_polish_host(c.ctypes.data, one.ctypes.data, 9, text, 1, None, out.ctypes.data, 16) < 0 and b"insertion columns" in lib.lrm_last_error()
    assert lib.lrm_pileup_polish_host(c.ctypes.data, None, 0, text, len(c), None, None, 5) < 0
    assert lib.lrm_pileup_polish_host(None, None, 0, None, 0, None, None, 0) == 0
    # the host add takes no bad argument and counts nothing then
    planes = np.zeros(4 * 9 * 10, dtype=np.uint32)
    ops, read = np.frombuffer(b"==II==", dtype=np.uint8).copy(), np.frombuffer(b"ACGTAC", dtype=np.uint8).copy()
    for args in ((ops.ctypes.data, 6, read.ctypes.data, 6, 100, 100, 110, 0), (ops.ctypes.data, 6, read.ctypes.data, 6, 100, 100, 110, 9),
                 (ops.ctypes.data, 0, read.ctypes.data, 6, 100, 100, 110, 4), (ops.ctypes.data, 6, read.ctypes.data, 6, 100, 110, 110, 4),
                 (None, 6, read.ctypes.data, 6, 100, 100, 110, 4)):
        lib.lrm_pileup_ins_add_host(*args, planes.ctypes.data)
        assert not planes.any(), args[-1]
    lib.lrm_pileup_ins_add_host(ops.ctypes.data, 6, None, 6, 100, 100, 110, 4, planes.ctypes.data)       # no read: every byte is behind its end
    assert not planes.any()
    lib.lrm_pileup_ins_add_host(ops.ctypes.data, 6, read.ctypes.data, 6, 100, 100, 110, 4, planes.ctypes.data)
    assert planes.sum() == 2 and planes[(4 * 0 + 2) * 10 + 1] == 1 and planes[(4 * 1 + 3) * 10 + 1] == 1     # G in column 0, T in column 1, behind position 101


def test_record_layout_and_binding(tmp_path):
    """the 16-byte record by the host C compiler: a small program of its own prints sizeof and offsetof"""
    src = tmp_path / "allele.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lrm_accel.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %d %u %u\\n", sizeof(lrm_pileup_ins_allele), offsetof(lrm_pileup_ins_allele, n_col0),\n'
                   '           offsetof(lrm_pileup_ins_allele, len), offsetof(lrm_pileup_ins_allele, flags), offsetof(lrm_pileup_ins_allele, pad),\n'
                   '           offsetof(lrm_pileup_ins_allele, bases), LRM_PILEUP_INS_COLS_MAX, LRM_INS_ENTERS, LRM_INS_FULL);\n    return 0;\n}\n')
    exe = tmp_path / "allele"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    says = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    dt = capi.PILEUP_INS_ALLELE_DT
    assert says == [dt.itemsize] + [dt.fields[f][1] for f in ("n_col0", "len", "flags", "pad", "bases")] + [capi.PILEUP_INS_COLS_MAX, capi.INS_ENTERS, capi.INS_FULL]
    assert says == [16, 0, 4, 5, 6, 8, 8, 1, 2] and dt.names == ("n_col0", "len", "flags", "pad", "bases") and dt.fields["bases"][0].shape == (8,)
    assert (IR.ENTERS, IR.FULL) == (capi.INS_ENTERS, capi.INS_FULL)
    assert [capi.CONSTANTS[k] for k in ("LRM_PILEUP_INS_COLS_MAX", "LRM_INS_ENTERS", "LRM_INS_FULL")] == [8, 1, 2]
    assert lib.lrm_abi_version() == 3 and capi.N_KERNELS == 9 and len(capi.STRUCTS) == 25
    for name in ("lrm_pileup_create_ins", "lrm_pileup_ins_cols", "lrm_pileup_ins_read_dev", "lrm_pileup_polish_dev", "lrm_pileup_site_alleles_dev",
                 "lrm_pileup_ins_add_host", "lrm_pileup_polish_host", "lrm_pileup_ins_allele_host", "lrm_debug_pileup_ins_raw"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
    assert lib.lrm_pileup_ins_cols(None) == 0
    from longreadmapper_amd import mapper
    assert all(hasattr(mapper.DeviceMapper, f) for f in ("pileup_ins_columns", "pileup_polish", "pileup_site_alleles"))


def test_write_sites_with_alleles(tmp_path):
    from longreadmapper_amd import synth
    hi = index.HostIndex.build([synth.reference(300, seed=5)], names=["chr1"], hlen=3)
    off = hi.mta()[0][1]
    sites = np.zeros(3, dtype=capi.PILEUP_SITE_DT)
    for k in range(3):
        sites[k] = (off + 5 * k, 20, 8, 0, 0, 12, ord("A"), ord("."), ord("A"), 4)
    alleles = np.zeros(3, dtype=capi.PILEUP_INS_ALLELE_DT)
    alleles["len"] = [2, 0, 8]
    alleles["bases"][0, :2] = list(b"GT")
    alleles["bases"][2] = list(b"ACGTACGT")
    assert textio.write_sites(str(tmp_path / "plain.tsv"), hi, sites) == 3
    assert textio.write_sites(str(tmp_path / "with.tsv"), hi, sites, alleles=alleles, chunk=2) == 3
    plain, with_ = open(tmp_path / "plain.tsv").read().splitlines(), open(tmp_path / "with.tsv").read().splitlines()
    assert plain == textio.sites_text(hi, sites).decode().splitlines()            # the default output is what it was
    assert with_ == [p + "\t" + a for p, a in zip(plain, ("GT", ".", "ACGTACGT"))]
    hi.close()


# ---------------------------------------------------------------------------------------------------------
# the sanitizer build
# ---------------------------------------------------------------------------------------------------------
def test_sanitized_host_harness(tmp_path):
    """tests/models/pileup_ins_harness.cpp, with its own main, built with -fsanitize=address,undefined and run as a child
    process: every row's op bytes and read bytes, the records, the words, the text and the output in heap blocks of exactly
    their size."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "pileup_ins_harness"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "longreadmapper_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "models", "pileup_ins_harness.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(blob):
        (tmp_path / "in.bin").write_bytes(blob)
        p = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        return (tmp_path / "out.bin").read_bytes()

    rows = [c for c in K.ROWS if live(c)]
    for ins_cols in K.KS:
        blob = struct.pack("<IIQQQ", 0, ins_cols, LO, HI, len(rows))
        for c in rows:
            ops = P.effective_ops(c)
            blob += struct.pack("<QII", c.loc, len(ops), len(c.read)) + ops + c.read
        assert np.array_equal(np.frombuffer(run(blob), dtype=np.uint32), ref_ins(K.ROWS, ins_cols).planes()), ins_cols
    cols, text, words = K.polish_positions()
    want = IR.polish(R.cols_array(cols), words, text, K.DEF)
    for cap in (len(want), len(want) - 1, 5, 0):
        raw = run(struct.pack("<IIQQIII", 1, 8, len(cols), cap, 0, 0, 0) + as_cols(cols).tobytes() + words.tobytes() + text)
        kept = min(cap, len(want))
        assert struct.unpack("<Q", raw[:8])[0] == len(want) and raw[8:8 + kept] == want[:cap] and len(raw) == 8 + kept + 16 * len(cols), cap
        recs = np.frombuffer(raw[8 + kept:], dtype=capi.PILEUP_INS_ALLELE_DT)
        assert [IR.allele_tuple(r) for r in recs] == [IR.allele(c[0], c[7], w, K.DEF) for c, w in zip(cols, words)]
    raw = run(struct.pack("<IIQQIII", 1, 0, len(cols), 64, 0, 0, 0) + as_cols(cols).tobytes() + text)
    assert raw[8:] == IR.polish(R.cols_array(cols), None, text, K.DEF)


# ---------------------------------------------------------------------------------------------------------
# the end-to-end inputs on the oracle
# ---------------------------------------------------------------------------------------------------------
def shift(w, x):
    """text position x of the original, away from every planted variant, lies at x + shift in the copy"""
    return sum(ln for p, ln in w["ins"] if p < x) - sum(ln for p, ln in w["dels"] if p + ln <= x)


def copy_slice(w, a, b):
    """the copy's bytes that text positions [a, b) of the original turn into (a and b away from every planted variant)"""
    return bytes(w["copy"][a + shift(w, a):b + shift(w, b)])


def test_planted_insertions_on_the_oracle():
    """The end-to-end inputs of tests/test_gpu_pileup_ins.py, proved where no GPU is needed: the oracle maps the reads of the
    copy against the original text (classic mode), their op bytes go through the host rules with K = 8 and the default
    options, and the polished text positions [6000, 194000) are the copy's own bytes.  A condition on the input."""
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
    # the invariant on column 0: the reads hold bases only
    assert np.array_equal(words[:, 0, :].astype(np.int64).sum(axis=1), cols["n_ins"].astype(np.int64))
    content = bytes(hi.content()[lo:hi_])
    a, b = 6000, 194000
    got, total, _ = host_polish(cols[a:b], words[a:b], content[a:b])
    want = copy_slice(w, a, b)
    plain, _, _ = host_polish(cols[a:b], None, content[a:b])
    print("polished [%d, %d): %d bytes, the copy's slice %d; without insertion bases %d" % (a, b, total, len(want), len(plain)))
    assert total == len(got) == len(want) == 187_995 and got == want
    assert len(plain) == len(want) - sum(ln for _, ln in w["ins"]) == len(want) - 29        # every planted insertion lies inside the slice
    assert got == IR.polish(cols[a:b], words[a:b], content[a:b], R.options())
    hi.close()
