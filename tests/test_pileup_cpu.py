"""The pileup on the host (docs/GACT_SPEC.md, "Pileup"): the constructed cases reach their edges; lrm_pileup_add_host +
lrm_pileup_cols_host -- the kernel's own word step as plain C++ -- equal tests/pileup_ref.py on every case; the text writer;
the record and the ABI; a stand-alone sanitizer build of the word step and the host walk, run as a child process."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pileup_cases as K
import pileup_ref
from longreadmapper_amd import capi, index, synth, textio
from longreadmapper_amd.capi import lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LO, HI, W = K.LO, K.HI, K.HI - K.LO


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(1, dtype=np.uint8)


def host_add(planes, c, lo=LO, hi=HI):
    """One case through lrm_pileup_add_host, the aligned test and the filter applied by the caller as the rule says."""
    ops = K.effective_ops(c)
    if not pileup_ref.aligned(ops, c.score, c.meta_r) or c.mapq < K.MIN_MAPQ:
        return
    o, r = _u8(ops).copy(), _u8(c.read).copy()
    lib.lrm_pileup_add_host(o.ctypes.data, len(ops), r.ctypes.data if len(c.read) else None, len(c.read), c.loc, lo, hi, planes.ctypes.data)


def host_cols(planes, first=0, count=None, lo=LO, hi=HI):
    count = hi - lo - first if count is None else count
    out = np.zeros(max(count, 1), dtype=capi.PILEUP_COL_DT)
    capi.check(lib.lrm_pileup_cols_host(planes.ctypes.data, lo, hi, first, count, out.ctypes.data), "lrm_pileup_cols_host")
    return out[:count]


def ref_add(ref, c):
    ref.add(K.effective_ops(c), c.read, c.loc, c.score, c.meta_r, c.mapq, K.MIN_MAPQ)


def test_cases_reach_their_edges():
    names = [c.name for c in K.CASES]
    assert len(set(names)) == len(names) > 200
    missed = [c.name for c in K.CASES if not c.reaches()]
    assert not missed, missed
    assert {len(c.ops) for c in K.CASES} >= set(K.N_OPS)
    assert {c.loc % 16 for c in K.CASES} == set(range(16))
    assert K.CASES[-1].last and sum(c.last for c in K.CASES) == 1
    # the window's edges are hit from both sides: events at lo - 1, lo, hi - 1, hi; alignments over either edge and over both
    spans = [(c.loc, c.loc + K.span(K.effective_ops(c))) for c in K.CASES]
    assert any(b == LO for a, b in spans) and any(a == HI for a, b in spans)
    assert any(a < LO < b < HI for a, b in spans) and any(LO < a < HI < b for a, b in spans) and any(a < LO and HI < b for a, b in spans)
    assert {c.mapq for c in K.CASES} >= {K.MIN_MAPQ - 1, K.MIN_MAPQ}
    assert any(c.meta_r == 0 for c in K.CASES) and any(c.score == -1 for c in K.CASES) and any(c.n_ops is not None and c.n_ops <= 0 for c in K.CASES)


def test_host_rule_on_every_case():
    bad = []
    total = pileup_ref.Pileup(LO, HI)
    planes_all = np.zeros(8 * W + 1, dtype=np.uint32)
    for c in K.CASES:
        ref = pileup_ref.Pileup(LO, HI)
        ref_add(ref, c)
        ref_add(total, c)
        planes = np.zeros(8 * W + 1, dtype=np.uint32)
        host_add(planes, c)
        host_add(planes_all, c)
        want = ref.columns()
        if not pileup_ref.same(host_cols(planes), want):
            bad.append((c.name, pileup_ref.first_difference(host_cols(planes), want)))
        other = planes[W + 1 + 4 * W:W + 1 + 5 * W].astype(np.int64)
        if not np.array_equal(other, ref.other()):
            bad.append((c.name, "x_other"))
    assert not bad, (len(bad), bad[:5])
    want = total.columns()
    got = host_cols(planes_all)
    assert pileup_ref.same(got, want), pileup_ref.first_difference(got, want)
    # the cases leave something to see: every counter somewhere, inside the window and at both of its ends
    for f in pileup_ref.COL_FIELDS:
        assert want[f].any(), f
    assert total.other().any() and want["depth"][0] > 0 and want["depth"][-1] > 0
    # sub-ranges, and the derived `other`
    for first, count in ((0, 1), (1, 17), (W - 1, 1), (2047, 3), (W // 2, 0), (333, 4096)):
        assert pileup_ref.same(host_cols(planes_all, first, count), total.columns(first, count)), (first, count)
    derived = got["depth"].astype(np.int64) - got["n_eq"] - got["x_a"] - got["x_c"] - got["x_g"] - got["x_t"] - got["n_del"]
    assert np.array_equal(derived, total.other())
    assert lib.lrm_pileup_cols_host(planes_all.ctypes.data, LO, HI, W, 1, None) < 0 and b"outside a window" in lib.lrm_last_error()
    assert lib.lrm_pileup_cols_host(planes_all.ctypes.data, HI, LO, 0, 0, None) < 0


def test_counters_wrap():
    """32-bit wrapping counters: planes that start near the top come round."""
    planes = np.zeros(8 * 4 + 1, dtype=np.uint32)
    planes[0] = 0xFFFFFFFF                                             # a depth of 2^32 - 1 at the first position
    planes[4 + 1 + 5 * 4] = 0xFFFFFFFF                                 # ... and as many 'D' columns
    o, r = _u8(b"=D"), _u8(b"A")
    lib.lrm_pileup_add_host(o.ctypes.data, 2, r.ctypes.data, 1, 99, 100, 104, planes.ctypes.data)     # covers 99, 100: 'D' on 100
    got = host_cols(planes, lo=100, hi=104)
    assert got["depth"].tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF] and got["n_del"][0] == 0 and got["n_eq"][0] == 0


def _format(mta, seq, seq_pos, content, cols, room=None):
    cols = np.ascontiguousarray(cols)
    room = 200 * (len(cols) + 1) if room is None else room
    buf = C.create_string_buffer(room)
    c = np.ascontiguousarray(content)
    k = lib.lrm_pileup_format(mta, len(mta), seq, seq_pos, len(cols), c.ctypes.data, cols.ctypes.data, buf, room)
    return k, buf.raw[:max(k, 0)].decode()


def test_format_lines(tmp_path):
    seqs = [synth.reference(300, seed=5), synth.reference(200, seed=6)]
    hi = index.HostIndex.build(seqs, names=["chr1 primary", "chr2"], hlen=3)
    content = hi.content().copy()
    entries = hi.mta()
    mta = textio.mta_table(entries)
    rng = np.random.default_rng(8)
    for s, (name, offset, seq_len) in enumerate(entries):
        cols = np.zeros(seq_len, dtype=capi.PILEUP_COL_DT)
        for f in ("x_a", "x_c", "x_g", "x_t", "n_del", "n_ins"):
            cols[f] = rng.integers(0, 50, seq_len)
        other = rng.integers(0, 5, seq_len)
        cols["n_eq"] = rng.integers(0, 4_000_000_000, seq_len)
        cols["depth"] = (cols["n_eq"].astype(np.int64) + cols["x_a"] + cols["x_c"] + cols["x_g"] + cols["x_t"] + cols["n_del"] + other) & 0xFFFFFFFF
        for p0, cnt in ((0, seq_len), (7, 20), (seq_len - 1, 1), (seq_len, 0)):
            want = "".join("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
                name, p + 1, chr(content[offset + p]), cols["depth"][p], cols["n_eq"][p], cols["x_a"][p], cols["x_c"][p], cols["x_g"][p],
                cols["x_t"][p], other[p], cols["n_del"][p], cols["n_ins"][p]) for p in range(p0, p0 + cnt))
            k, text = _format(mta, s, p0, content, cols[p0:p0 + cnt])
            assert k == len(want) and text == want, (s, p0, cnt)
        k, _ = _format(mta, s, 0, content, cols, room=100)
        assert k < 0 and b"too small" in lib.lrm_last_error()
        assert _format(mta, s, seq_len - 3, content, cols[:4])[0] < 0 and b"outside a sequence" in lib.lrm_last_error()
    assert _format(mta, 2, 0, content, cols[:1])[0] < 0
    # the helpers of the Python layer: the window of a sequence, the file writer
    assert [index.text_window(hi, s) for s in range(2)] == [(o, o + n) for _, o, n in entries]
    lo, hi_ = index.text_window(hi, 1)
    window = np.zeros(hi_ - 3 - lo, dtype=capi.PILEUP_COL_DT)              # a window that ends three bases short of the sequence
    window["depth"] = np.arange(len(window))
    path = tmp_path / "out.pileup"
    assert textio.write_pileup(str(path), hi, window, lo) == len(window)
    lines = open(path).read().splitlines()
    assert len(lines) == len(window) and lines[5].split("\t")[:4] == ["chr2", "6", chr(content[lo + 5]), "5"]
    both = np.zeros(hi_, dtype=capi.PILEUP_COL_DT)                          # a window over both sequences and the filler between them
    assert textio.write_pileup(str(path), hi, both, 0) == sum(n for _, _, n in entries)
    assert [l.split("\t")[0] for l in open(path).read().splitlines()].count("chr1 primary") == 300
    hi.close()


def test_record_and_abi():
    assert lib.lrm_abi_version() == 3 and capi.N_KERNELS == 9
    assert C.sizeof(capi.MapOptions) == 76 and C.sizeof(capi.BatchExtras) == 24
    assert C.sizeof(capi.PileupCol) == 32 == capi.PILEUP_COL_DT.itemsize
    assert [getattr(capi.PileupCol, f).offset for f in pileup_ref.COL_FIELDS] == list(range(0, 32, 4))
    assert capi.LATER_STRUCTS[capi.PileupCol] == "lrm_pileup_col" and capi.CONSTANTS["LRM_PILEUP_TILE"] == capi.PILEUP_TILE
    assert capi.PILEUP_TILE % 256 == 0
    for name in ("lrm_pileup_create", "lrm_pileup_free", "lrm_pileup_bytes", "lrm_pileup_reset", "lrm_pileup_add_dev", "lrm_pileup_read_dev",
                 "lrm_pileup_add_host", "lrm_pileup_cols_host", "lrm_pileup_format"):
        assert name in capi.SYMBOLS and hasattr(lib, name)


def test_sanitized_host_harness(tmp_path):
    """tests/models/pileup_host_harness.cpp, with its own main, built with -fsanitize=address,undefined and run as a child
    process over every aligned case: rows in heap blocks of exactly their size."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "pileup_host_harness"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "longreadmapper_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "models", "pileup_host_harness.cpp"), "-o", str(exe)])
    ref = pileup_ref.Pileup(LO, HI)
    rows = []
    for c in K.CASES:
        ops = K.effective_ops(c)
        if pileup_ref.aligned(ops, c.score, c.meta_r):
            ref.add(ops, c.read, c.loc)
            rows.append(struct.pack("<QII", c.loc, len(ops), len(c.read)) + ops + c.read)
    # a read shorter than its ops ask for: the bytes behind its end read as zeros, never from memory
    short = (b"=" * 20 + b"X" * 20, b"ACGT" * 6, LO + 64)
    ref.add(*short)
    rows.append(struct.pack("<QII", short[2], len(short[0]), len(short[1])) + short[0] + short[1])
    (tmp_path / "rows.bin").write_bytes(struct.pack("<QQI", LO, HI, len(rows)) + b"".join(rows))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe), str(tmp_path / "rows.bin"), str(tmp_path / "cols.bin")], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.startswith("%d rows, %d positions" % (len(rows), W))
    got = np.fromfile(tmp_path / "cols.bin", dtype=capi.PILEUP_COL_DT)
    want = ref.columns()
    assert pileup_ref.same(got, want), pileup_ref.first_difference(got, want)
