"""The call rule of the pileup on the host (docs/GACT_SPEC.md, "Pileup calls"): the constructed positions reach their edges;
lrm_pileup_sites_host -- the kernels' own rule as plain C++ -- equals tests/pileup_call_ref.py on every case and on random
records, for every cap; the text writer; the records and the ABI; the planted-variant workload of the GPU tests proved on
the oracle; a stand-alone sanitizer build of the rule and the host walk, run as a child process."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import orc
import pileup_call_cases as K
import pileup_call_ref as R
from longreadmapper_amd import capi, index, synth, textio
from longreadmapper_amd.capi import lib

FILL = 0xAB
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def host_sites(cols, content, pos0, opt=None, cap=None, cons=True, pad=4):
    """lrm_pileup_sites_host on a table and a cons buffer that lie in fill -> (site tuples written, total, cons bytes, the
    bytes of the table from cap on and of both paddings, the same of the cons buffer)"""
    cols = np.ascontiguousarray(cols, dtype=capi.PILEUP_COL_DT)
    content = np.frombuffer(bytes(content), dtype=np.uint8).copy() if len(content) else np.zeros(1, dtype=np.uint8)
    n = len(cols)
    cap = n if cap is None else cap
    table = np.full((cap + 2 * pad) * 32, FILL, dtype=np.uint8)
    cbuf = np.full(n + 32, FILL, dtype=np.uint8)
    o = capi.PileupCallOptions(*opt) if opt is not None else None
    total = lib.lrm_pileup_sites_host(cols.ctypes.data if n else None, content.ctypes.data, pos0, n, C.byref(o) if o is not None else None,
                                      table.ctypes.data + 32 * pad if cap else None, cap, cbuf.ctypes.data + 16 if cons else None)
    if total < 0:
        return None, total, None, None, None
    k = min(total, cap)
    written = R.as_tuples(table[32 * pad:32 * (pad + k)].view(capi.PILEUP_SITE_DT))
    outside = np.concatenate([table[:32 * pad], table[32 * (pad + k):]])
    return written, total, bytes(cbuf[16:16 + n]), outside, np.concatenate([cbuf[:16], cbuf[16 + n:]])


def as_cols(rows):
    out = np.zeros(len(rows), dtype=capi.PILEUP_COL_DT)
    ref = R.cols_array(rows)
    for f in ref.dtype.names:
        out[f] = ref[f]
    return out


def opt_tuple(opt):
    return (opt.get("min_depth", 0), opt.get("min_count", 0), opt.get("min_pct", 0), 0)


def test_cases_reach_their_edges():
    names = [c.name for c in K.CASES]
    assert len(set(names)) == len(names) >= 80
    missed = [c.name for c in K.CASES if not c.reaches()]
    assert not missed, missed
    # the case list holds what the rule's edges ask for, by the reference's own reading of each case
    got = {c.name: R.call(c.col, c.byte, R.options(*opt_tuple(c.opt))) for c in K.CASES}
    for kind, bit in (("snv", R.SNV), ("del", R.DEL), ("ins", R.INS)):
        for below, at in (("depth-7", "depth-8"), ("count-3", "count-4"), ("pct-depth-9-count-2", "pct-depth-8-count-2")):
            assert got["%s-%s" % (kind, below)][0] == 0 and got["%s-%s" % (kind, at)][0] == bit, (kind, below, at)
    assert {chr(got[n][1]) for n in names if n.startswith("alt-tie-")} == set("ACG") and chr(got["alt-none-all-equal"][1]) == "."
    assert [chr(got[n][3]) for n in ("cons-tie-ref-A-vs-C", "cons-tie-ref-T-vs-A", "cons-tie-base-vs-base", "cons-tie-base-vs-deletion",
                                     "cons-tie-ref-vs-deletion", "cons-deletion-wins", "cons-all-five-zero", "cons-below-min-depth")] == list("ATCTC-NN")
    assert {got[n][0] for n in names if n.startswith("kinds-")} == {1, 2, 3, 4, 5, 6, 7}
    assert {chr(c.byte) for c in K.CASES} >= set("ACGTacgtNn")
    assert sum(K.plantable(c) for c in K.CASES) >= 50
    assert all(R.options(*o) is None for o in K.REFUSED)


def test_host_rule_on_every_case():
    bad = []
    for c in K.CASES:
        opt = opt_tuple(c.opt)
        want, want_cons = R.sites(R.cols_array([c.col]), bytes([c.byte]), 777, R.options(*opt))
        got, total, cons, _, _ = host_sites(as_cols([c.col]), bytes([c.byte]), 777, opt)
        if (got, total, cons) != (want, len(want), want_cons):
            bad.append((c.name, got, want, cons, want_cons))
    assert not bad, (len(bad), bad[:5])
    # all cases that take the default options as one run of positions, with and without an options struct
    dflt = [c for c in K.CASES if not c.opt]
    cols, content = as_cols([c.col for c in dflt]), bytes(c.byte for c in dflt)
    want, want_cons = R.sites(cols, content, 1 << 33, R.options())
    assert 20 < len(want) < len(dflt)
    for opt in (None, (0, 0, 0, 0), (8, 4, 25, 0)):
        got, total, cons, _, _ = host_sites(cols, content, 1 << 33, opt)
        assert (got, total, cons) == (want, len(want), want_cons), opt


def test_refused_options_and_null_arguments():
    cols = as_cols([K.CASES[0].col])
    for o in K.REFUSED:
        _, total, _, _, _ = host_sites(cols, b"A", 0, o)
        assert total < 0 and (b"min_pct" in lib.lrm_last_error() or b"reserved" in lib.lrm_last_error()), o
    assert lib.lrm_pileup_sites_host(None, None, 0, 1, None, None, 0, None) < 0 and b"null argument" in lib.lrm_last_error()
    assert lib.lrm_pileup_sites_host(cols.ctypes.data, b"A", 0, 1, None, None, 1, None) < 0
    assert lib.lrm_pileup_sites_host(None, None, 0, 0, None, None, 0, None) == 0


@pytest.fixture(scope="module")
def random_records():
    """10 000 records with small and large counters over text bytes of every kind, and the reference's answer (made once)"""
    rng = np.random.default_rng(4242)
    n = 10_000
    rows = []
    for k in range(n):
        hi = (3, 12, 40, 2**31)[k % 4]
        x = rng.integers(0, hi, 4) * (rng.random(4) < 0.5)
        n_eq, other, n_del = int(rng.integers(0, 2 * hi)), int(rng.integers(0, 3)), int(rng.integers(0, hi) * (rng.random() < 0.4))
        rows.append((n_eq + int(x.sum()) + other + n_del, n_eq, *(int(v) for v in x), n_del, int(rng.integers(0, hi) * (rng.random() < 0.4))))
    content = bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTacgtNn-", dtype=np.uint8), size=n))
    opts = {o: R.sites(R.cols_array(rows), content, 12345, R.options(*o)) for o in ((0, 0, 0, 0), (3, 2, 10, 0), (30, 1, 100, 0))}
    return as_cols(rows), content, opts


def test_host_rule_on_random_records(random_records):
    cols, content, opts = random_records
    assert (cols["depth"].astype(np.int64) != cols["depth"]).sum() == 0 and (cols["depth"] < cols["n_eq"]).any()    # some depths wrapped
    for o, (want, want_cons) in opts.items():
        assert 500 < len(want) < len(cols) and {chr(b) for b in want_cons} == set("ACGTN-"), o
        got, total, cons, outside, cons_outside = host_sites(cols, content, 12345, o)
        assert total == len(want) and got == want and cons == want_cons, o
        assert (outside == FILL).all() and (cons_outside == FILL).all()


def test_cap_below_at_and_above_the_total(random_records):
    cols, content, opts = random_records
    want, want_cons = opts[(0, 0, 0, 0)]
    total = len(want)
    for cap in (0, 1, total // 2, total - 1, total, total + 1, total + 100):
        got, n, cons, outside, cons_outside = host_sites(cols, content, 12345, None, cap=cap)
        assert n == total and got == want[:cap] and cons == want_cons, cap
        assert (outside == FILL).all() and (cons_outside == FILL).all(), cap      # nothing from cap on, nothing outside cons[0 .. count)
    got, n, cons, outside, _ = host_sites(cols, content, 12345, None, cap=7, cons=False)
    assert n == total and got == want[:7] and (outside == FILL).all()
    # a sub-range: position and content move together
    got, n, cons, _, _ = host_sites(cols[100:150], content[100:150], 12345 + 100, None)
    assert got == [s for s in want if 12345 + 100 <= s[0] < 12345 + 150] and cons == want_cons[100:150]


def test_format_lines(random_records, tmp_path):
    cols, content, opts = random_records
    seqs = [synth.reference(300, seed=5), synth.reference(200, seed=6)]
    hi = index.HostIndex.build(seqs, names=["chr1 primary", "chr2"], hlen=3)
    entries = hi.mta()
    mta = textio.mta_table(entries)
    (n1, off1, len1), (n2, off2, len2) = entries
    # the sites of the random records, re-seated on positions of both sequences, the second sequence first in part
    want = opts[(0, 0, 0, 0)][0][:120]
    at = [off1, off1 + 1, off1 + len1 - 1, off2, off2 + 7, off2 + len2 - 1, off1 + 5] + [off1 + 10 + 2 * k for k in range(113)]
    sites = np.zeros(len(want), dtype=capi.PILEUP_SITE_DT)
    tuples = []
    for k, (s, p) in enumerate(zip(want, at)):
        tuples.append((p,) + s[1:])
        sites[k] = tuples[-1]
    assert {t[9] for t in tuples} == {1, 2, 3, 4, 5, 6, 7}
    lines = "".join(R.line(*((n2, p - off2 + 1) if p >= off2 else (n1, p - off1 + 1)), t) for p, t in zip(at, tuples))
    room = 200 * len(sites)
    buf = C.create_string_buffer(room)
    k = lib.lrm_pileup_sites_format(mta, len(mta), sites.ctypes.data, len(sites), buf, room)
    assert k == len(lines) and buf.raw[:k].decode() == lines and buf.raw[k] == 0
    assert lines.splitlines()[0].split("\t")[:2] == ["chr1 primary", "1"] and lines.splitlines()[3].split("\t")[:2] == ["chr2", "1"]
    assert textio.sites_text(hi, sites).decode() == lines
    assert textio.write_sites(str(tmp_path / "a.sites"), hi, sites, chunk=50) == len(sites) and open(tmp_path / "a.sites").read() == lines
    # no sites: an empty text; a buffer that is too small, a position in no sequence and null arguments are refused
    assert lib.lrm_pileup_sites_format(mta, len(mta), None, 0, buf, room) == 0 and buf.raw[0] == 0
    for small in (1, 20, len(lines) // 2, len(lines)):
        assert lib.lrm_pileup_sites_format(mta, len(mta), sites.ctypes.data, len(sites), buf, small) < 0 and b"too small" in lib.lrm_last_error(), small
    gap = sites[:3].copy()
    gap["pos"][1] = off1 + len1                                          # the filler between the sequences
    assert lib.lrm_pileup_sites_format(mta, len(mta), gap.ctypes.data, 3, buf, room) < 0 and b"no sequence" in lib.lrm_last_error()
    gap["pos"][1] = off2 + len2
    assert lib.lrm_pileup_sites_format(mta, len(mta), gap.ctypes.data, 3, buf, room) < 0
    assert lib.lrm_pileup_sites_format(None, 2, sites.ctypes.data, 1, buf, room) < 0 and lib.lrm_pileup_sites_format(mta, len(mta), sites.ctypes.data, 1, None, room) < 0
    # the consensus of a sequence as FASTA: deletions dropped, 60 columns
    lo, hi_ = index.text_window(hi, 1)
    cons = np.frombuffer(b"ACGTN-" * 100, dtype=np.uint8)[:hi_ - lo + 5]
    assert textio.write_consensus(str(tmp_path / "c.fa"), hi, 1, cons, lo) == len2 - bytes(cons[:len2]).count(b"-")
    got = open(tmp_path / "c.fa").read().splitlines()
    assert got[0] == ">chr2" and "".join(got[1:]) == bytes(cons[:len2]).decode().replace("-", "") and {len(l) for l in got[1:-1]} == {60} and 0 < len(got[-1]) <= 60
    hi.close()


def test_records_and_abi():
    assert lib.lrm_abi_version() == 3 and capi.N_KERNELS == 9
    assert C.sizeof(capi.PileupSite) == 32 == capi.PILEUP_SITE_DT.itemsize and C.sizeof(capi.PileupCallOptions) == 16
    assert [(f, getattr(capi.PileupSite, f).offset) for f, _ in capi.PileupSite._fields_] == [
        ("pos", 0), ("depth", 8), ("n_ref", 12), ("n_alt", 16), ("n_del", 20), ("n_ins", 24), ("ref", 28), ("alt", 29), ("cons", 30), ("kinds", 31)]
    assert [f for f, _ in capi.PileupCallOptions._fields_] == ["min_depth", "min_count", "min_pct", "reserved"]
    assert capi.LATER_STRUCTS[capi.PileupSite] == "lrm_pileup_site" and capi.LATER_STRUCTS[capi.PileupCallOptions] == "lrm_pileup_call_options"
    assert (capi.CALL_SNV, capi.CALL_DEL, capi.CALL_INS) == (R.SNV, R.DEL, R.INS) == (1, 2, 4)
    assert [capi.CONSTANTS["LRM_CALL_" + k] for k in ("SNV", "DEL", "INS")] == [1, 2, 4]
    assert capi.PILEUP_SITE_DT.names == R.SITE_FIELDS
    for name in ("lrm_pileup_sites_dev", "lrm_pileup_sites_host", "lrm_pileup_sites_format"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
    from longreadmapper_amd import mapper
    assert hasattr(mapper.DeviceMapper, "pileup_sites") and all(hasattr(textio, f) for f in ("sites_text", "write_sites", "write_consensus"))


def test_sanitized_host_harness(random_records, tmp_path):
    """tests/models/pileup_call_harness.cpp, with its own main, built with -fsanitize=address,undefined and run as a child
    process: the records, the text, the table and the cons buffer in heap blocks of exactly their size, for a table that
    holds every site, one that is a record short, one of a single record and none."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "pileup_call_harness"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "longreadmapper_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "models", "pileup_call_harness.cpp"), "-o", str(exe)])
    cols, content, opts = random_records
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    for o, (want, want_cons) in opts.items():
        for cap in (len(want), len(want) - 1, 1, 0):
            (tmp_path / "in.bin").write_bytes(struct.pack("<QQQIII", 12345, len(cols), cap, *o[:3]) + cols.tobytes() + content)
            p = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, capture_output=True, text=True)
            assert p.returncode == 0, p.stderr[-3000:]
            raw = (tmp_path / "out.bin").read_bytes()
            kept = min(cap, len(want))
            assert struct.unpack("<Q", raw[:8])[0] == len(want) and len(raw) == 8 + 32 * kept + len(cols), (o, cap)
            assert R.as_tuples(np.frombuffer(raw[8:8 + 32 * kept], dtype=capi.PILEUP_SITE_DT)) == want[:cap] and raw[8 + 32 * kept:] == want_cons, (o, cap)


def test_planted_variants_on_the_oracle():
    """The end-to-end inputs of tests/test_gpu_pileup_sites.py, proved where no GPU is needed: the oracle maps the reads of
    the copy against the original text (classic mode), their op bytes go through the host rules, and every planted variant
    is found.  These are conditions on the inputs: a seed that misses them is replaced here, before any GPU run."""
    w = K.planted()
    hi = index.HostIndex.build([w["text"]], hlen=10)
    oi = orc.OracleIndex.from_host_index(hi)
    best, _ = oi.seed_batch(w["reads"], w["lens"], nthreads=8)
    reads = w["reads"].copy()
    ext = oi.extend_batch(reads, w["lens"], best, nthreads=8)
    lo, hi_ = index.text_window(hi, 0)
    W = hi_ - lo
    assert W == K.PLANT_TEXT
    planes = np.zeros(8 * W + 1, dtype=np.uint32)
    for i in range(len(reads)):
        n = int(ext["n_ops"][i])
        if n > 0 and ext["meta_r"][i] != 0 and ext["score"][i] != -1:
            lib.lrm_pileup_add_host(ext["ops"][i].ctypes.data, n, reads[i].ctypes.data, int(w["lens"][i]), int(ext["meta"]["loc"][i]), lo, hi_,
                                    planes.ctypes.data)
    cols = np.zeros(W, dtype=capi.PILEUP_COL_DT)
    capi.check(lib.lrm_pileup_cols_host(planes.ctypes.data, lo, hi_, 0, W, cols.ctypes.data), "lrm_pileup_cols_host")
    assert 35 < cols["depth"].mean() < 45
    content = hi.content()[lo:hi_].copy()
    sites = np.zeros(W, dtype=capi.PILEUP_SITE_DT)
    cons = np.zeros(W, dtype=np.uint8)
    total = lib.lrm_pileup_sites_host(cols.ctypes.data, content.ctypes.data, lo, W, None, sites.ctypes.data, W, cons.ctypes.data)
    assert total >= 60
    sites = sites[:total]
    want, want_cons = R.sites(cols, bytes(content), lo, R.options())
    assert R.as_tuples(sites) == want and bytes(cons) == want_cons
    missing, away = K.planted_conditions(w, sites, lo)
    print("planted variants: %d sites, %d of them more than 10 positions from every planted variant" % (total, away))
    assert not missing, missing
    hi.close()
