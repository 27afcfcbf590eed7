"""Mapping quality (docs/GACT_SPEC.md, "Mapping quality") without a GPU:

  (a) longreadmapper_amd/csrc/mapq_rule.h -- the arithmetic mapq_vote_kernel compiles -- built as plain C and held against
      tests/mapq_ref.py: radius, window edges, wrapped keys, the staggered histograms, the 32-bit table word, the formula;
  (b) the boundary: the record's layout, lrm_result_flags_mapq, the entry points, lrm_map_options untouched;
  (c) lrm_sam_format_mapq: column 5, v1:i / v2:i, the primary's entry inside a supplementary line's SA:Z."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapq_ref
from longreadmapper_amd import capi, mapper, textio
from longreadmapper_amd.capi import lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "mapq_rule_harness.c")
HDR = os.path.join(HERE, "..", "longreadmapper_amd", "csrc", "mapq_rule.h")
LIB = os.path.join(HERE, "models", "libmapq_rule_harness.so")
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def mq():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-o", LIB, SRC])
    so = C.CDLL(LIB)
    u32, u64 = C.c_uint32, C.c_uint64
    for name, res, args in (("mqh_radius_log2", u32, [u32]), ("mqh_radius", u32, [u32]), ("mqh_inside", C.c_int, [u64, u64, u32]),
                            ("mqh_bucket", u64, [u64, u32, u32]), ("mqh_tag", u32, [u64, u32, u32]), ("mqh_tag_empty", u32, []),
                            ("mqh_value", u32, [u32, u32])):
        getattr(so, name).restype, getattr(so, name).argtypes = res, args
    return so


# ---------------------------------------------------------------------------------------------------------
# (a) the kernel's arithmetic against the rule
# ---------------------------------------------------------------------------------------------------------
def test_radius(mq):
    want = {1: 512, 4096: 512, 4097: 1024, 16384: 2048, 16385: 4096, 1 << 20: 1 << 17, 10_000: 2048, 100_000: 16384, 0: 512}
    for n, R in want.items():
        assert mq.mqh_radius(n) == R == mapq_ref.radius(n) == 1 << mq.mqh_radius_log2(n), n
    rng = np.random.default_rng(1)
    for n in [int(x) for x in rng.integers(1, 1 << 24, 2000)] + [(1 << k) + d for k in range(1, 31) for d in (-1, 0, 1)]:
        R = mq.mqh_radius(n)
        assert R == mapq_ref.radius(n)
        if n > 4096:
            assert n / 8 <= R < n / 4 + 1 and R & (R - 1) == 0


@pytest.mark.parametrize("best", [0, 5, 511, 512, 1 << 20, (1 << 39) - 1, M64, M64 - 700, (-(1 << 32)) & M64])
def test_window_edges_and_wrapped_keys(mq, best):
    for r in (9, 10, 11, 14, 17):
        R = 1 << r
        for delta, want in ((0, 1), (R, 1), (-R, 1), (R + 1, 0), (-R - 1, 0), (R - 1, 1), (1 - R, 1), (3 * R, 0), (-(1 << 40), 0)):
            key = (best + delta) & M64
            assert mq.mqh_inside(key, best, r) == want == int(mapq_ref.inside(key, best, r)), (best, r, delta)


def test_a_cluster_R_wide_lies_whole_in_one_bucket_of_one_histogram(mq):
    for r in (9, 11):
        R = 1 << r
        for base in (0, 7 << 20, (-3 * R) & M64, (-(1 << 32)) & M64, (1 << 39) - 4 * R):
            for off in range(0, 2 * R, 7 if r == 11 else 1):                       # every offset mod 2 R (a stride for the wide one)
                lo = (base + off) & M64
                ends = [lo, (lo + R) & M64, (lo + R // 2) & M64]
                whole = [len({mq.mqh_bucket(k, r, h) for k in ends}) == 1 for h in (0, 1)]
                assert any(whole), (r, base, off)
                for k in ends:
                    for h in (0, 1):
                        assert mq.mqh_bucket(k, r, h) == mapq_ref.bucket(k, r, h)
                # one base further apart than the two histograms promise: still never split in BOTH unless wider than R
                assert len({mq.mqh_bucket(lo, r, 0), mq.mqh_bucket((lo + 2 * R) & M64, r, 0)}) == 2


def test_the_table_word_identifies_the_pair(mq):
    """32 bits of (histogram, bucket): distinct buckets of the key range give distinct words, none is the EMPTY mark."""
    empty = mq.mqh_tag_empty()
    rng = np.random.default_rng(3)
    for r in (9, 12, 17):
        keys = [int(x) for x in rng.integers(0, 1 << 39, 4000)] + [(-int(x)) & M64 for x in rng.integers(1, 1 << 32, 4000)]
        keys += [0, (1 << 39) - 1, M64, (-(1 << 32)) & M64, (-(1 << r)) & M64, (-(1 << r) - 1) & M64, (-(3 << r)) & M64]
        seen = {}
        for k in keys:
            for h in (0, 1):
                t = mq.mqh_tag(k, r, h)
                assert t != empty and (t & 1) == h
                b = mq.mqh_bucket(k, r, h)
                assert seen.setdefault(t, b) == b, (r, k, h)
        assert len(seen) > 1000


def test_formula(mq):
    for n1 in range(0, 13):
        for n2 in range(0, 15):
            assert mq.mqh_value(n1, n2) == mapq_ref.value(n1, n2), (n1, n2)
    assert [mapq_ref.value(*x) for x in ((0, 0), (1, 0), (5, 0), (10, 0), (200, 0), (200, 200), (200, 300), (200, 10), (12, 1))] == \
        [0, 6, 30, 60, 60, 0, 0, 57, 55]
    for n1, n2 in ((4_000_000_000, 0), (4_000_000_000, 3_999_999_999), (123_456_789, 6_172_839)):      # 64-bit products
        assert mq.mqh_value(n1, n2) == mapq_ref.value(n1, n2)


def test_rule_on_constructed_hits():
    """mapq_ref on hand-made hit lists: two equal copies, a unique locus with strays, few hits, the overflow switch."""
    R = 512
    copy_a = [1000 + 3 * i for i in range(40)]
    copy_b = [50_000 + 3 * i for i in range(40)]
    assert mapq_ref.record_of_hits(copy_a + copy_b, (1000, 9, 62), 1000, 0)[:6] == (40, 40, R, 0, 0, 0)
    strays = [200_000 + 5000 * i for i in range(3)]
    assert mapq_ref.record_of_hits(copy_a + strays, (1000, 9, 62), 1000, 4)[:6] == (40, 1, R, 58, 4, 0)
    assert mapq_ref.record_of_hits(copy_a[:4], (1000, 4, 62), 1000, 20)[:6] == (4, 0, R, 24, 20, 0)
    assert mapq_ref.record_of_hits(copy_a, (0, 0, 0), 1000, 20)[:6] == (0, 0, 0, 0, 0, 0)                  # no locus
    # a rival cluster R wide that straddles a bucket edge of histogram 0 is whole in histogram 1
    edge = [4096 * 10 + 1024 - 256 + i * 8 for i in range(64)]
    assert mapq_ref.record_of_hits(copy_a + edge, (1000, 9, 62), 1000, 0)[:2] == (40, 64)
    # hits R + 1 away from the winner are rivals, hits R away are support
    assert mapq_ref.record_of_hits([1000, 1000 + R, 1000 + R + 1, 1000 - R, 999 - R], (1000, 1, 62), 1000, 0)[:2] == (3, 1)
    many = [10_000_000 + 3000 * i for i in range(20)]
    rec = mapq_ref.record_of_hits(copy_a + many, (1000, 9, 62), 1000, 0, slots=16)
    assert rec[6] > 16 and rec[:6] == (40, 40, R, 0, 0, mapq_ref.OVERFLOW)
    assert mapq_ref.record_of_hits(copy_a + many[:4], (1000, 9, 62), 1000, 0, slots=16)[5] == 0


# ---------------------------------------------------------------------------------------------------------
# (b) the boundary
# ---------------------------------------------------------------------------------------------------------
def test_record_layout_symbols_and_untouched_options():
    assert C.sizeof(capi.Mapq) == 16 == mapper.MAPQ_DT.itemsize == mapq_ref.REC_DT.itemsize
    assert [(f, mapper.MAPQ_DT.fields[f][1]) for f in ("n1", "n2", "radius", "mapq", "phase", "flags")] == \
        [("n1", 0), ("n2", 4), ("radius", 8), ("mapq", 12), ("phase", 13), ("flags", 14)]
    assert capi.Mapq.mapq.offset == 12 and capi.Mapq.flags.offset == 14
    assert (capi.MAPQ_SLOTS, capi.MAPQ_OVERFLOW) == (mapq_ref.SLOTS, mapq_ref.OVERFLOW) == (4096, 1)
    for name in ("lrm_seed_batch_mapq_dev", "lrm_map_batch_submit_mapq", "lrm_result_flags_mapq", "lrm_sam_format_mapq",
                 "lrm_accaln_mapq", "lrm_debug_set_mapq_slots"):
        assert getattr(lib, name) is not None and name in capi.SYMBOLS
    # the stage is asked for per call: lrm_map_options did not grow, its init leaves every word but struct_size zero
    o = capi.map_options()
    assert o.struct_size == C.sizeof(capi.MapOptions) and not any(bytes(o)[4:])
    assert lib.lrm_abi_version() == 3 and mapper.N_KERNELS == 9
    assert lib.lrm_debug_set_mapq_slots(None, 16) < 0


def test_result_flags_with_and_without_records():
    rng = np.random.default_rng(9)
    n = 500
    score = rng.integers(-1, 50, n).astype(np.int32)
    meta_r = (rng.random(n) < 0.9).astype(np.int32)
    meta = np.zeros(n, dtype=mapper.META_DT)
    meta["strand"] = rng.integers(0, 2, n)
    rec = np.zeros(n, dtype=mapper.MAPQ_DT)
    rec["mapq"] = rng.integers(0, 61, n)
    rec["n1"], rec["n2"] = rng.integers(0, 500, n), rng.integers(0, 500, n)
    flag0, mapq0, valid0 = mapper.result_flags(score, meta_r, meta)
    flag, out, valid = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.lrm_result_flags_mapq(score.ctypes.data, meta_r.ctypes.data, meta.ctypes.data, None, n, flag.ctypes.data, out.ctypes.data,
                              valid.ctypes.data)
    assert np.array_equal(flag, flag0) and np.array_equal(out, mapq0) and np.array_equal(valid, valid0)        # NULL: lrm_result_flags
    flag1, mapq1, valid1 = mapper.result_flags(score, meta_r, meta, mapq=rec)
    unmapped = (meta_r == 0) | (score == -1)
    assert unmapped.any() and (~unmapped).any()
    assert np.array_equal(flag1, flag0) and np.array_equal(valid1, valid0)
    assert not mapq1[unmapped].any() and np.array_equal(mapq1[~unmapped], rec["mapq"][~unmapped])
    assert set(mapq0[~unmapped]) == {255}


# ---------------------------------------------------------------------------------------------------------
# (c) SAM text
# ---------------------------------------------------------------------------------------------------------
def _batch(tmp_path, recs):
    p = tmp_path / "r.fq"
    p.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (nm, s, q) for nm, s, q in recs))
    rd = textio.Reader(p)
    assert rd.next(100) == len(recs)
    return rd, rd.batch


def test_sam_lines_with_records(tmp_path):
    rng = np.random.default_rng(11)
    mta = textio.mta_table([(b"chrA", 0, 100000), (b"chrB", 200000, 50000)])
    lens = [900, 400, 300, 250]
    seqs = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, k)) for k in lens]
    quals = [bytes(33 + (i + j) % 60 for j in range(k)) for i, k in enumerate(lens)]
    # read 0: a reported right segment; 1: reverse strand; 2: forward; 3: unmapped
    ops = [b"=" * 600 + b"S" * 300, b"=" * 200 + b"X" + b"=" * 199, b"=" * 300, b""]
    score = np.array([3, 1, 0, -1], dtype=np.int32)
    meta_r = np.array([1, 1, 1, 1], dtype=np.int32)
    meta = np.zeros(4, dtype=mapper.META_DT)
    meta["seq_id"], meta["off"], meta["strand"] = [0, 1, 0, 0], [17, 2017, 4017, 0], [0, 1, 0, 0]
    rd, b = _batch(tmp_path, [(b"q%d" % i, seqs[i], quals[i]) for i in range(4)])
    cig, keep1 = textio.cigar_array(ops, score)
    seg = np.zeros(1, dtype=mapper.SEGMENT_DT)
    seg[0] = (0, 600, 300, capi.SEG_RIGHT | capi.SEG_ALIGNED)
    rows = np.zeros((1, 320), dtype=np.uint8)
    rows[0, :300] = np.frombuffer(seqs[0][600:], dtype=np.uint8)
    sscore, smeta_r = np.array([7], dtype=np.int32), np.array([1], dtype=np.int32)
    smeta = np.zeros(1, dtype=mapper.META_DT)
    smeta["seq_id"], smeta["off"] = 1, 5000
    scig, keep2 = textio.cigar_array([b"=" * 300], sscore)
    out = capi.SplitOut(1, 1, seg.ctypes.data, rows.ctypes.data, 320, None, None, scig.ctypes.data, None, 0,
                        sscore.ctypes.data, smeta.ctypes.data, smeta_r.ctypes.data, None, None)
    rec = np.zeros(4, dtype=mapper.MAPQ_DT)
    rec["n1"], rec["n2"], rec["mapq"], rec["radius"] = [31, 12, 9, 5], [2, 12, 0, 1], [56, 0, 54, 33], 512

    def fmt(split, mqp):
        return textio.sam_format(b, mta, cig, score, meta, meta_r, 4, split=split, mapq=mqp, entry="lrm_sam_format_mapq")

    def fmt_split(split):
        return textio.sam_format(b, mta, cig, score, meta, meta_r, 4, split=split, entry="lrm_sam_format_split")

    for split in (None, out):
        plain = fmt_split(split)
        assert fmt(split, None) == plain                                  # NULL: lrm_sam_format_split byte for byte
        got = fmt(split, rec).splitlines()
        base = plain.splitlines()
        assert len(got) == len(base) == (5 if split else 4)
        want = []
        for ln in base:
            f = ln.split("\t")
            i = int(f[0][1:])
            if int(f[1]) & 2048:                                          # a segment's line: its own MAPQ stays 255, the primary's entry carries the record's
                assert f[4] == "255" and f[-1] == "SA:Z:chrA,18,+,600M300S,255,3;"
                f[-1] = "SA:Z:chrA,18,+,600M300S,56,3;"
            else:
                f[4] = "0" if i == 3 else str(int(rec["mapq"][i]))
                at = next(k for k, x in enumerate(f) if x.startswith("ED:I:"))
                f[at + 1:at + 1] = ["v1:i:%d" % rec["n1"][i], "v2:i:%d" % rec["n2"][i]]
            want.append("\t".join(f))
        assert got == want
        assert [x.split("\t")[4] for x in got if not int(x.split("\t")[1]) & 2048] == ["56", "0", "54", "0"]
    first = fmt(out, rec).splitlines()[0].split("\t")
    assert first[-3:] == ["v1:i:31", "v2:i:2", "SA:Z:chrB,5001,+,600S300M,255,7;"]       # the segment's own entry keeps 255
    rd.close()


def test_reference_on_the_oracle_agrees_with_the_scalar_rule():
    """mapq_ref.batch (numpy over the oracle's trace) against the rule applied hit by hit with Python integers."""
    import orc
    import workloads
    for name in ("ont-2k", "repeats-ties", "ragged", "last-phase-break"):
        sc = workloads.scenario(name)
        oi = orc.OracleIndex.from_host_index(sc["hi"])
        recs, pairs = mapq_ref.batch(oi, sc["reads"][:12], sc["lens"][:12], sc["seed_len"], sc["thres"])
        sa = oi.sa()
        for i in range(min(12, len(sc["lens"]))):
            read = bytes(sc["reads"][i, :int(sc["lens"][i])])
            tr = oi.seed_read(read, sc["seed_len"], sc["thres"], trace=True)
            best, d = tr["best"], tr["phases"] - 1
            got = tuple(int(recs[i][f]) for f in ("n1", "n2", "radius", "mapq", "phase", "flags"))
            if best[1] == 0:
                assert got == (0,) * 6
                continue
            r = mapq_ref.radius_log2(len(read))
            n1, hist = 0, {}
            for j, rr, k, l in tr["seeds"]:
                if 0 < rr < sc["thres"]:
                    for row in range(k, l + 1):
                        key = (int(sa[row]) - j) & M64
                        if mapq_ref.inside(key, best[0], r):
                            n1 += 1
                        else:
                            for h in (0, 1):
                                hist[(h, mapq_ref.bucket(key, r, h))] = hist.get((h, mapq_ref.bucket(key, r, h)), 0) + 1
            n2 = max(hist.values()) if hist else 0
            assert got == (n1, n2, 1 << r, mapq_ref.value(n1, n2), d, 0) and pairs[i] == len(hist) and n1 >= 1, (name, i)
        if name == "ont-2k":
            assert (recs["mapq"] >= 50).all() and (recs["phase"] == 20).all()
        if name == "repeats-ties":
            assert (recs["mapq"] == 0).sum() >= 4 and (recs["n2"] > 0).all()      # reads inside the 40-copy element: every copy ties
