"""Secondary alignments (docs/GACT_SPEC.md, "Secondary alignments") without a GPU:

  (a) longreadmapper_amd/csrc/rival_rule.h -- the arithmetic rival_locus_kernel compiles -- built as plain C, and
      lrm_rival_host, held against tests/rival_ref.py on constructed key sets: ties of pairs and of sub-buckets, bucket edges,
      wrapped keys, every sub-bucket width, both sides of the candidate thresholds;
  (b) lrm_secondary_plan against the rule on random records;
  (c) the boundary: the structs, the symbols, what must not have grown."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapq_ref
import rival_ref
from longreadmapper_amd import capi, mapper
from longreadmapper_amd.capi import lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "rival_rule_harness.c")
HDRS = [os.path.join(HERE, "..", "longreadmapper_amd", "csrc", h) for h in ("rival_rule.h", "mapq_rule.h")]
LIB = os.path.join(HERE, "models", "librival_rule_harness.so")
M64 = (1 << 64) - 1
WIN = [1000 + 3 * i for i in range(40)]          # the winner's cluster of the constructed sets: n1 = 40 around key 1000
BEST = (1000, 9, 62)


@pytest.fixture(scope="module")
def rv():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-o", LIB, SRC])
    so = C.CDLL(LIB)
    u32, u64 = C.c_uint32, C.c_uint64
    for name, res, args in (("rvh_min_hits", u32, [u32]), ("rvh_ratio_pct", u32, [u32]), ("rvh_candidate", C.c_int, [u32] * 5),
                            ("rvh_sub_shift", u32, [u32]), ("rvh_off", u32, [u64, u32, u32]), ("rvh_key_of", u64, [u32, u32, u32]),
                            ("rvh_tag", u32, [u64, u32, u32]), ("rvh_sub_buckets", u32, [])):
        getattr(so, name).restype, getattr(so, name).argtypes = res, args
    return so


def host_rule(keys, best, length, min_hits=0, ratio_pct=0, slots=0):
    """lrm_rival_host -> ((key, val, bucket), candidate)"""
    k = np.array([x & M64 for x in keys], dtype=np.uint64)
    b, out = capi.Entry(*best), capi.Entry(7, 7, 7)
    rc = capi.check(lib.lrm_rival_host(k.ctypes.data, len(k), C.byref(b), length, min_hits, ratio_pct, slots, C.byref(out)), "lrm_rival_host")
    return (out.key, out.val, out.bucket), rc


def rule(keys, best=BEST, length=1000, min_hits=0, ratio_pct=0, slots=0):
    """The entry three ways -- numpy, hit by hit, lrm_rival_host -- and in three orders of the hits; they agree."""
    want, rec = rival_ref.rival_of_hits(list(keys), best, length, min_hits, ratio_pct, slots or mapq_ref.SLOTS)
    assert rival_ref.rival_of_hits_scalar(list(keys), best, length, min_hits, ratio_pct, slots or mapq_ref.SLOTS)[0] == want
    rng = np.random.default_rng(len(keys))
    for order in (list(keys), list(keys)[::-1], [keys[i] for i in rng.permutation(len(keys))]):
        got, rc = host_rule(order, best, length, min_hits, ratio_pct, slots)
        assert got == want and rc == int(want != rival_ref.ZERO), (got, want)
    return want


# ---------------------------------------------------------------------------------------------------------
# (a) the arithmetic and the rule
# ---------------------------------------------------------------------------------------------------------
def test_arithmetic_of_the_header(rv):
    assert [rv.rvh_min_hits(x) for x in (0, 1, 8, 65535, 65536)] == [8, 1, 8, 65535, 0]
    assert [rv.rvh_ratio_pct(x) for x in (0, 1, 50, 100, 101)] == [50, 1, 50, 100, 0]
    assert [rv.rvh_sub_shift(r) for r in (9, 11, 14, 15, 17, 29)] == [4, 4, 4, 5, 7, 19] == [rival_ref.sub_shift(r) for r in (9, 11, 14, 15, 17, 29)]
    assert rv.rvh_sub_buckets() == 2048 and all((2 << r) >> rv.rvh_sub_shift(r) <= 2048 for r in range(9, 30))
    rng = np.random.default_rng(5)
    for n1, n2, flags, H, pct in rng.integers(0, 120, (4000, 5)):
        H, pct = int(H) % 70 + 1, int(pct) % 100 + 1
        assert rv.rvh_candidate(n1, n2, flags & 1, H, pct) == int(rival_ref.candidate(int(n1), int(n2), int(flags & 1), H, pct))
    assert rv.rvh_candidate(3_000_000_000, 1_500_000_000, 0, 8, 50) == 1 and rv.rvh_candidate(3_000_000_000, 1_499_999_999, 0, 8, 50) == 0
    # a hit's offset in its pair, and back: the key from the 32-bit table word and the offset
    for r in (9, 11, 14, 15, 17):
        R = 1 << r
        keys = [int(x) for x in rng.integers(0, 1 << 39, 2000)] + [(-int(x)) & M64 for x in rng.integers(1, 1 << 32, 2000)]
        keys += [0, R - 1, R, (1 << 39) - 1, M64, (-R) & M64, (-R - 1) & M64, (-(1 << 32)) & M64]
        for k in keys:
            for h in (0, 1):
                off = rv.rvh_off(k, r, h)
                assert off == ((k + h * R) - (mapq_ref.bucket(k, r, h) << (r + 1))) & M64 and off < 2 * R
                assert rv.rvh_key_of(rv.rvh_tag(k, r, h), r, off) == k, (r, k, h)


def test_tied_pairs_in_the_same_and_in_different_histograms():
    a = [50_000 + 2 * i for i in range(20)]          # upper half of bucket 48 of histogram 0: whole in (48, 0) and in (49, 1)
    b = [90_000 + 2 * i for i in range(20)]          # (87, 0) and (88, 1)
    # four pairs of 20: the smallest bucket wins; its sub-buckets 53 and 54 hold 8 hits each, 55 holds 4: the smallest index
    assert rule(WIN + a + b) == rule(WIN + b + a) == (50_000, 8, 50_000 >> 4)
    low = [49_152 + 100 + 2 * i for i in range(20)]  # lower half of bucket 48: (48, 0) and (48, 1) tie -- histogram 0 first
    assert rule(WIN + low + b) == (49_264, 8, 49_264 >> 4)   # offsets 100 .. 138: six hits in sub-bucket 6, the first eight in 7
    assert rule(WIN + b + [50_000 + 2 * i for i in range(21)])[0] == 50_000 and rule(WIN + a[:19] + b)[0] == 90_000     # no tie: the fullest


def test_cluster_across_a_bucket_edge_of_histogram_0_lies_whole_in_histogram_1():
    edge = [4096 * 10 + 1024 - 256 + i * 8 for i in range(64)]      # 32 hits on either side of 41 * 1024; (41, 1) holds all 64
    assert mapq_ref.record_of_hits(WIN + edge, BEST, 1000, 0)[:2] == (40, 64)
    assert rule(WIN + edge) == (edge[0], 2, edge[0] >> 4)            # sub-buckets of two hits each, all tied: the first
    dense = edge + [edge[40] + 1, edge[40] + 2]                      # ... but one of four
    assert rule(WIN + dense) == (edge[40], 4, edge[40] >> 4)


def test_three_sub_buckets_tied_and_the_smallest_key_last():
    base = 300 * 1024                                               # bucket 300 of histogram 0, lower half
    hits = [base + 16 * 9 + x for x in (15, 7, 3)] + [base + 16 * 5 + x for x in (12, 4, 9)] + [base + 16 * 20 + x for x in (0, 1, 2)]
    hits += [base + 16 * 7 + x for x in (1, 2)]
    got = rule(WIN + hits, min_hits=3, ratio_pct=1)
    assert got == (base + 16 * 5 + 4, 3, (base + 16 * 5 + 4) >> 4)
    got = rule(WIN + hits + [base + 16 * 5 + 0], min_hits=3, ratio_pct=1)         # the smallest key of the winner arrives last
    assert got == (base + 16 * 5, 4, (base + 16 * 5) >> 4)


def test_wrapped_keys_beside_plain_ones():
    wrapped = [(-3008 + 2 * i) & M64 for i in range(30)]       # 2^64 - 3008 is a multiple of 16: eight hits in its first sub-bucket
    plain = [70_000 + 2 * i for i in range(20)]
    assert rule(WIN + wrapped + plain) == (wrapped[0], 8, wrapped[0] >> 4)                     # the rival is the wrapped cluster
    assert rule(WIN + wrapped[:20] + plain)[0] == 70_000                                       # tied: the plain bucket is the smaller
    # around zero: histogram 1 puts -200 .. 200 into ONE bucket, 0; the smallest offset belongs to the most negative key
    zero = [(x - 200) & M64 for x in range(0, 400, 4)]
    best = (500_000, 9, 500_000 >> 4)
    win = [500_000 + 3 * i for i in range(40)]
    got = rule(win + zero, best)
    assert mapq_ref.record_of_hits(win + zero, best, 1000, 0)[:2] == (40, 100)
    # offsets 312, 316, ... in (0, 1): sub-bucket 19 holds two hits, 20 the first four -- the key at offset 320 is -192
    assert got == ((-192) & M64, 4, ((-192) & M64) >> 4)
    # a wrapped winner, a plain rival
    wb = (wrapped[0], 9, wrapped[0] >> 4)
    assert rule(wrapped + wrapped + plain, wb, ratio_pct=30)[0] == 70_000


@pytest.mark.parametrize("length, r, s", [(1000, 9, 4), (10_000, 11, 4), (100_000, 14, 4), (140_000, 15, 5), (600_000, 17, 7)])
def test_every_sub_bucket_width(length, r, s):
    assert mapq_ref.radius_log2(length) == r and rival_ref.sub_shift(r) == s
    R = 1 << r
    rng = np.random.default_rng(r)
    n_cand = 0
    for trial in range(12):
        at = int(rng.integers(10 * R, 1 << 30))
        keys = [at + int(x) for x in rng.integers(-R // 2, R // 2, 60)]
        for _ in range(int(rng.integers(1, 6))):                    # rival clusters of several sizes and widths, some wrapped
            c = int(rng.integers(1 << 31, 1 << 38)) if rng.random() < 0.8 else (-int(rng.integers(1, 1 << 31))) & M64
            width = int(rng.integers(1, 3 * R))
            keys += [(c + int(x)) & M64 for x in rng.integers(0, width, int(rng.integers(5, 80)))]
        got = rule(keys, (at, 9, at >> 4), length)
        n_cand += got != rival_ref.ZERO
        if got != rival_ref.ZERO:
            assert got[0] in keys and got[2] == got[0] >> 4 and 1 <= got[1] <= 80
    assert n_cand >= 6
    # sub-buckets are 2^s wide: 2^s hits in one of them, one hit next door
    base = 5000 * 2 * R
    one = [base + (3 << s) + x for x in range(0, 1 << s, max(1, (1 << s) // 16))]
    assert rule([at + x for x in range(40)] + one + [base + (4 << s)], (at, 9, at >> 4), length, ratio_pct=1) == (one[0], len(one), one[0] >> 4)


def test_both_sides_of_the_thresholds():
    rival = [50_000 + 2 * i for i in range(20)]
    assert rule(WIN[:10] + rival[:7]) == rival_ref.ZERO and rule(WIN[:10] + rival[:8])[0] == 50_000            # n2 = H - 1, n2 = H
    assert rule(WIN[:10] + rival[:2], min_hits=3) == rival_ref.ZERO and rule(WIN[:10] + rival[:3], min_hits=3, ratio_pct=30)[0] == 50_000
    assert rule(WIN + rival[:19]) == rival_ref.ZERO and rule(WIN + rival)[0] == 50_000                         # 100 n2 = pct n1, one below
    assert rule(WIN + rival[:9], ratio_pct=25) == rival_ref.ZERO and rule(WIN + rival[:10], ratio_pct=25)[0] == 50_000
    assert rule(WIN + rival + rival, ratio_pct=100)[0] == 50_000 and rule(WIN + rival + rival[:19], ratio_pct=100) == rival_ref.ZERO
    # more pairs than slots: the record overflows, no candidate -- with room for them it is one
    many = [10_000_000 + 3000 * i for i in range(20)]
    assert rule(WIN + rival + many, slots=16) == rival_ref.ZERO and rule(WIN + rival + many, slots=64)[0] == 50_000
    assert rule(WIN + rival + many[:6], slots=16)[0] == 50_000
    assert rule(WIN + rival, (1000, 0, 62)) == rival_ref.ZERO                                                  # no locus
    assert rule([], (0, 0, 0)) == rival_ref.ZERO and rule(WIN) == rival_ref.ZERO
    for bad in (dict(min_hits=65536), dict(ratio_pct=101)):
        with pytest.raises(capi.LrmError, match="outside"):
            host_rule(WIN + rival, BEST, 1000, **bad)


# ---------------------------------------------------------------------------------------------------------
# (b) the table
# ---------------------------------------------------------------------------------------------------------
def _plan(rec, min_hits, ratio_pct, cap):
    table = np.zeros(max(cap, 1), dtype=mapper.SECONDARY_DT)
    table["read"] = 0xABCD
    k = C.c_uint64()
    rc = lib.lrm_secondary_plan(rec.ctypes.data, len(rec), min_hits, ratio_pct, table.ctypes.data if cap else None, cap, C.byref(k))
    return rc, int(k.value), table


def test_plan_against_the_rule_on_random_records():
    rng = np.random.default_rng(21)
    n = 3000
    rec = np.zeros(n, dtype=mapper.MAPQ_DT)
    rec["n1"], rec["n2"] = rng.integers(0, 60, n), rng.integers(0, 60, n)
    rec["flags"] = rng.random(n) < 0.1
    rec[::17] = 0
    for H, pct in ((0, 0), (1, 1), (20, 90), (8, 100), (65535, 50)):
        want = rival_ref.plan(rec, H, pct)
        rc, k, table = _plan(rec, H, pct, n)
        assert rc == 0 and k == len(want) and np.array_equal(table["read"][:k], want)
        assert not table["hits"][:k].any() and not table["flags"][:k].any() and not table["_pad"][:k].any() and (table["read"][k:] == 0xABCD).all()
        if 0 < k:
            rc, k2, table = _plan(rec, H, pct, k - 1)
            assert rc == -3 and k2 == k and (table["read"] == 0xABCD).all()
            assert _plan(rec, H, pct, k)[0] == 0
    assert len(rival_ref.plan(rec)) > 300 and len(rival_ref.plan(rec, 65535, 50)) == 0
    assert _plan(rec, 0, 0, 0)[0] == -3 and _plan(rec[:0], 0, 0, 0)[:2] == (0, 0)
    assert _plan(rec, 70000, 0, n)[0] == -1 and _plan(rec, 0, 101, n)[0] == -1


# ---------------------------------------------------------------------------------------------------------
# (c) the boundary
# ---------------------------------------------------------------------------------------------------------
def test_structs_symbols_and_what_did_not_grow():
    for name in ("lrm_rival_dev", "lrm_rival_host", "lrm_secondary_plan", "lrm_secondary_batch_dev", "lrm_secondary_batch",
                 "lrm_sam_format_secondary", "lrm_accaln_secondary"):
        assert getattr(lib, name) is not None and name in capi.SYMBOLS
    assert lib.lrm_abi_version() == 3 and capi.N_KERNELS == 9 == mapper.N_KERNELS
    assert C.sizeof(capi.MapOptions) == 76 and C.sizeof(capi.BatchExtras) == 24
    assert C.sizeof(capi.Secondary) == 16 == mapper.SECONDARY_DT.itemsize and C.sizeof(capi.SecondaryOptions) == 32
    assert [(f, mapper.SECONDARY_DT.fields[f][1]) for f in ("read", "hits", "flags", "_pad")] == [("read", 0), ("hits", 4), ("flags", 8), ("_pad", 12)]
    assert [f for f, _ in capi.SecondaryDev._fields_] == ["cap", "table", "rows", "row_stride", "lens", "rival", "store", "store_stride",
                                                          "n_ops", "score", "meta", "meta_r", "anchor", "clip"]
    for s, c_name in ((capi.Secondary, "lrm_secondary"), (capi.SecondaryOptions, "lrm_secondary_options"), (capi.SecondaryDev, "lrm_secondary_dev")):
        assert capi.LATER_STRUCTS[s] == c_name                       # compared with the header by tests/test_aln_diff_cpu.py
    assert (capi.SEC_ALIGNED, capi.SEC_DUPLICATE) == (rival_ref.SEC_ALIGNED, rival_ref.SEC_DUPLICATE) == (1, 2)
    assert capi.CONSTANTS["LRM_SEC_ALIGNED"] == 1 and capi.CONSTANTS["LRM_SEC_DUPLICATE"] == 2
    k = C.c_uint64()
    assert lib.lrm_secondary_batch_dev(None, None, None, 0, None, 0, None, None, None, None, capi.Params(0, 20, 300), capi.GactParams(0, 0, 0),
                                       None, None, C.byref(k), None) < 0
    assert lib.lrm_secondary_batch(None, None, 0, None, 0, None, None, None, capi.Params(0, 20, 300), capi.GactParams(0, 0, 0), None, None, None) < 0
    assert hasattr(mapper, "secondary_batch") and hasattr(mapper, "SecondaryBuffers")
    assert lib.lrm_rival_dev(None, None, None, 0, capi.Params(0, 20, 300), None, None, 0, 0, None, None) < 0
