"""End clipping of the anchored mode (docs/GACT_SPEC.md, "End clipping") without a GPU:

  (a) longreadmapper_amd/csrc/anchor_clip.h -- the per-lane fold and the merge operator anchor_clip_kernel compiles --
      built as plain C and held against tests/clip_ref.py: every short row, and long rows cut into lane and wavefront
      pieces at every alignment of the seams;
  (b) properties of clip_ref.extend_clipped on the constructed texts of tests/anchored_cases.py;
  (c) the boundary: run-length text of op rows with 'S' runs, the option fields, the exported entry point."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import anchored_cases
import anchored_ref
import clip_ref
import orc
import sam_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "anchor_clip_harness.c")
HDR = os.path.join(HERE, "..", "longreadmapper_amd", "csrc", "anchor_clip.h")
LIB = os.path.join(HERE, "models", "libanchor_clip_harness.so")
BIAS = 1 << 31


@pytest.fixture(scope="module")
def acl():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", LIB, SRC])
    so = C.CDLL(LIB)
    so.acl_clip_row.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    so.acl_clip_row.restype = C.c_uint32
    return so


def _kernel_form(so, ops, P, B, first=16):
    """-> (keep, non_eq, non_I, non_D, best, sum) from the kernel's source."""
    out = (C.c_uint32 * 5)()
    keep = so.acl_clip_row(ops, len(ops), P, B, first, out)
    return keep, out[0], out[1], out[2], out[3] - BIAS, out[4] - BIAS


def _spec_form(ops, P, B):
    keep = clip_ref.clip_job(ops, P, B)
    kept = ops[:keep]
    scores = [clip_ref.prefix_score(ops, k, P) for k in range(len(ops) + 1)] if len(ops) <= 64 else None
    return (keep, len(kept) - kept.count(b"="), len(kept) - kept.count(b"I"), len(kept) - kept.count(b"D"),
            max(scores) if scores else None, scores[-1] if scores else None)


# ---------------------------------------------------------------------------------------------------------
# (a) the kernel's source against the rule
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,B", [(1, 1), (1, 6), (2, 1), (2, 6), (5, 1), (5, 6)])
def test_every_short_row(acl, P, B):
    checked = 0
    for m in range(10):
        for t in itertools.product(b"=XID", repeat=m):
            ops = bytes(t)
            assert _kernel_form(acl, ops, P, B) == _spec_form(ops, P, B), ops
            checked += 1
    assert checked == (4 ** 10 - 1) // 3
    # pieces of other widths see the same rows (the first piece 1 .. 16 columns wide)
    for t in itertools.product(b"=XID", repeat=6):
        ops = bytes(t) + b"==X="
        want = _spec_form(ops, P, B)
        for first in (1, 2, 5, 9, 10):
            assert _kernel_form(acl, ops, P, B, first) == want, (ops, first)


def _random_row(rng, m, p_eq):
    return bytes(rng.choice(np.frombuffer(b"=XID", dtype=np.uint8), size=m, p=[p_eq] + [(1 - p_eq) / 3] * 3))


def test_random_rows_at_every_alignment_of_the_seams(acl):
    rng = np.random.default_rng(1)
    lengths = [1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 5000] + [int(x) for x in rng.integers(1, 5001, 40)]
    kept_whole = clipped = 0
    for m in lengths:
        # a good stretch, then noise: the maximum lies somewhere inside the row
        cut = int(rng.integers(0, m + 1))
        ops = _random_row(rng, cut, 0.88) + _random_row(rng, m - cut, float(rng.choice([0.4, 0.6, 0.88])))
        for P, B in ((2, 6), (1, 1), (5, 6), (15, 255)):
            want = _spec_form(ops, P, B)[:4]
            for first in range(1, 17):
                assert _kernel_form(acl, ops, P, B, first)[:4] == want, (m, P, B, first)
            kept_whole += want[0] == m
            clipped += want[0] < m
    assert kept_whole > 20 and clipped > 20


def _rows_with_the_maximum_at(k, m):
    """Rows of m columns whose best prefix is exactly k (k > 0: column k - 1 is '=' and what follows only loses)."""
    good = b"=" * k
    return [good + b"X" * (m - k), good + (b"I=" * m)[:m - k], good + (b"D" * 3 + b"==" * 1) * ((m - k) // 5) + b"X" * ((m - k) % 5)]


@pytest.mark.parametrize("k", [0, 1, 15, 16, 17, 1008, 1023, 1024, 1025, 1040, 2048, 3072])
def test_maximum_at_zero_at_the_end_and_on_piece_boundaries(acl, k):
    """k = 0 (nothing aligns), k = m (nothing to clip), and k on a lane boundary (16), a wavefront boundary (1024, 2048)
    and one column either side of them."""
    for m in (k, k + 7, k + 16, k + 1024, k + 1500):
        for ops in _rows_with_the_maximum_at(k, m):
            assert len(ops) == m
            for P, B in ((2, 6), (1, 1)):
                want = _spec_form(ops, P, B)[:4]
                loss = sum(1 if c == ord("=") else -P for c in ops[k:])
                assert want[0] == (k if -loss > B else m)
                for first in (16, 1, 7, 15):
                    assert _kernel_form(acl, ops, P, B, first)[:4] == want, (k, m, P, B, first)


def test_ties_in_the_best_score_take_the_smallest_prefix(acl):
    # s = 0 at k = 0, back to 0 at k = 3 ("X=="), again at 6: keep 0 when the tail loses more than B
    for first in (16, 1, 2, 3, 4):
        assert _kernel_form(acl, b"X==X==" + b"X" * 4, 2, 6, first)[0] == 0
        assert _kernel_form(acl, b"X==X==" + b"X" * 3, 2, 6, first)[0] == 9            # gains exactly B: kept whole
        # the same peak twice, the second 16 / 1024 columns later (on the seams of the lanes / of the wavefront steps)
        for gap in (3, 16, 48, 1023, 1024, 1026):
            assert gap % 3 == 0 or gap in (16, 1024)
            back = (b"X==" * (gap // 3 + 1))[:gap] if gap % 3 == 0 else b"X" * (gap // 3) + b"=" * (gap - gap // 3)
            ops = b"=" * 20 + back + b"X" * 10
            keep = clip_ref.clip_job(ops, 2, 6)
            assert _kernel_form(acl, ops, 2, 6, first)[0] == keep
            if gap % 3 == 0:
                assert clip_ref.prefix_score(ops, 20 + gap, 2) == 20 and keep == 20


def test_the_end_bonus_is_a_strict_threshold(acl):
    for B in (1, 6, 40, 255):
        for P in (1, 2, 15):
            for x in range(0, B // P + 3):
                ops = b"=" * 30 + b"X" * x
                want = 30 if P * x > B else 30 + x
                assert clip_ref.clip_job(ops, P, B) == want and _kernel_form(acl, ops, P, B)[0] == want


def test_defaults_of_the_reference():
    assert clip_ref.clip_job(b"=" * 12 + b"XXXX") == clip_ref.clip_job(b"=" * 12 + b"XXXX", 2, 6) == 12
    assert clip_ref.clip_job(b"=" * 12 + b"XXX") == 15


# ---------------------------------------------------------------------------------------------------------
# (b) the rule on whole reads
# ---------------------------------------------------------------------------------------------------------
TEXT, MTA, CASES = anchored_cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_clipped_read_properties(case):
    S, len_s = MTA[case["seq"]]
    read, n = case["read"], len(case["read"])
    base = anchored_ref.extend(read, TEXT, case["L"], S, len_s, min_len=case["min_len"])
    for P, B in ((0, 0), (1, 1), (5, 40)):
        e = clip_ref.extend_clipped(read, TEXT, case["L"], S, len_s, min_len=case["min_len"], P=P, B=B)
        ops, cl, cr = e["ops"], e["clip_left"], e["clip_right"]
        assert e["n_ops"] == len(ops) and anchored_ref.query_bases(ops) == n
        mid = clip_ref.aligned_part(e)
        assert ops == b"S" * cl + mid + b"S" * cr and b"S" not in mid
        assert e["score"] == len(mid) - mid.count(b"=")
        if not base["flags"] & anchored_ref.ANCHORED:
            assert {k: v for k, v in e.items() if not k.startswith("clip_")} == base and cl == cr == 0
            continue
        assert not cl or mid[:1] == b"="
        assert not cr or mid[-1:] == b"="
        assert bool(e["flags"] & clip_ref.SOFT_LEFT) == (cl > 0) and bool(e["flags"] & clip_ref.SOFT_RIGHT) == (cr > 0)
        assert e["flags"] & ~(clip_ref.SOFT_LEFT | clip_ref.SOFT_RIGHT) == base["flags"]
        # the anchor's columns are never clipped and still sit right behind the left part
        assert ops[e["left_ops"]:e["left_ops"] + e["len"]] == b"=" * e["len"] and e["left_ops"] >= cl
        left = ops[cl:e["left_ops"]]
        assert e["loc"] == e["text_pos"] - (len(left) - left.count(b"I")) and e["off"] == e["loc"] - S and e["loc"] >= S
        assert e["loc"] + len(mid) - mid.count(b"I") <= S + len_s
        # what is kept is a piece of the unclipped alignment around the anchor
        at = base["left_ops"] - (e["left_ops"] - cl)
        assert base["ops"][at:at + len(mid)] == mid
    # P / B so large that nothing clips: the mode without the step
    e = clip_ref.extend_clipped(read, TEXT, case["L"], S, len_s, min_len=case["min_len"], P=1, B=10 ** 9)
    assert (e.pop("clip_left"), e.pop("clip_right")) == (0, 0) and e == base


def test_noise_around_a_planted_core_is_clipped_and_the_core_kept():
    """The constructed reads mismatch everywhere outside their planted run: with the defaults all of that is soft-clipped."""
    by = {c["name"]: c for c in CASES}
    c = by["longer run later beats the earlier one"]
    S, len_s = MTA[c["seq"]]
    e = clip_ref.extend_clipped(c["read"], TEXT, c["L"], S, len_s)
    r, delta, j = c["want"]
    assert (e["clip_left"], e["clip_right"]) == (j, len(c["read"]) - j - r)
    assert clip_ref.aligned_part(e) == b"=" * r and e["score"] == 0 and e["loc"] == e["text_pos"] and e["left_ops"] == j
    # an overhang past the end of the sequence comes out as 'S', not as 'I'
    c = by["right window clipped by the sequence end"]
    S, len_s = MTA[c["seq"]]
    base = anchored_ref.extend(c["read"], TEXT, c["L"], S, len_s)
    e = clip_ref.extend_clipped(c["read"], TEXT, c["L"], S, len_s)
    assert base["flags"] & anchored_ref.RIGHT_CLIPPED and e["clip_right"] > 0 and not clip_ref.aligned_part(e).endswith(b"I")


# ---------------------------------------------------------------------------------------------------------
# (c) the boundary
# ---------------------------------------------------------------------------------------------------------
def test_run_length_text_of_rows_with_soft_clips():
    from longreadmapper_amd.capi import lib
    rng = np.random.default_rng(4)
    for _ in range(200):
        n = int(rng.integers(1, 300))
        mid = b"=" + bytes(rng.choice(list(b"====XID"), size=n).astype(np.uint8)) + b"="
        cl, cr = (int(x) for x in rng.integers(0, 40, 2))
        ops = b"S" * cl + mid + b"S" * cr
        buf = C.create_string_buffer(2 * len(ops) + 16)
        ln = lib.lrm_parse_cigar(np.frombuffer(ops, dtype=np.uint8).ctypes.data, len(ops), buf, len(buf))
        text = buf.value.decode()
        assert text == sam_ref.rle(ops) == orc.parse_cigar(ops) and ln == len(text)
        assert text.startswith("%dS" % cl) == (cl > 0) and text.endswith("%dS" % cr) == (cr > 0)
        assert text.count("S") == (cl > 0) + (cr > 0)


def test_option_fields_and_the_exported_entry_point():
    from longreadmapper_amd import capi, mapper
    names = [f for f, _ in capi.MapOptions._fields_]
    at = names.index("anchor_min_len")
    assert names[at + 1:at + 4] == ["clip", "clip_penalty", "clip_end_bonus"]
    assert C.sizeof(capi.MapOptions) == 76                                    # the fields came out of the reserved words
    assert capi.MapOptions.clip.offset == 56 and capi.MapOptions.reserved.size == 8
    o = capi.map_options()
    assert (o.clip, o.clip_penalty, o.clip_end_bonus) == (0, 0, 0) and o.struct_size == 76
    assert capi.lib.lrm_extend_batch_clipped_dev is not None and capi.lib.lrm_abi_version() == 3
    assert C.sizeof(capi.Clip) == 8 == mapper.CLIP_DT.itemsize
    assert (capi.ANCHOR_SOFT_LEFT, capi.ANCHOR_SOFT_RIGHT) == (clip_ref.SOFT_LEFT, clip_ref.SOFT_RIGHT) == (32, 64)
    assert mapper._anchor_options(None, False, 0, clip=True) == dict(anchored=1, anchor_min_len=0, clip=1, clip_penalty=0,
                                                                     clip_end_bonus=0)
