"""The anchored extension mode's reference (tests/anchored_ref.py: brute-force anchor, two orc_gact-spec jobs, stitch) on
the constructed cases of tests/anchored_cases.py.  No GPU: this pins the reference the GPU tests compare against."""
import numpy as np
import pytest

import anchored_cases
import anchored_ref
import gact_ref
import orc

TEXT, MTA, CASES = anchored_cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_anchor_rule(case):
    S, len_s = MTA[case["seq"]]
    got = anchored_ref.find_anchor(case["read"], TEXT, case["L"], S, len_s, case["min_len"])
    assert got == case["want"]
    if got:                                   # the run is maximal, exact, and inside the sequence
        r, delta, j = got
        p = case["L"] + delta + j
        assert S <= p and p + r <= S + len_s
        assert bytes(case["read"][j:j + r]) == bytes(TEXT[p:p + r])
        assert j == 0 or p == S or case["read"][j - 1] != TEXT[p - 1] or case["read"][j - 1] == ord("N")
        assert j + r == len(case["read"]) or p + r == S + len_s or case["read"][j + r] != TEXT[p + r]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_jobs_and_stitch(case):
    S, len_s = MTA[case["seq"]]
    read, n = case["read"], len(case["read"])
    e = anchored_ref.extend(read, TEXT, case["L"], S, len_s, min_len=case["min_len"])
    assert anchored_ref.query_bases(e["ops"]) == n and e["n_ops"] == len(e["ops"])
    assert e["score"] == len(e["ops"]) - e["ops"].count(b"=")
    if case["want"] is None:
        assert e["flags"] == anchored_ref.FALLBACK and e["loc"] == case["L"] and e["left_ops"] == 0
        assert e["ops"] == orc.gact(bytes(read), bytes(TEXT[case["L"]:case["L"] + n]))[1]
        return
    r, delta, j = case["want"]
    p = case["L"] + delta + j
    assert (e["len"], e["delta"], e["read_pos"], e["text_pos"]) == (r, delta, j, p)
    assert bool(e["flags"] & anchored_ref.NO_LEFT) == (j == 0) and (e["left_ops"] == 0) == (j == 0)
    # the anchor's bases are '=' columns right behind the left job's ops, and POS is the text base the first column faces
    assert e["ops"][e["left_ops"]:e["left_ops"] + r] == b"=" * r
    left = e["ops"][:e["left_ops"]]
    assert e["loc"] == p - (len(left) - left.count(b"I")) and e["off"] == e["loc"] - S and e["loc"] >= S
    assert anchored_ref.query_bases(left) == j
    consumed = len(e["ops"]) - e["ops"].count(b"I")
    assert e["loc"] + consumed <= S + len_s


def test_clipped_windows_and_strands():
    by = {c["name"]: c for c in CASES}
    for name, flag in (("left window clipped by the sequence start", anchored_ref.LEFT_CLIPPED),
                       ("right window clipped by the sequence end", anchored_ref.RIGHT_CLIPPED)):
        c = by[name]
        S, len_s = MTA[c["seq"]]
        e = anchored_ref.extend(c["read"], TEXT, c["L"], S, len_s)
        assert e["flags"] & flag and e["flags"] & anchored_ref.ANCHORED
    # the left job's target is the reverse complement of the text in front of the anchor
    c = by["anchor at j = n - A: right job of exactly A bases"]
    S, len_s = MTA[c["seq"]]
    p, tr, yl, tl, flags = anchored_ref.plan(c["want"], c["L"], len(c["read"]), S, len_s)
    assert tr == 20 + 3 and tl == 280 + 35
    assert bytes(TEXT[yl:yl + tl]) == bytes(anchored_ref.revcomp(TEXT[p - tl:p]))


def test_both_aligners_agree_on_the_stitched_result():
    def second(q, d, T, O, W):
        return gact_ref.align(q, d, T, O, W)[:2]
    for c in CASES[:6]:
        S, len_s = MTA[c["seq"]]
        a = anchored_ref.extend(c["read"], TEXT, c["L"], S, len_s)
        b = anchored_ref.extend(c["read"], TEXT, c["L"], S, len_s, aligner=second)
        assert a == b


def test_deletion_rich_read_finishes_without_a_tail_of_insertions():
    """One eighth of slack in the target: a read that lost 8 % of its bases still ends in matches."""
    rng = np.random.default_rng(5)
    seq = anchored_cases.seqs()[0]
    S, len_s = MTA[0]
    src = seq[1000:3200]
    keep = np.ones(len(src), dtype=bool)
    keep[rng.choice(np.arange(100, len(src) - 50), size=len(src) * 8 // 100, replace=False)] = False
    read = src[keep]
    e = anchored_ref.extend(read, TEXT, S + 1000 + 9, S, len_s)
    assert e["flags"] & anchored_ref.ANCHORED and not e["ops"].endswith(b"I" * 8)
    classic = orc.gact(bytes(read), bytes(TEXT[S + 1009:S + 1009 + len(read)]))
    assert classic[1].endswith(b"I" * 50) and e["score"] < classic[0]
