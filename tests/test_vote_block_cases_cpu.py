"""tests/vote_block_cases.py on the CPU: every text's suffix array is the suffix array, brute force and the oracle's trace agree
on phase 0 of every read, every case reaches the edge it is named for (its predicate: c and H on the named path, the survivor
indices and with them threads, wavefronts and chunks, the tie, the repeat hit with the smallest key and the earliest order, the
pass of every named bucket, the measured ballast bound), and every lifted read keeps the top two of the small case it was
lifted from.  The GPU file (test_gpu_vote_block.py) then holds the device to the same records."""
import numpy as np
import pytest

import constructed as K
import vote_block_cases as V

IDS = ["%s" % c for _, c in V.CASES]


def test_harness_is_the_kernels_hash():
    """csrc/vote_hash.h through the harness: a few values recorded from the harness itself (they pin the file), and the same
    arithmetic restated here."""
    buckets = [0, 1, 1000, (1 << 31) - 1, 1 << 35, (1 << 60) - 1, ((1 << 64) - 56) >> 4]
    assert V.bucket_hashes(buckets) == [0x0, 0xf2862a35, 0x5c38ffda, 0xc4ec7f28, 0xb167fe54, 0x4a6b0000, 0x84ac65b5]

    def restated(b):
        x = (b ^ (b >> 29)) & 0xFFFFFFFF
        x = x * 0x9E3779B1 & 0xFFFFFFFF
        x ^= x >> 15
        return x * 0x85EBCA6B & 0xFFFFFFFF
    rng = np.random.default_rng(5)
    more = [int(x) for x in rng.integers(0, 1 << 60, size=2000, dtype=np.uint64)] + buckets
    hs = V.bucket_hashes(more)
    assert hs == [restated(b) for b in more]
    for passes in (2, 3, 21, 164):
        assert V.bucket_passes(more, passes) == [(h >> 16) % passes for h in hs]
    assert V.bucket_passes(more, 1) == [0] * len(more)
    for counters in (1024, 4096):
        assert V.sketch_counters(more, counters) == [(h >> 5) & (counters - 1) for h in hs]


def test_path_model():
    assert [V.fast_path(c) for c in (0, 1, 192, 193, 1536, 1537)] == ["none", "fast-wave", "fast-wave", "fast-block", "fast-block", "exact"]
    assert V.exact_path(192)["tier"] == "wave" and V.exact_path(193) == dict(tier="block", passes=1, cache=False, table="lds")
    assert [V.exact_path(h)["passes"] for h in (768, 769, 1536, 1537, 16384)] == [1, 2, 2, 3, 22]
    assert [V.exact_path(h)["cache"] for h in (768, 769, 1536, 1537, 16384, 16385)] == [False, False, False, True, True, False]
    assert V.exact_path(16385)["table"] == "global" and V.exact_path(16385, (100, 512)) == dict(tier="block", passes=164, cache=False, table="lds")
    assert V.exact_path(2100, (100, 512)) == dict(tier="block", passes=21, cache=True, table="lds")
    assert [(V.thread(s), V.wave(s), V.chunk(s)) for s in (10, 100, 250, 260, 300)] == [(10, 0, 0), (100, 1, 0), (250, 3, 0), (4, 0, 1), (44, 0, 1)]


@pytest.mark.parametrize("gname", list(V.GROUPS))
def test_texts(gname):
    """(world() has checked the suffix array with check_sa and the index text against the planted sequence)"""
    w = V.world(gname)
    assert len(w["pl"].seq) <= V.MAX_TEXT
    assert bytes(w["hi"].content()) == K.index_text([w["pl"].seq])
    t = w["text"]
    assert sorted(t.reads) == sorted(t.tokens) or gname == "no-unique"
    assert all(len(r["seq"]) <= 1537 * V.P for r in t.reads.values())


@pytest.mark.parametrize("gname,cname", V.CASES, ids=IDS)
def test_predicate_holds(gname, cname):
    """(_derive has compared brute force with the oracle's trace on phase 0 and read c and H from the trace)"""
    c = V.resolve(gname, cname)
    c["predicate"]()
    for r in c["reads"]:
        assert r["c"] >= 193 and r["H"] > V.T1_LIMIT and r["top"][1][1] > 0
        assert r["trace"]["phase_recs"][0]["iter"] == 0
    assert c["limits"][1] == 512 and 60 <= c["limits"][0] <= 140


LIFTED = [(g, c) for g, c in V.CASES if g != "no-unique"]         # (that one is constructed.vote_case at scale 20, not a lifted read)


@pytest.mark.parametrize("gname,cname", LIFTED, ids=[c for _, c in LIFTED])
def test_lift_keeps_the_top_two(gname, cname):
    """The read cut behind its last locus -- the small case -- has the same top two as the lifted read: the same counts, made of
    the same loci's hits, in the same order."""
    w = V.world(gname)
    c = V.resolve(gname, cname)
    for r in c["reads"]:
        small = w["text"].small(r["name"])
        hits, rrs = V.hit_list(small["seq"], w["cen"], w["rank"])
        assert len(rrs) < r["c"] or gname in ("list",)
        assert V.top_loci(hits, small["who"]) == V.top_loci(r["hits"], w["text"].reads[r["name"]]["who"]), r["name"]


def test_cases_build_the_same_every_time():
    t1, _ = V.GROUPS["sketch"]()
    t2, _ = V.GROUPS["sketch"]()
    assert t1 is not t2 and t1.build().seq == t2.build().seq and t1.reads.keys() == t2.reads.keys()
    assert all(t1.reads[k]["seq"] == t2.reads[k]["seq"] for k in t1.reads)
    assert len(set(c for _, c in V.CASES)) == len(V.CASES)
