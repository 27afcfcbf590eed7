"""The rival-locus rule (docs/GACT_SPEC.md, "Secondary alignments") in Python on top of mapq_ref: from the hits of a read,
its winner and its mapping-quality record to the lrm_entry the secondary extension starts from."""
import numpy as np

import mapq_ref

M64 = (1 << 64) - 1
MIN_HITS_DEFAULT, RATIO_PCT_DEFAULT = 8, 50
ZERO = (0, 0, 0)
SEC_ALIGNED, SEC_DUPLICATE = 1, 2


def candidate(n1, n2, flags, min_hits=0, ratio_pct=0):
    """best.val > 0 (n1 > 0: a read without a locus has an all-zero record), no overflow, n2 >= H, 100 n2 >= pct n1."""
    H = min_hits or MIN_HITS_DEFAULT
    pct = ratio_pct or RATIO_PCT_DEFAULT
    return bool(n1 > 0 and not (flags & mapq_ref.OVERFLOW) and n2 >= H and 100 * int(n2) >= pct * int(n1))


def sub_shift(r):
    return max(4, r - 10)


def pairs_of(keys, best, r):
    """{(bucket, h): [keys]} of the hits outside the winner's window, with Python integers."""
    out = {}
    for k in keys:
        k = int(k) & M64
        if mapq_ref.inside(k, best[0], r):
            continue
        for h in (0, 1):
            out.setdefault((mapq_ref.bucket(k, r, h), h), []).append(k)
    return out


def rival_of_hits(keys, best, length, min_hits=0, ratio_pct=0, slots=mapq_ref.SLOTS):
    """-> ((key, val, bucket) of the rival entry, record).  keys: every hit of the evidence phases.  The rule in numpy (the long
    reads of the GPU tests have hundreds of thousands of hits); rival_of_hits_scalar is the same rule hit by hit."""
    rec = mapq_ref.record_of_hits(keys, best, length, 0, slots)
    if best[1] == 0 or not candidate(rec[0], rec[1], rec[5], min_hits, ratio_pct):
        return ZERO, rec
    keys = np.asarray([k & M64 for k in keys] if isinstance(keys, list) else keys, dtype=np.uint64)
    r = mapq_ref.radius_log2(length)
    R, sh, s = np.uint64(1 << r), np.uint64(r + 1), np.uint64(sub_shift(r))
    with np.errstate(over="ignore"):
        other = keys[~((keys - np.uint64(best[0]) + R) <= np.uint64(2) * R)]
        fullest = []
        for h in (0, 1):
            ub, cnt = np.unique((other + (R if h else np.uint64(0))) >> sh, return_counts=True)
            i = int(np.argmax(cnt))                                # the first maximum: the smallest bucket (ub ascends as uint64)
            fullest.append((-int(cnt[i]), int(ub[i]), h))
        n2, b, h = min(fullest)
        v = other + (R if h else np.uint64(0))
        mine = (v >> sh) == np.uint64(b)
        off = v[mine] & (np.uint64(2) * R - np.uint64(1))
    assert -n2 == rec[1] == int(mine.sum())
    sub = (off >> s).astype(np.int64)
    idx = int(np.argmax(np.bincount(sub)))                         # the first maximum: the smallest index
    assert sub.max() < 2048
    at = sub == idx
    key = int(other[mine][at][int(np.argmin(off[at]))])
    return (key, int(at.sum()), key >> 4), rec


def rival_of_hits_scalar(keys, best, length, min_hits=0, ratio_pct=0, slots=mapq_ref.SLOTS):
    """rival_of_hits with Python integers, hit by hit."""
    rec = mapq_ref.record_of_hits(keys, best, length, 0, slots)
    n1, n2, flags = rec[0], rec[1], rec[5]
    if best[1] == 0 or not candidate(n1, n2, flags, min_hits, ratio_pct):
        return ZERO, rec
    r = mapq_ref.radius_log2(length)
    R = 1 << r
    pairs = pairs_of(keys, best, r)
    (b, h), members = min(pairs.items(), key=lambda kv: (-len(kv[1]), kv[0][0], kv[0][1]))      # fullest; then smallest bucket, h 0 first
    assert len(members) == n2
    s = sub_shift(r)
    sub = {}
    for k in members:
        off = ((k + h * R) - (b << (r + 1))) & M64
        assert 0 <= off < 2 * R
        sub.setdefault(off >> s, []).append((off, k))
    assert max(sub) < 2048
    idx, hits = min(sub.items(), key=lambda kv: (-len(kv[1]), kv[0]))
    key = min(hits)[1]
    return (key, len(hits), key >> 4), rec


def entry(oi, read, seed_len=20, thres=300, min_hits=0, ratio_pct=0, slots=mapq_ref.SLOTS):
    keys, d, best = mapq_ref.hits_of(oi, read, seed_len, thres)
    return rival_of_hits(keys, best, len(read), min_hits, ratio_pct, slots)[0]


def batch(oi, reads, lens, seed_len=20, thres=300, min_hits=0, ratio_pct=0, slots=mapq_ref.SLOTS):
    """-> (n, 3) uint64 rival entries {key, val, bucket}; all zero for a read that is not a candidate"""
    out = np.zeros((len(lens), 3), dtype=np.uint64)
    for i, n in enumerate(lens):
        out[i] = entry(oi, bytes(reads[i, :int(n)]), seed_len, thres, min_hits, ratio_pct, slots)
    return out


def plan(records, min_hits=0, ratio_pct=0):
    """The reads of the candidate table, ascending, from the lrm_mapq records."""
    return np.array([i for i, q in enumerate(records) if candidate(int(q["n1"]), int(q["n2"]), int(q["flags"]), min_hits, ratio_pct)],
                    dtype=np.uint32)
