"""The mapping-quality rule (docs/GACT_SPEC.md, "Mapping quality") in Python on top of the oracle: the survivors of the
phases the reference's loop ran, their hits SA[row] - j, the winner's window, two staggered histograms, the formula."""
import numpy as np

M64 = (1 << 64) - 1
SLOTS = 4096
OVERFLOW = 1
REC_DT = np.dtype([("n1", "<u4"), ("n2", "<u4"), ("radius", "<u4"), ("mapq", "u1"), ("phase", "u1"), ("flags", "u1"),
                   ("_pad", "u1")])


def radius_log2(length):
    c = 0
    while (1 << c) < length:
        c += 1
    return 9 if c <= 12 else c - 3


def radius(length):
    return 1 << radius_log2(length)


def inside(key, best, r):
    """|key - best| <= R on the signed difference of the wrapped 64-bit values."""
    d = (key - best) & M64
    if d >= 1 << 63:
        d -= 1 << 64
    return -(1 << r) <= d <= (1 << r)


def bucket(key, r, h):
    return ((key + ((1 << r) if h else 0)) & M64) >> (r + 1)


def value(n1, n2):
    if n1 == 0:
        return 0
    return 60 * (n1 - min(n2, n1)) * min(n1, 10) // (10 * n1)


_SEED_DT = np.dtype([("j", "<i4"), ("_pad", "<i4"), ("rr", "<u8"), ("k", "<u8"), ("l", "<u8")])      # orc.SeedRec


def hits_of(oi, read, seed_len, thres):
    """-> (keys of every hit of the evidence phases as a uint64 array, deciding phase d, best).  What
    OracleIndex.seed_read(read, trace=True) returns -- every seed (j, rr, k, l) of the phases the loop ran, the number of
    phases, best -- read straight into numpy: the large batches of the GPU tests have millions of seeds."""
    import ctypes as C
    import orc
    assert C.sizeof(orc.SeedRec) == _SEED_DT.itemsize
    best, tr = orc.Entry(), orc.Trace()
    read = bytes(read)
    phases = orc.lib.orc_seed_read(C.byref(oi.ix), read, len(read), seed_len, thres, C.byref(best), C.byref(tr), None)
    n = int(tr.n_seeds)
    if n:
        raw = np.ctypeslib.as_array(C.cast(tr.seeds, C.POINTER(C.c_uint8)), shape=(n * _SEED_DT.itemsize,))
        seeds = raw.view(_SEED_DT).copy()
    else:
        seeds = np.zeros(0, dtype=_SEED_DT)
    orc._libc.free(C.cast(tr.seeds, C.c_void_p))
    orc._libc.free(C.cast(tr.phases, C.c_void_p))
    sv = seeds[(seeds["rr"] > 0) & (seeds["rr"] < thres)]                # the trace holds the phases 0 .. d only
    cnt = (sv["l"] - sv["k"] + 1).astype(np.int64)
    assert np.array_equal(cnt, sv["rr"].astype(np.int64))
    first = np.repeat(sv["k"].astype(np.int64), cnt)
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    keys = oi.sa()[first + within] - np.repeat(sv["j"].astype(np.int64), cnt).astype(np.uint64)      # SA[row] - j, 64-bit wrap
    return keys.astype(np.uint64), phases - 1, (int(best.key), int(best.val), int(best.bucket))


def record_of_hits(keys, best, length, d, slots=SLOTS):
    """-> (n1, n2, radius, mapq, phase, flags, distinct pairs)"""
    if best[1] == 0:
        return (0, 0, 0, 0, 0, 0, 0)
    keys = np.asarray([k & M64 for k in keys] if isinstance(keys, list) else keys, dtype=np.uint64)
    r = radius_log2(length)
    R = np.uint64(1 << r)
    with np.errstate(over="ignore"):
        win = (keys - np.uint64(best[0]) + R) <= np.uint64(2) * R          # |key - best| <= R, signed, on the wrapped values
        other = keys[~win]
        b0 = other >> np.uint64(r + 1)
        b1 = (other + R) >> np.uint64(r + 1)
    n1 = int(win.sum())
    c0 = np.unique(b0, return_counts=True)[1]
    c1 = np.unique(b1, return_counts=True)[1]
    pairs = len(c0) + len(c1)
    n2 = int(max(c0.max(), c1.max())) if pairs else 0
    flags = 0
    if pairs > slots:
        flags, n2 = OVERFLOW, n1
    return (n1, n2, 1 << r, value(n1, n2), d, flags, pairs)


def record(oi, read, seed_len=20, thres=300, slots=SLOTS):
    keys, d, best = hits_of(oi, read, seed_len, thres)
    return record_of_hits(keys, best, len(read), d, slots)


def batch(oi, reads, lens, seed_len=20, thres=300, slots=SLOTS):
    """-> (REC_DT records, distinct pairs per read)"""
    out = np.zeros(len(lens), dtype=REC_DT)
    pairs = np.zeros(len(lens), dtype=np.int64)
    for i, n in enumerate(lens):
        rec = record(oi, bytes(reads[i, :int(n)]), seed_len, thres, slots)
        out[i] = rec[:6] + (0,)
        pairs[i] = rec[6]
    return out, pairs
