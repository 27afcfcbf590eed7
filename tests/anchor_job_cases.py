"""Constructed reads that pin the JOB ROWS of the anchored extension (anchor_kernels.hip, anchor_jobs: the right job is a
straight copy of read[j ..), the left job the mirrored complement of read[.. j), 16 bytes per lane with a bytewise tail) at
their edges.  tests/anchored_cases.py varies what the scan sees; here the scan's answer is fixed by construction and the
place j of the anchor varies.

    seq()      one random sequence of SEQ_LEN bases
    cases()    list of dict(name, start, n, j, strand, fwd, plain): fwd is seq[start .. start + n) with a substitution at
               every 12th base -- no exact run of it reaches 12, the shortest anchor_min_len there is -- and ONE exact run of
               RUN bases at j, closed by a substitution on either side: the anchor at the locus start is (RUN, 0, j).
               plain: the same without the run.  strand 1: the read is sequenced as revcomp(fwd)
    batch(cs, S, len_s, stride)   reads (n, stride) as sequenced, lens, best keys for a sequence at text offset S
    strides(max_len)              max_len + 1, max_len + 2, and the multiple of 16 above max_len

j (the left job's length) takes every residue mod 16, 1 .. 15 (the bytewise tail alone), 16, 17 and the AN_CHUNK edges
4095, 4096, 4097, 4111, 4112, and one 0 (no left job).  n - j (the right job's length) holds the anchor, so it cannot be
below RUN: it takes RUN .. RUN + 17 -- every residue mod 16, two or three whole 16-byte steps in front of every tail -- and
the same AN_CHUNK edges."""
import numpy as np

import anchored_ref

SEQ_LEN = 40_000
RUN = 40
PERIOD = 12
AN_CHUNK = 4096
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNK_EDGES = [AN_CHUNK - 1, AN_CHUNK, AN_CHUNK + 1, AN_CHUNK + 15, AN_CHUNK + 16]
J_VALUES = list(range(1, 18)) + CHUNK_EDGES
R_VALUES = list(range(RUN, RUN + 18)) + CHUNK_EDGES


def seq():
    return _BASES[np.random.default_rng(1201).integers(0, 4, SEQ_LEN)]


def _other(b):
    """a base other than b, for every element"""
    return _BASES[(np.searchsorted(_BASES, b) + 1) % 4]


def pairs():
    """(j, n - j): every value of either list twice, against a short and against a long partner; the chunk edges against
    each other; one read without a left job"""
    out = []
    for a, j in enumerate(J_VALUES):
        out += [(j, R_VALUES[(5 * a) % 18]), (j, R_VALUES[18 + a % 5])]
    for b, r in enumerate(R_VALUES):
        out += [(J_VALUES[(7 * b + 3) % 17], r), (J_VALUES[17 + b % 5], r)]
    out += [(0, 1000)]
    return list(dict.fromkeys(out))


def cases():
    s = seq()
    rng = np.random.default_rng(1202)
    out = []
    for k, (j, r) in enumerate(pairs()):
        n = j + r
        start = int(rng.integers(0, SEQ_LEN - n + 1))
        plain = s[start:start + n].copy()
        phase = int(rng.integers(0, PERIOD))
        plain[phase::PERIOD] = _other(plain[phase::PERIOD])
        fwd = plain.copy()
        fwd[j:j + RUN] = s[start + j:start + j + RUN]
        for e in (j - 1, j + RUN):                                    # the run ends where it was planted
            if 0 <= e < n:
                fwd[e] = _other(s[start + e])
        out.append(dict(name="j%d_r%d" % (j, r), start=start, n=n, j=j, strand=k % 2, fwd=fwd, plain=plain))
    return out


def strides(max_len):
    return (max_len + 1, max_len + 2, (max_len + 16) // 16 * 16)


def batch(cs, S, len_s, stride):
    reads = np.zeros((len(cs), stride), dtype=np.uint8)
    lens = np.array([c["n"] for c in cs], dtype=np.uint32)
    keys = np.zeros(len(cs), dtype=np.uint64)
    for i, c in enumerate(cs):
        reads[i, :c["n"]] = anchored_ref.revcomp(c["fwd"]) if c["strand"] else c["fwd"]
        keys[i] = S + 2 * len_s - (c["start"] + c["n"]) if c["strand"] else S + c["start"]
    return reads, lens, keys
