"""Constructed cases of the anchored extension mode: a three-sequence text with both strands, and (read, sequence, locus)
triples whose anchor is known by construction.  Shared by the CPU tests (tests/anchored_ref.py alone) and the GPU tests
(lrm_debug_anchor and the batch calls against it)."""
import numpy as np

import constructed

SEG = 2048                  # bases per segment of the scan kernel (AN_SEG_WORDS * 32 in anchor_kernels.hip)
A = 20                      # default shortest anchor
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def seqs(seed=7):
    rng = np.random.default_rng(seed)
    return [_BASES[rng.integers(0, 4, n)] for n in (9000, 5000, 700)]


def text_of(ss):
    """-> (text as uint8 array, [(S, len_s)])"""
    text = np.frombuffer(constructed.index_text([bytes(s) for s in ss]), dtype=np.uint8)
    mta, off = [], 0
    for s in ss:
        mta.append((off, len(s)))
        off += 2 * len(s)
    return text, mta


def noise(rng, n, avoid):
    """n bases that differ from `avoid` (same length) everywhere: no accidental match on the planted diagonal."""
    r = _BASES[rng.integers(0, 4, n)]
    clash = r == avoid
    r[clash] = _BASES[(np.searchsorted(_BASES, r[clash]) + 1) % 4]
    return r


def planted(rng, seq, S, start, n, runs, delta=0, loc_shift=0):
    """A read of n bases whose base k faces seq[start + k]: mismatching everywhere except inside runs = [(j, r), ...].
    The voted locus is S + start - delta + loc_shift... i.e. the planted diagonal sits `delta` off the locus.
    -> (read, L)"""
    lo, hi = max(0, -start), min(n, len(seq) - start)
    face = np.full(n, ord("A"), dtype=np.uint8)
    face[lo:hi] = seq[start + lo:start + hi]
    read = noise(rng, n, face)
    for j, r in runs:
        read[j:j + r] = face[j:j + r]
    return read, S + start - delta


def cases(seed=3):
    """-> text, mta, [dict(name, read, seq, L, min_len, want=(r, delta, j) or None)]"""
    rng = np.random.default_rng(seed)
    ss = seqs()
    text, mta = text_of(ss)
    out = []

    def add(name, seq, start, n, runs, delta=0, want="first", min_len=0, edit=None):
        read, L = planted(rng, ss[seq], mta[seq][0], start, n, runs, delta)
        if edit:
            edit(read)
        if want == "first":
            want = (runs[0][1], delta, runs[0][0])
        out.append(dict(name=name, read=read, seq=seq, L=L, min_len=min_len, want=want))

    add("anchor at j = 0: no left job", 0, 1000, 300, [(0, 40)])
    add("anchor at j = n - A: right job of exactly A bases", 0, 1000, 300, [(280, A)])
    add("run of A - 1: unanchored", 0, 1000, 300, [(100, A - 1)], want=None)
    add("min_len 12 finds the run of 19", 0, 1000, 300, [(100, A - 1)], min_len=12)
    add("tie: equal runs on one diagonal, the smaller j wins", 0, 2000, 400, [(50, 30), (200, 30)])
    add("longer run later beats the earlier one", 0, 2000, 400, [(50, 30), (200, 31)], want=(31, 0, 200))
    add("delta = -32 found", 0, 3000, 200, [(60, 25)], delta=-32)
    add("delta = 31 found", 0, 3000, 200, [(60, 25)], delta=31)
    add("delta = -33 not found", 0, 3000, 200, [(60, 25)], delta=-33, want=None)
    add("delta = 32 not found", 0, 3000, 200, [(60, 25)], delta=32, want=None)
    for k in (-1, 0, 1):                                   # runs around a segment boundary of the scan
        add("run ends at the segment boundary %+d" % k, 0, 500, 2 * SEG + 300, [(SEG + k - 40, 40)])
        add("run starts at the segment boundary %+d" % k, 0, 500, 2 * SEG + 300, [(SEG + k, 40)])
        add("read length = segment %+d, run to the last base" % k, 0, 500, SEG + k, [(SEG + k - 33, 33)])
    add("run crosses a segment boundary", 0, 500, 2 * SEG + 300, [(SEG - 17, 50)])
    add("run crosses two segment boundaries", 0, 200, 3 * SEG + 100, [(SEG - 5, SEG + 30)])
    add("run inside one 32-base word", 0, 4000, 200, [(65, 24)])
    add("run of exactly 64 on word boundaries", 0, 4000, 300, [(64, 64)])

    def with_n(read):
        read[120] = ord("N")
    add("an N inside a run splits it", 0, 1000, 300, [(100, 50)], want=(29, 0, 121), edit=with_n)
    add("run touching the first base of a sequence and of the text", 0, 0, 200, [(0, 30)])
    add("run touching the last base of a sequence", 0, 9000 - 200, 200, [(170, 30)])
    add("run touching the last base of the last sequence", 2, 700 - 200, 200, [(170, 30)])
    add("left window clipped by the sequence start", 1, 10, 400, [(200, 30)], delta=5)
    add("right window clipped by the sequence end", 1, 5000 - 420, 400, [(100, 30)], delta=-5)
    add("read hangs over the sequence start: bases outside never match", 1, -15, 200, [(15, 40)], delta=-3)

    # two diagonals, equal runs: |delta| decides, then the sign
    def two_diagonals(name, d1, d2, want_delta):
        seq, start, n, r = 0, 6000, 400, 30
        read, L = planted(rng, ss[seq], mta[seq][0], start, n, [(50, r)], 0)
        x = d2 - d1
        read[250:250 + r] = ss[seq][start + 250 + x:start + 250 + x + r]
        for k in (249, 250 + r):                              # flanks that match on neither diagonal
            read[k] = next(b for b in _BASES if b != ss[seq][start + k] and b != ss[seq][start + k + x])
        j = 50 if want_delta == d1 else 250
        out.append(dict(name=name, read=read, seq=seq, L=L - d1, min_len=0, want=(r, want_delta, j)))
    two_diagonals("tie: the smaller |delta| wins", -7, 3, 3)
    two_diagonals("tie: equal |delta|, the negative delta wins", 4, -4, -4)
    return text, mta, out
