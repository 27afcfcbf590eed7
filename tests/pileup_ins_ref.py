"""The insertion rule of the pileup (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus") as a plain column
walk: one Python loop over the op bytes of one read, a dictionary of counts; the allele and the polished sequence as loops
over positions.  Written from the rule; it shares nothing with the product (the cons letter comes from
tests/pileup_call_ref.py, the reference of the call rule)."""
import numpy as np

import pileup_call_ref as R
from pileup_ref import COL_FIELDS, aligned

BASES = b"ACGT"
ENTERS, FULL = 1, 2
M32 = 0xFFFFFFFF


def base_class(b):
    return BASES.find(bytes([b]).upper()) if bytes([b]).upper() in (b"A", b"C", b"G", b"T") else None


class InsPileup:
    """The insertion counters of a window [lo, hi) with K columns: c[pos - lo, j, k]."""

    def __init__(self, lo, hi, K):
        assert lo < hi and 1 <= K <= 8
        self.lo, self.hi, self.K = lo, hi, K
        self.c = np.zeros((hi - lo, K, 4), dtype=np.int64)
        self.col0_other = np.zeros(hi - lo, dtype=np.int64)         # column-0 bytes that are no base (or behind the read's end)

    def add(self, ops, read, loc, score=5, meta_r=1, mapq=None, min_mapq=0):
        if not aligned(ops, score, meta_r):
            return
        if mapq is not None and mapq < min_mapq:
            return
        t = q = j = 0
        for o in ops:
            ch = chr(o)
            if ch == "I":
                pos = loc + t - 1
                if t > 0 and self.lo <= pos < self.hi:
                    k = base_class(read[q]) if q < len(read) else None
                    if k is None:
                        if j == 0:
                            self.col0_other[pos - self.lo] += 1
                    elif j < self.K:
                        self.c[pos - self.lo, j, k] += 1
                j += 1
            else:
                j = 0
            t += ch in "=XD"
            q += ch in "=XIS"

    def words(self, first=0, count=None):
        """-> uint32 (count, K, 4), wrapped"""
        count = self.hi - self.lo - first if count is None else count
        return (self.c[first:first + count] & M32).astype(np.uint32)

    def planes(self):
        """the device's layout: plane 4 * j + k of W words"""
        return np.ascontiguousarray(self.words().transpose(1, 2, 0)).reshape(-1)


def allele(depth, n_ins, s, opt):
    """s: (K, 4) words -> (n_col0, len, flags, bases bytes of length len)"""
    min_depth = opt[0]
    K = len(s)
    sup = [sum(int(v) for v in s[j]) & M32 for j in range(K)]
    ln = 0
    while ln < K and 2 * sup[ln] > n_ins:
        ln += 1
    bases = bytes(BASES[max(range(4), key=lambda k: (int(s[j][k]), -k))] for j in range(ln))
    flags = (ENTERS if depth >= min_depth and 2 * n_ins > depth else 0) | (FULL if ln == K else 0)
    return sup[0] if K else 0, ln, flags, bases


def polish(cols, words, content, opt):
    """cols: records with the fields of lrm_pileup_col, words: (count, K, 4) or None, content: the text bytes -> bytes"""
    out = bytearray()
    for g in range(len(cols)):
        c = cols[g]
        col = tuple(int(c[f]) for f in COL_FIELDS)
        letter = R.call(col, content[g], opt)[3]
        if letter != ord("-"):
            out.append(letter)
        if words is not None and words.shape[1]:
            _, ln, flags, bases = allele(col[0], col[7], words[g], opt)
            if flags & ENTERS:
                out += bases
    return bytes(out)


def allele_tuple(rec):
    """a PILEUP_INS_ALLELE_DT record -> (n_col0, len, flags, bases), after checking the zero padding"""
    ln = int(rec["len"])
    assert not rec["pad"].any() and not rec["bases"][ln:].any(), rec
    return int(rec["n_col0"]), ln, int(rec["flags"]), bytes(rec["bases"][:ln])
