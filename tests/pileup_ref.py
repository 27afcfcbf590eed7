"""The pileup rule (docs/GACT_SPEC.md, "Pileup") as a plain column walk: one Python loop over the op bytes of one read,
dictionaries of counts.  Written from the rule; it shares nothing with the product."""
import numpy as np

COL_FIELDS = ("depth", "n_eq", "x_a", "x_c", "x_g", "x_t", "n_del", "n_ins")
CLASS_OF = {ord("A"): "x_a", ord("a"): "x_a", ord("C"): "x_c", ord("c"): "x_c", ord("G"): "x_g", ord("g"): "x_g",
            ord("T"): "x_t", ord("t"): "x_t"}


def aligned(ops, score, meta_r):
    return len(ops) > 0 and meta_r != 0 and score != -1


class Pileup:
    """The counters of a window [lo, hi): depth, the five 'X' classes, del and ins per position."""

    def __init__(self, lo, hi):
        assert lo < hi
        self.lo, self.hi = lo, hi
        self.c = {name: np.zeros(hi - lo, dtype=np.int64) for name in ("depth", "x_a", "x_c", "x_g", "x_t", "x_other", "n_del", "n_ins")}

    def _count(self, name, pos):
        if self.lo <= pos < self.hi:
            self.c[name][pos - self.lo] += 1

    def add(self, ops, read, loc, score=5, meta_r=1, mapq=None, min_mapq=0):
        """One read: its op bytes, its bases in the orientation of the ops, meta.loc."""
        if not aligned(ops, score, meta_r):
            return
        if mapq is not None and mapq < min_mapq:
            return
        t = q = 0
        before = None
        for o in ops:
            ch = chr(o)
            if ch == "X":
                b = read[q] if q < len(read) else 0
                self._count(CLASS_OF.get(b, "x_other"), loc + t)
            elif ch == "D":
                self._count("n_del", loc + t)
            elif ch == "I" and before != "I" and t > 0:
                self._count("n_ins", loc + t - 1)
            if ch in "=XD":
                self._count("depth", loc + t)
                t += 1
            if ch in "=XIS":
                q += 1
            before = ch

    def columns(self, first=0, count=None):
        """-> a record array with COL_FIELDS (uint32, wrapped) of positions lo + first .. lo + first + count - 1"""
        count = self.hi - self.lo - first if count is None else count
        out = np.zeros(count, dtype=[(f, "<u4") for f in COL_FIELDS])
        s = slice(first, first + count)
        c = self.c
        x_all = c["x_a"] + c["x_c"] + c["x_g"] + c["x_t"] + c["x_other"]
        out["depth"] = c["depth"][s] & 0xFFFFFFFF
        out["n_eq"] = (c["depth"] - x_all - c["n_del"])[s] & 0xFFFFFFFF
        for f in ("x_a", "x_c", "x_g", "x_t", "n_del", "n_ins"):
            out[f] = c[f][s] & 0xFFFFFFFF
        return out

    def other(self, first=0, count=None):
        count = self.hi - self.lo - first if count is None else count
        return self.c["x_other"][first:first + count].copy()


def same(got, want):
    """got: records with the fields of lrm_pileup_col (any dtype layout); want: columns() -> bool, field by field"""
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]).astype(np.int64), want[f].astype(np.int64)) for f in COL_FIELDS)


def first_difference(got, want):
    for f in COL_FIELDS:
        bad = np.flatnonzero(np.asarray(got[f]).astype(np.int64) != want[f].astype(np.int64))
        if len(bad):
            return f, int(bad[0]), int(got[f][bad[0]]), int(want[f][bad[0]])
    return None
