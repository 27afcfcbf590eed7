"""Stage mix: one batch on which every stage of the mapper has work at once -- mapping quality, the clipped extension, split,
secondary, summary, difference events, pileup -- and the references of all of them, so that a mapper with every stage on
can be compared with the mappers that run one stage each (tests/test_gpu_stage_mix.py; the premises, on the references
alone: tests/test_stage_mix_cpu.py).

    world()        the text (the planted two-copy repeat of tests/test_gpu_secondary.py: 120 kbp, [A0, A0 + LN) copied to
                   [B0, B0 + LN), cut into two sequences so that the second copy lies in sequence 1), ~200 reads of at most
                   3 kbp in five classes, shuffled
    references()   tests/hostile_buffers.py references() over them (seed, MAPQ, rival, the extensions, the split table and rows,
                   the secondary table and rows), and beside them the summary records, the difference events and the pileup
    every_third()  the second, smaller batch of the "used mapper" test

The classes:
    a   plain reads in unique text (four of them with a long insertion: candidates whose secondary is a duplicate)
    b   reads wholly inside a copy: secondary candidates
    c   chimeras of a piece inside a copy and a piece of >= 400 bases of unique text, in both orders: a secondary candidate
        with a clipped end of at least split_min_len
    d   three-part chimeras whose middle part wins (every other middle lies inside a copy): two segments from one read
    e   junk, and reads of 1, 19 and 37 bases: no locus (best is the zero entry), no segment, never a candidate
"""
import numpy as np

import aln_summary_ref
import anchored_ref
import hostile_buffers as H
import md_ref
import pileup_ref
from longreadmapper_amd import index, synth

A0, B0, LN = 20_000, 80_000, 12_000
TEXT, CUT = 120_000, 60_000                   # sequence 0: [0, CUT), sequence 1: [CUT, TEXT)
MAX_LEN = 3000
HLEN, SMALL = 10, dict(lc_long_max=13)
CLASSES = "abcde"
_cache = {}


def _unique(pos, span):
    """[pos, pos + span) of the uncut text touches neither copy"""
    end = pos + span
    return (end <= A0 or pos >= A0 + LN) and (end <= B0 or pos >= B0 + LN)


class _Pieces:
    """Read pieces of a length drawn with synth.reads on both strands: inside a copy, or in unique text."""

    def __init__(self, seqs, base):
        self.seqs, self.copy, self.sets, self.seed = seqs, [base[A0:A0 + LN].copy()], {}, 100

    def take(self, where, length):
        """-> (bases, strand) of the next unused piece of that kind"""
        key = (where, length)
        if key not in self.sets:
            self.seed += 1
            r = synth.reads(self.copy if where == "copy" else self.seqs, 400 if where == "unique" else 120, length, synth.ONT,
                            seed=self.seed)
            ok = [i for i in range(len(r["lens"])) if where == "copy" or
                  _unique(int(r["pos"][i]) + CUT * int(r["seq"][i]), int(r["span"][i]))]
            self.sets[key] = [r, ok, 0]
        r, ok, at = self.sets[key]
        self.sets[key][2] += 1
        i = ok[at]
        return r["reads"][i, :int(r["lens"][i])].copy(), int(r["strand"][i])


def world():
    """-> dict(seqs, hi, n, reads (n, MAX_LEN + 1) uint8, lens, cls [class letter per read], parts [per read: (where, strand) of
    its pieces in read order], con_len)"""
    if "world" in _cache:
        return _cache["world"]
    base = synth.reference(TEXT, seed=61).copy()
    base[B0:B0 + LN] = base[A0:A0 + LN]
    seqs = [base[:CUT].copy(), base[CUT:].copy()]
    hi = index.HostIndex.build(seqs, names=["chrP", "chrQ"], hlen=HLEN)
    rng = np.random.default_rng(2025)
    px = _Pieces(seqs, base)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    junk = lambda k: (acgt[rng.integers(0, 4, k)], None)
    made = []                                                 # (class, [(where, (bases, strand))])

    def add(cls, *parts):
        made.append((cls, [(w, px.take(w, ln) if w != "junk" else junk(ln)) for w, ln in parts]))

    for k in range(66):
        add("a", ("unique", (3000, 2000, 1000, 640, 2500, 1500)[k % 6]))
    # ... four of them with 700 foreign bases in the middle: the second half's hits lie outside the winner's window, its
    # extension lands within half a read of the primary's -- a candidate that is flagged a duplicate
    for k in range(4):
        src = bytes(seqs[1]) if k % 2 == 0 else bytes(anchored_ref.revcomp(seqs[1]))
        at = 40_000 + 3_000 * k                                # (either strand: [40 k, 52 k) of the oriented sequence is unique text)
        left, used = H._noisy(rng, src, at, 1000, *H.ONT)
        right, _ = H._noisy(rng, src, at + used, 1000, *H.ONT)
        rd = np.frombuffer(left + bytes(junk(700)[0]) + right, dtype=np.uint8)
        made.append(("a", [("unique-ins", (rd, k % 2))]))
    for k in range(40):
        add("b", ("copy", (3000, 1500, 2200, 900)[k % 4]))
    for k in range(48):                                       # copy piece first, or last; both pieces on either strand
        cp, un = ("copy", (1900, 1600)[k % 2]), ("unique", (800, 450, 1000)[k % 3])
        add("c", *((cp, un) if k % 4 < 2 else (un, cp)))
    for k in range(24):
        add("d", ("unique", (450, 600)[k % 2]), ("copy" if k % 2 == 0 else "unique", 1800), ("unique", (500, 420)[k // 2 % 2]))
    for ln in (1, 19, 37, 600, 2100, 3000, 37, 19, 1, 1300):
        add("e", ("junk", ln))

    order = rng.permutation(len(made))
    n = len(made)
    reads = np.zeros((n, MAX_LEN + 1), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    cls, parts = [], []
    for row, i in enumerate(order):
        c, ps = made[i]
        rd = np.concatenate([p[0] for _, p in ps])[:MAX_LEN]
        reads[row, :len(rd)], lens[row] = rd, len(rd)
        cls.append(c)
        parts.append([(w, p[1]) for w, p in ps])
    w = dict(seqs=seqs, hi=hi, n=n, reads=reads, lens=lens, cls=np.array(cls), parts=parts, con_len=int(hi.h.con_len))
    _cache["world"] = w
    return w


def extras_of(ext, oriented, lens, content, window):
    """What the stages behind the extension make of an extension_ref result: the summary records (list of dicts of
    aln_summary_ref.FIELDS), the event offsets (n + 1) and words, and the pileup_ref.Pileup over the window"""
    n = len(lens)
    summary, off, events = [], [0], []
    pile = pileup_ref.Pileup(*window)
    for i in range(n):
        ops, score, meta_r, loc = ext["ops"][i], int(ext["score"][i]), int(ext["meta_r"][i]), int(ext["loc"][i])
        summary.append(aln_summary_ref.record(ops, score, meta_r))
        events += md_ref.events(ops, content, loc, score, meta_r)
        off.append(len(events))
        pile.add(ops, bytes(oriented[i, :lens[i]]), loc, score, meta_r)
    return dict(summary=summary, diff_off=np.array(off, dtype=np.uint64), diff_events=np.array(events, dtype=np.uint32), pileup=pile)


def references(rows=None, lens=None):
    """hostile_buffers.references over the world's reads (or over other rows of it) in the clipped mode, plus extras_of the
    primary's extension over the whole text; the world's own are computed once and must be left unchanged"""
    w = world()
    own = rows is None
    if own and "ref" in _cache:
        return _cache["ref"]
    rows, lens = (w["reads"].copy(), w["lens"]) if own else (rows.copy(), lens)
    ref = H.references(dict(hi=w["hi"]), rows, lens, modes=("clipped",))
    ref.update(extras_of(ref["clipped"], ref["oriented"], lens, bytes(w["hi"].content()), (0, w["con_len"])))
    if own:
        _cache["ref"] = ref
    return ref


def every_third():
    """-> (rows, lens, the indices) of the second batch: every third read of the world"""
    w = world()
    pick = np.arange(0, w["n"], 3)
    return w["reads"][pick].copy(), w["lens"][pick].copy(), pick
