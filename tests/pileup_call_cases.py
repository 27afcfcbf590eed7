"""Constructed positions for the call rule of the pileup (docs/GACT_SPEC.md, "Pileup calls"): a record, a text byte and
options at every edge of the rule -- the depth, the count and the percentage either side of their thresholds, every tie of
`alt` and of `cons`, text bytes in lower case and outside ACGT, every combination of kinds, non-default and refused options.
Every case carries a predicate that its inputs reach the edge it is named after; tests/test_pileup_call_cpu.py asserts them
all.  A case is PLANTABLE when rows of five or six columns stacked on one position of an upper-case ACGT text give its
record (tests/test_gpu_pileup_sites.py)."""
from collections import namedtuple
from itertools import combinations

import numpy as np

BASES = "ACGT"
# col: (depth, n_eq, x_a, x_c, x_g, x_t, n_del, n_ins); other: the 'X' columns whose read byte is no base (inside depth)
Case = namedtuple("Case", "name col other byte opt reaches")
DEF = (8, 4, 25)


def rec(n_eq=0, x=None, other=0, n_del=0, n_ins=0):
    x = x or {}
    xs = [x.get(b, 0) for b in BASES]
    return (n_eq + sum(xs) + other + n_del, n_eq, *xs, n_del, n_ins)


def thresholds(opt):
    return tuple(opt.get(k, 0) or d for k, d in zip(("min_depth", "min_count", "min_pct"), DEF))


def plantable(c):
    depth, n_eq, _, _, _, _, _, n_ins = c.col
    return chr(c.byte) in BASES and depth <= 64 and n_ins <= n_eq


# what a predicate looks at: the depth, allele[A..T] (n_eq added to the text byte's own class), the deletions, the opening
# insertions, the class of the text byte (4: no base) and the three thresholds
View = namedtuple("View", "depth allele n_del n_ins rc thr")


def view(col, byte, opt):
    depth, n_eq, xa, xc, xg, xt, n_del, n_ins = col
    rc = BASES.find(chr(byte).upper()) if chr(byte).upper() in BASES else 4
    return View(depth, [x + (n_eq if k == rc else 0) for k, x in enumerate((xa, xc, xg, xt))], n_del, n_ins, rc, thresholds(opt))


def top5(v):
    """the largest of the five counts that compete for the consensus, and who holds it (0..3: bases, 4: the deletion)"""
    five = v.allele + [v.n_del]
    return max(five), [k for k in range(5) if five[k] == max(five)]


def build():
    cases = []

    def add(name, byte, reaches, opt=None, **kw):
        other = kw.get("other", 0)
        col, opt = rec(**kw), opt or {}
        v = view(col, ord(byte), opt)
        pred = (lambda: reaches(v)) if reaches.__code__.co_varnames[:1] == ("v",) else reaches
        cases.append(Case(name, col, other, ord(byte), opt, pred))

    # the depth either side of min_depth, with a count that passes the other two tests
    for kind, kw in (("snv", lambda n: dict(x={"C": n})), ("del", lambda n: dict(n_del=n)), ("ins", lambda n: dict(n_ins=n))):
        for depth in (7, 8):
            k = kw(4)
            n_eq = depth - (0 if kind == "ins" else 4)
            add("%s-depth-%d" % (kind, depth), "A", lambda depth=depth: (depth == DEF[0] - 1 or depth == DEF[0]) and 4 >= DEF[1] and 400 >= DEF[2] * depth,
                n_eq=n_eq, **k)
        # the count either side of min_count, at a depth where the percentage passes for both
        for n in (3, 4):
            k = kw(n)
            add("%s-count-%d" % (kind, n), "G" if kind == "snv" else "T", lambda n=n: n in (DEF[1] - 1, DEF[1]) and 100 * 3 >= DEF[2] * 12,
                n_eq=12 - (0 if kind == "ins" else n), **k)
        # exactly on the percentage (depth 8, count 2, 25 %) and one read below it (depth 9, count 2); min_count out of the way
        for depth in (8, 9):
            k = kw(2)
            add("%s-pct-depth-%d-count-2" % (kind, depth), "T" if kind == "snv" else "C",
                lambda depth=depth: (100 * 2 == 25 * depth) if depth == 8 else (100 * 2 < 25 * depth <= 100 * 3), opt=dict(min_count=2),
                n_eq=depth - (0 if kind == "ins" else 2), **k)
    # alt ties between every pair of bases: both above the third non-reference base; the earlier letter wins
    for a, b in combinations(BASES, 2):
        ref = next(c for c in BASES if c not in (a, b))
        third = next(c for c in BASES if c not in (a, b, ref))
        add("alt-tie-%s%s-ref-%s" % (a, b, ref), ref, lambda a=a, b=b, ref=ref: ref not in (a, b) and a < b, n_eq=8, x={a: 5, b: 5, third: 2})
    add("alt-tie-of-three", "T", lambda v: v.allele[0] == v.allele[1] == v.allele[2] > 0 and v.rc == 3, n_eq=9, x={"A": 4, "C": 4, "G": 4})
    add("alt-later-letter-larger", "A", lambda v: v.allele[3] > v.allele[1] > 0, n_eq=9, x={"C": 2, "T": 6})
    # alt with count 0
    add("alt-none-all-equal", "C", lambda v: sum(v.allele) == v.allele[v.rc] == v.depth, n_eq=15)
    add("alt-none-only-deletions", "G", lambda v: sum(v.allele) == v.allele[v.rc] and v.n_del > v.allele[v.rc], n_eq=3, n_del=9)
    add("alt-none-only-x-on-the-reference-base", "G", lambda v: sum(v.allele) == v.allele[v.rc] == v.depth, n_eq=6, x={"G": 4})
    # cons ties
    add("cons-tie-ref-A-vs-C", "A", lambda v: top5(v)[1] == [0, 1] and v.rc == 0, n_eq=5, x={"C": 5})
    add("cons-tie-ref-T-vs-A", "T", lambda v: top5(v)[1] == [0, 3] and v.rc == 3, n_eq=5, x={"A": 5})             # the reference class wins over an earlier letter
    add("cons-tie-ref-G-vs-A-and-del", "G", lambda v: top5(v)[1] == [0, 2, 4] and v.rc == 2, n_eq=4, x={"A": 4}, n_del=4)
    add("cons-tie-base-vs-base", "A", lambda v: top5(v)[1] == [1, 2] and v.rc == 0, n_eq=2, x={"C": 5, "G": 5})
    add("cons-tie-base-vs-base-later-pair", "C", lambda v: top5(v)[1] == [2, 3] and v.rc == 1, n_eq=1, x={"G": 6, "T": 6})
    add("cons-tie-base-vs-deletion", "A", lambda v: top5(v)[1] == [3, 4] and v.rc == 0, n_eq=1, x={"T": 5}, n_del=5)
    add("cons-tie-ref-vs-deletion", "C", lambda v: top5(v)[1] == [1, 4] and v.rc == 1, n_eq=5, n_del=5)
    add("cons-deletion-wins", "A", lambda v: top5(v)[1] == [4] and v.depth >= v.thr[0], n_eq=3, n_del=6)
    add("cons-base-wins-over-ref", "G", lambda v: top5(v)[1] == [3] and v.rc == 2, n_eq=3, x={"T": 7})
    add("cons-x-on-ref-base-counts-for-ref", "C", lambda v: top5(v)[1] == [1] and v.rc == 1 and v.allele[1] - 3 < v.allele[0], n_eq=3, x={"C": 2, "A": 4})   # allele[C] = 5 > 4
    add("cons-all-five-zero", "A", lambda v: top5(v)[0] == 0 and v.depth >= v.thr[0], other=9)                          # depth 9, every read shows a non-base
    add("cons-all-five-zero-with-ins", "T", lambda v: top5(v)[0] == 0 and v.depth >= v.thr[0] and v.n_ins >= v.thr[1], other=9, n_ins=5)
    add("cons-below-min-depth", "A", lambda v: v.depth == v.thr[0] - 1 and top5(v)[0] > 0, n_eq=7)
    add("cons-nothing-at-all", "C", lambda v: v.depth == 0 and top5(v)[0] == 0)
    # text bytes in lower case, and bytes that are no base (rc = other: no allele takes n_eq, every base is an alt)
    for byte, up in (("a", "A"), ("c", "C"), ("g", "G"), ("t", "T")):
        nxt = BASES[(BASES.index(up) + 1) % 4]
        add("text-lower-%s" % byte, byte, lambda byte=byte: byte.islower(), n_eq=5, x={nxt: 4})
        add("text-lower-%s-all-equal" % byte, byte, lambda byte=byte: byte.islower(), n_eq=11)
    for byte in "Nn-R\x00":
        add("text-other-%r-all-equal" % byte, byte, lambda byte=byte: byte.upper() not in BASES, n_eq=9)
        add("text-other-%r-a-base" % byte, byte, lambda byte=byte: byte.upper() not in BASES, n_eq=4, x={"A": 5})
        add("text-other-%r-tie-CT-and-del" % byte, byte, lambda byte=byte: byte.upper() not in BASES, n_eq=1, x={"C": 4, "T": 4}, n_del=4)
    # every combination of kinds
    parts = dict(S=dict(x={"G": 4}), D=dict(n_del=4), I=dict(n_ins=4))
    for r in (1, 2, 3):
        for combo in combinations("SDI", r):
            kw = dict(n_eq=8)
            for k in combo:
                kw.update(parts[k])
            add("kinds-%s" % "".join(combo), "A", lambda v, combo=combo: v.depth >= v.thr[0] and [100 * n >= v.thr[2] * v.depth and n >= v.thr[1] for n in (v.allele[2], v.n_del, v.n_ins)] == [k in combo for k in "SDI"], **kw)             # depth <= 16: 4 of 16 is 25 %
    # non-default options
    add("opt-loose-passes", "A", lambda v: v.thr == (2, 1, 1) and v.depth == 2 and v.allele[1] == 1, opt=dict(min_depth=2, min_count=1, min_pct=1), n_eq=1, x={"C": 1})
    add("opt-loose-depth-1", "A", lambda v: v.thr == (2, 1, 1) and v.depth == 1, opt=dict(min_depth=2, min_count=1, min_pct=1), x={"C": 1})
    add("opt-pct-100-all-reads", "C", lambda v: v.thr[2] == 100 and v.allele[2] == v.depth, opt=dict(min_pct=100), x={"G": 8})
    add("opt-pct-100-one-short", "C", lambda v: v.thr[2] == 100 and v.allele[2] == v.depth - 1, opt=dict(min_pct=100), n_eq=1, x={"G": 7})
    add("opt-min-depth-20-below", "T", lambda v: v.depth == 19 == v.thr[0] - 1, opt=dict(min_depth=20), n_eq=9, x={"A": 10})
    add("opt-min-depth-20-at", "T", lambda v: v.depth == 20 == v.thr[0], opt=dict(min_depth=20), n_eq=10, x={"A": 10})
    add("opt-min-count-9-below", "G", lambda v: v.n_del == 8 == v.thr[1] - 1, opt=dict(min_count=9), n_eq=8, n_del=8)
    add("opt-min-count-9-at", "G", lambda v: v.n_del == 9 == v.thr[1], opt=dict(min_count=9), n_eq=8, n_del=9)
    # counts for which the percentage needs 64 bits: 100 * n is past 2^32
    big = 4_000_000_000
    add("pct-64-bit-on-it", "A", lambda: 100 * 1_000_000_000 > 2**32 and 100 * 1_000_000_000 == 25 * big, n_eq=big - 1_000_000_000, x={"C": 1_000_000_000})
    add("pct-64-bit-one-below", "A", lambda: 100 * 999_999_999 < 25 * big, n_eq=big - 999_999_999, x={"C": 999_999_999})
    return cases


CASES = build()
# options that are refused with an error string, as (min_depth, min_count, min_pct, reserved)
REFUSED = [(0, 0, 101, 0), (0, 0, 2**32 - 1, 0), (0, 0, 0, 1), (8, 4, 25, 2**31), (1, 1, 101, 7)]


# ---------------------------------------------------------------------------------------------------------
# the end-to-end inputs: reads from a copy of the text that carries planted variants, mapped against the ORIGINAL text
# ---------------------------------------------------------------------------------------------------------
PLANT_SEED = 5
PLANT_TEXT, PLANT_READS, PLANT_READ_LEN = 200_000, 1600, 5000
_planted = {}


def planted(seed=PLANT_SEED):
    """-> dict(text, copy, snv [(pos, base)], dels [(pos, len)], ins [(pos, len)], reads, lens): 40 SNVs, 10 deletions and 10
    insertions of 1..5 bases, pairwise at least 500 positions apart and at least 6000 from either end of the 200 kbp text;
    a deletion removes text[pos .. pos + len), an insertion puts len bases behind text[pos]; 1600 ONT-profile reads of
    5 kbp from the copy: a depth of about 40."""
    if seed in _planted:
        return _planted[seed]
    from longreadmapper_amd import synth
    rng = np.random.default_rng(seed)
    text = synth.reference(PLANT_TEXT, seed=100 + seed)
    at = [6000 + 3000 * i + int(rng.integers(0, 2000)) for i in range(60)]
    assert min(b - a for a, b in zip(at, at[1:])) >= 500 and at[0] >= 6000 and at[-1] + 6000 <= PLANT_TEXT
    kinds = np.array(["S"] * 40 + ["D"] * 10 + ["I"] * 10)
    rng.shuffle(kinds)
    snv, dels, ins, pieces, done = [], [], [], [], 0
    for p, k in zip(at, kinds):
        if k == "S":
            base = int(rng.choice([b for b in b"ACGT" if b != text[p]]))
            snv.append((p, base))
            pieces += [text[done:p], np.array([base], dtype=np.uint8)]
            done = p + 1
        elif k == "D":
            ln = int(rng.integers(1, 6))
            dels.append((p, ln))
            pieces.append(text[done:p])
            done = p + ln
        else:
            ln = int(rng.integers(1, 6))
            ins.append((p, ln))
            pieces += [text[done:p + 1], rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln)]
            done = p + 1
    pieces.append(text[done:])
    copy = np.ascontiguousarray(np.concatenate(pieces))
    r = synth.reads([copy], PLANT_READS, PLANT_READ_LEN, synth.ONT, seed=200 + seed)
    _planted[seed] = dict(text=text, copy=copy, snv=snv, dels=dels, ins=ins, reads=r["reads"], lens=r["lens"])
    return _planted[seed]


def planted_conditions(w, sites, lo):
    """The three conditions on a site table (records with the fields of lrm_pileup_site) of the planted workload whose text
    starts at text position lo -> (list of what is missing, the number of sites more than 10 positions from every planted
    variant)."""
    by_pos = {int(s["pos"]) - lo: s for s in sites}
    missing = []
    for p, base in w["snv"]:
        s = by_pos.get(p)
        if s is None or not int(s["kinds"]) & 1 or int(s["alt"]) != base or int(s["cons"]) != base:
            missing.append(("snv", p, chr(base), None if s is None else (int(s["kinds"]), chr(s["alt"]), chr(s["cons"]))))
    for name, bit, planted_at in (("del", 2, w["dels"]), ("ins", 4, w["ins"])):
        for p, ln in planted_at:
            if not any(int(by_pos[q]["kinds"]) & bit for q in range(p - 10, p + 11) if q in by_pos):
                missing.append((name, p, ln))
    every = [p for p, _ in w["snv"] + w["dels"] + w["ins"]]
    away = sum(1 for q in by_pos if all(abs(q - p) > 10 for p in every))
    return missing, away
