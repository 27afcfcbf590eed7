"""Constructed positions for the variant rule of the pileup (docs/GACT_SPEC.md, "Pileup variants and VCF"): record arrays
that put the merge of deleted positions, the order of a position's records, the genotype threshold and the inserted allele at
their edges.  Every case carries a predicate over the reference's reading of it (tests/pileup_var_ref.py), so that a case
that no longer reaches its edge fails in test_cases_reach_their_edges and not silently."""
from collections import namedtuple

import numpy as np

import pileup_var_ref as V

SNV, DEL, INS = V.SNV, V.DEL, V.INS
POS0 = 1_000_003                       # the text position of a case's first record
# opt: (min_depth, min_count, min_pct, reserved, hom_pct); first, count: the range inside the rows (None: all of them)
Case = namedtuple("Case", "name rows text words opt first count reaches")
DEF = (0, 0, 0, 0, 0)


def col(depth, n_del=0, x=(0, 0, 0, 0), n_ins=0):
    """(depth, n_eq, x_a, x_c, x_g, x_t, n_del, n_ins): every read that is neither an X nor a D is an '='"""
    return (depth, depth - sum(x) - n_del, *x, n_del, n_ins)


C_ = col(20)                           # a clean position
D_ = col(20, n_del=12)                 # a deleted one under the default options
THREE = col(30, n_del=8, x=(0, 8, 0, 0), n_ins=8)      # text 'A': a DEL, an SNV to C and an INS record


def words_of(rows, K, at=None):
    """(len(rows), K, 4) insertion words, all zero except `at`: {position: [(a, c, g, t)] * K}"""
    w = np.zeros((len(rows), K, 4), dtype=np.uint32)
    for g, cols in (at or {}).items():
        w[g, :len(cols)] = cols
    return w


def kinds_lens(recs):
    return [(r[6], r[0] - POS0, r[1]) for r in recs]


def case(name, rows, reaches, text=None, words=None, opt=DEF, first=None, count=None):
    return Case(name, rows, text or b"A" * len(rows), words, opt, first, count, reaches)


CASES = [
    case("run-of-1", [C_, D_, C_], lambda r: kinds_lens(r) == [(DEL, 1, 1)]),
    case("run-at-position-0", [D_, D_, C_], lambda r: kinds_lens(r) == [(DEL, 0, 2)]),
    case("run-ends-on-the-last-position", [C_, D_, D_, D_], lambda r: kinds_lens(r) == [(DEL, 1, 3)]),
    case("all-deleted", [D_] * 5, lambda r: kinds_lens(r) == [(DEL, 0, 5)]),
    case("two-runs-one-apart", [D_, D_, C_, D_], lambda r: kinds_lens(r) == [(DEL, 0, 2), (DEL, 3, 1)]),
    # the counts fall inside the run but every position still passes (6 of 20 and 5 of 20: 25 % is enough); the record
    # carries the counts of the FIRST position
    case("counts-fall-mid-run", [col(20, n_del=18), col(20, n_del=6), col(20, n_del=5), col(20, n_del=4)],
         lambda r: kinds_lens(r) == [(DEL, 0, 3)] and r[0][2:5] == (20, 2, 18) and r[0][9] == 2),
    case("counts-rise-mid-run", [col(20, n_del=5), col(20, n_del=19)], lambda r: kinds_lens(r) == [(DEL, 0, 2)] and r[0][4] == 5 and r[0][9] == 1),
    # a position of depth min_depth - 1 is no site at all: it cuts the run in two
    case("interrupted-by-shallow-depth", [D_, col(7, n_del=7), D_], lambda r: kinds_lens(r) == [(DEL, 0, 1), (DEL, 2, 1)]),
    case("interrupted-by-shallow-depth-20", [D_, col(19, n_del=19), D_], lambda r: kinds_lens(r) == [(DEL, 0, 1), (DEL, 2, 1)], opt=(20, 0, 0, 0, 0)),
    case("range-cut-at-first", [C_, D_, D_, D_, D_, C_], lambda r: kinds_lens(r) == [(DEL, 3, 2)], first=3, count=3),
    case("range-cut-at-first+count", [C_, D_, D_, D_, D_, C_], lambda r: kinds_lens(r) == [(DEL, 1, 2)], first=0, count=3),
    case("range-cut-at-both-ends", [C_, D_, D_, D_, D_, C_], lambda r: kinds_lens(r) == [(DEL, 2, 2)], first=2, count=2),
    case("all-three-kinds", [C_, THREE, C_], lambda r: kinds_lens(r) == [(DEL, 1, 1), (SNV, 1, 1), (INS, 1, 2)] and r[1][8] == ord("C") and r[2][10] == b"GT",
         words=words_of([C_, THREE, C_], 4, {1: [(0, 0, 7, 1), (0, 0, 0, 6), (1, 1, 1, 1)]})),
    case("all-three-kinds-inside-a-run", [D_, THREE, D_], lambda r: kinds_lens(r) == [(DEL, 0, 3), (SNV, 1, 1), (INS, 1, 0)]),
    case("snv-lower-case-text", [col(20, x=(0, 0, 0, 9))], lambda r: kinds_lens(r) == [(SNV, 0, 1)] and r[0][7:9] == (ord("a"), ord("T")), text=b"a"),
    # the genotype, one count either side of the threshold
    case("gt-70-at", [col(20, n_del=14)], lambda r: r[0][9] == 2),
    case("gt-70-below", [col(20, n_del=13)], lambda r: r[0][9] == 1),
    case("gt-100-at", [col(20, n_del=20)], lambda r: r[0][9] == 2, opt=(0, 0, 0, 0, 100)),
    case("gt-100-below", [col(20, n_del=19)], lambda r: r[0][9] == 1, opt=(0, 0, 0, 0, 100)),
    case("gt-1", [col(400, n_del=4)], lambda r: r[0][9] == 2, opt=(0, 0, 1, 0, 1)),
    case("gt-50-snv-at", [col(20, x=(0, 0, 10, 0))], lambda r: r[0][6] == SNV and r[0][9] == 2, opt=(0, 0, 0, 0, 50)),
    case("gt-50-snv-below", [col(20, x=(0, 0, 9, 0))], lambda r: r[0][6] == SNV and r[0][9] == 1, opt=(0, 0, 0, 0, 50)),
    case("gt-64-bit", [col(0xF0000000, n_del=0xA8000000)], lambda r: r[0][9] == 2),            # 100 * n_alt is past 2^32
    case("gt-64-bit-below", [col(0xF0000000, n_del=0xA7FFFFFF)], lambda r: r[0][9] == 1),
    # the inserted allele
    case("ins-on-a-plain-accumulator", [col(20, n_ins=12)], lambda r: kinds_lens(r) == [(INS, 0, 0)] and r[0][5] == 0 and r[0][10:] == (b"", 0)),
    case("ins-full", [col(20, n_ins=12)], lambda r: r[0][1] == 2 and r[0][10:] == (b"CA", 3) and r[0][5] == 12,
         words=words_of([C_], 2, {0: [(1, 11, 0, 0), (9, 0, 0, 0)]})),
    case("ins-not-full", [col(20, n_ins=12)], lambda r: r[0][1] == 1 and r[0][10:] == (b"C", 1), words=words_of([C_], 2, {0: [(1, 11, 0, 0), (6, 0, 0, 0)]})),
    case("ins-minority-no-allele", [col(20, n_ins=6)], lambda r: kinds_lens(r) == [(INS, 0, 0)] and r[0][10:] == (b"", 0) and r[0][5] == 3,
         words=words_of([C_], 8, {0: [(3, 0, 0, 0)]})),
    case("ins-K-8-full", [col(20, n_ins=12)], lambda r: r[0][1] == 8 and r[0][10] == b"ACGTACGT" and r[0][11] == 3,
         words=words_of([C_], 8, {0: [tuple(12 if k == j % 4 else 0 for k in range(4)) for j in range(8)]})),
    case("nothing", [C_] * 4, lambda r: r == []),
    case("empty-range", [C_, D_], lambda r: r == [], first=1, count=0),
]

# every refused option set: (min_depth, min_count, min_pct, reserved, hom_pct, reserved3)
REFUSED = [(0, 0, 101, 0, 0, (0, 0, 0)), (0, 0, 0, 1, 0, (0, 0, 0)), (0, 0, 0, 0, 101, (0, 0, 0)), (0, 0, 0, 0, 0, (1, 0, 0)),
           (0, 0, 0, 0, 0, (0, 0, 7)), (0, 0, 0, 0, 2**32 - 1, (0, 0, 0))]


def random_records(n, K, seed):
    """n positions with deleted stretches of every length, SNVs and insertions on top -> (rows, text, words)"""
    rng = np.random.default_rng(seed)
    rows, g = [], 0
    while g < n:
        run = int(rng.integers(1, 12)) if rng.random() < 0.3 else 0
        for _ in range(min(run, n - g)):
            rows.append(("D", None))
        g += min(run, n - g)
        if g < n:
            rows.append(("C", None))
            g += 1
    out = []
    for kind, _ in rows:
        depth = int(rng.integers(5, 40))
        n_del = int(depth * rng.uniform(0.3, 1.0)) if kind == "D" else int(rng.integers(0, 3) * (rng.random() < 0.2))
        left = depth - n_del
        x = [0, 0, 0, 0]
        if rng.random() < 0.2 and left:
            x[int(rng.integers(0, 4))] = int(rng.integers(0, left + 1))
        out.append(col(depth, n_del, tuple(x), int(rng.integers(0, depth + 1)) if rng.random() < 0.25 else 0))
    text = bytes(rng.choice(np.frombuffer(b"ACGTACGTacgtNn", dtype=np.uint8), size=n))
    words = (rng.integers(0, 30, (n, K, 4)) * (rng.random((n, K, 4)) < 0.6)).astype(np.uint32) if K else None
    return out, text, words
