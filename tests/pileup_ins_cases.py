"""Constructed rows and records for the insertion columns of the pileup (docs/GACT_SPEC.md, "Pileup insertions and the
polished consensus").  ROWS: (ops, read, loc, ...) as tests/pileup_cases.py builds them, at every edge of an 'I' run against
the kernel's lanes (16 columns), steps (1024), step pairs (2048) and tail loop, against the number of insertion columns
K, the read's bytes, the window and the filter.  ALLELES: a position's record and insertion words at every edge of the
allele rule.  POLISH: runs of positions for the polished sequence.  Every case carries a predicate that it reaches the edge
it is named after; tests/test_pileup_ins_cpu.py asserts them all."""
from collections import namedtuple

import numpy as np

import pileup_cases as P
from pileup_cases import Case, walk, qlen, put

LO, HI, MIN_MAPQ = P.LO, P.HI, P.MIN_MAPQ
KS = (1, 4, 8)
RUN_LENGTHS = sorted({n for K in KS for n in (1, K - 1, K, K + 1, 17, 40) if n > 0})
MAX_ROW = 3200


def runs(ops):
    """-> [(first column, length)] of the 'I' runs"""
    out, c = [], 0
    while c < len(ops):
        if ops[c] == ord("I"):
            e = c
            while e < len(ops) and ops[e] == ord("I"):
                e += 1
            out.append((c, e - c))
            c = e
        else:
            c += 1
    return out


def build_rows():
    rng = np.random.default_rng(777)
    cases = []

    def add(name, ops, reaches, read=None, loc=None, score=5, meta_r=1, mapq=60, n_ops=None, last=False, letters=b"ACGT"):
        k = len(cases)
        assert len(ops) <= MAX_ROW
        read = bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), size=qlen(ops))) if read is None else read
        loc = LO + 100 + (41 * k) % 3000 if loc is None else loc      # inside the window, every residue mod 16
        cases.append(Case(name, ops, read, loc, score, meta_r, mapq, n_ops, last, reaches))

    # run lengths either side of every K, and longer than a lane and than two
    for n in RUN_LENGTHS:
        ops = b"=" * 21 + b"I" * n + b"=" * 20
        add("run-of-%d" % n, ops, lambda ops=ops, n=n: runs(ops) == [(21, n)])
    # a run across a lane edge: columns 14 .. 17
    ops = b"=" * 14 + b"IIII" + b"=" * 30
    add("run-across-15|16", ops, lambda ops=ops: runs(ops) == [(14, 4)])
    # runs that cover whole lanes: the saturated carry.  From inside lane 0 over lanes 1 .. 3; a lane that is exactly one run;
    # a short tail of lane 0, then a whole lane, then three more columns
    ops = b"=" * 10 + b"I" * 60 + b"=" * 26
    add("run-over-lanes-1-to-3", ops, lambda ops=ops: runs(ops) == [(10, 60)] and 10 < 16 and 10 + 60 > 64)
    ops = b"=" * 16 + b"I" * 18 + b"=" * 30
    add("run-is-lane-1-and-two-more", ops, lambda ops=ops: runs(ops) == [(16, 18)])
    ops = b"=" * 12 + b"I" * 23 + b"=" * 29
    add("run-tail-4-lane-16-head-3", ops, lambda ops=ops: runs(ops) == [(12, 23)])
    ops = b"=" * 13 + b"III" + b"I" * 16 + b"=" * 32                  # lane 1 all 'I' behind a carry of 3: 19 in front of lane 2
    add("run-ends-with-lane-1", ops, lambda ops=ops: runs(ops) == [(13, 19)])
    # runs across the step edge, the step-pair edge and into the tail loop (3150 columns: one pair, one step, a rest)
    row = b"=" * 3150
    for e in (1024, 2048, 3072):
        for at, n in ((e - 4, 8), (e - 1, 2), (e - 1, 1), (e, 3), (e - 30, 60), (e - 16, 20), (e - 2, 9)):
            ops = put(row, at, b"I" * n)
            add("run-%d+%d-at-%d" % (at - e, n, e), ops, lambda ops=ops, at=at, n=n: runs(ops) == [(at, n)])
    ops = put(put(put(row, 1020, b"I" * 8), 2044, b"I" * 8), 3068, b"I" * 8)
    add("runs-across-all-three-edges", ops, lambda ops=ops: runs(ops) == [(1020, 8), (2044, 8), (3068, 8)])
    # a run that ends on the row's last column, after every kind of row end; a row that is one 'I'
    for m in (40, 1024, 2048, 2049, 3089):
        ops = b"=" * (m - 5) + b"I" * 5
        add("run-ends-the-row-%d" % m, ops, lambda ops=ops, m=m: runs(ops) == [(m - 5, 5)] and len(ops) == m)
    add("row-is-one-I", b"I", lambda: True)
    # runs with no target column before them: counted nowhere
    ops = b"III" + b"=" * 40
    add("run-at-column-0", ops, lambda ops=ops: runs(ops)[0] == (0, 3) and walk(ops)[0][0] == 0)
    ops = b"S" * 21 + b"II" + b"=" * 30
    add("run-behind-S-only", ops, lambda ops=ops: runs(ops) == [(21, 2)] and walk(ops)[21] == (0, 21))
    # a run behind a 'D': the position is the deleted one
    ops = b"=" * 9 + b"DD" + b"III" + b"=" * 9
    add("run-behind-D", ops, lambda ops=ops: runs(ops) == [(11, 3)] and ops[10] == ord("D") and walk(ops)[11][0] == 11)
    # what ends a run: 'X', 'S', 'D', '=' and a foreign byte between two runs
    for mid in (b"X", b"S", b"D", b"=", b"N", b"\x00"):
        ops = b"=" * 13 + b"II" + mid + b"III" + b"=" * 20
        add("run-cut-by-%r" % mid, ops, lambda ops=ops: runs(ops) == [(13, 2), (16, 3)])
    # the read's bytes
    ops = (b"=" * 5 + b"II") * 12 + b"=" * 5
    add("read-lower-case", ops, lambda: True, letters=b"acgt")
    add("read-N-and-others", ops, lambda: True, letters=b"NnRYacgtACGT-\x00")
    add("read-only-N", ops, lambda: True, letters=b"N")
    ops = b"=" * 20 + b"I" * 9 + b"=" * 3
    add("read-ends-inside-the-run", ops, lambda ops=ops: walk(ops)[24][1] == 24, read=b"ACGT" * 6)
    # the window
    for edge, name in ((LO, "lo"), (HI, "hi")):
        for d in (-1, 0):                                              # the run is counted at position edge + d
            ops = b"=" * 8 + b"III" + b"=" * 8
            add("run-at-%s%+d" % (name, d), ops, lambda ops=ops, edge=edge, d=d: (edge + d - 7) + walk(ops)[8][0] - 1 == edge + d, loc=edge + d - 7)
    ops = b"=" * 10 + b"II" + b"=" * 30 + b"IIIII" + b"=" * 10
    add("starts-left-of-the-window", ops, lambda ops=ops: LO - 20 + 9 < LO <= LO - 20 + 39, loc=LO - 20)
    add("starts-at-hi", ops, lambda: True, loc=HI)
    # rows without an alignment and filtered rows, between live rows
    busy = (b"=" * 3 + b"IIII") * 100
    add("live-a", busy, lambda: True)
    add("dead-meta_r-0", busy, lambda: True, meta_r=0)
    add("dead-score--1", busy, lambda: True, score=-1)
    add("dead-n_ops-0", busy, lambda: True, n_ops=0)
    add("live-shorter-than-its-store-row", busy, lambda: True, n_ops=38)    # ends inside a run
    add("mapq-below", busy, lambda: True, mapq=MIN_MAPQ - 1)
    add("mapq-at", busy, lambda: True, mapq=MIN_MAPQ)
    # rows of every op byte, many runs of every length
    for m, p in ((500, [0.5, 0.1, 0.3, 0.05, 0.05]), (2049, [0.3, 0.05, 0.6, 0.03, 0.02]), (3100, [0.55, 0.1, 0.25, 0.05, 0.05]), (3199, [0.1, 0.02, 0.85, 0.02, 0.01])):
        ops = bytes(rng.choice(P.ALPHABET, size=m, p=p))
        add("random-%d" % m, ops, lambda ops=ops: max(n for _, n in runs(ops)) >= 5, letters=b"ACGTacgtN")
    # the read buffer's last byte: a run on the read's last bases, the row placed last
    ops = b"=" * 50 + b"S" + b"=" * 10 + b"IIII"
    add("run-on-the-last-read-bytes", ops, lambda ops=ops: walk(ops)[-1][1] == qlen(ops) - 1, last=True)
    cases.sort(key=lambda c: c.last)
    return cases


ROWS = build_rows()

# ---------------------------------------------------------------------------------------------------------
# the allele rule: (name, depth, n_ins, s[K][4], opt, reaches)
# ---------------------------------------------------------------------------------------------------------
Allele = namedtuple("Allele", "name depth n_ins s opt reaches")
DEF = (8, 4, 25)


def build_alleles():
    out = []

    def add(name, depth, n_ins, s, reaches, opt=DEF):
        s = [list(r) for r in s]
        out.append(Allele(name, depth, n_ins, s, opt, lambda: reaches([sum(r) & 0xFFFFFFFF for r in s])))

    # 2 * sup == n_ins against one more, in every column of every K
    for K in KS:
        for j in range(K):
            for more in (0, 1):
                s = [[9, 0, 0, 0]] * j + [[2, 1, 1, 1 + more]] + [[9, 0, 0, 0]] * (K - j - 1)
                add("K%d-col%d-sup-%s" % (K, j, "above" if more else "on"), 20, 10, s, lambda sup, j=j, more=more: 2 * sup[j] == 10 + 2 * more)
    # 2 * n_ins == depth against one more; the depth either side of min_depth
    add("enters-on", 20, 10, [[8, 0, 0, 0]] * 4, lambda sup: 2 * 10 == 20)
    add("enters-above", 20, 11, [[8, 0, 0, 0]] * 4, lambda sup: 2 * 11 == 20 + 2)
    add("depth-below-min", 7, 7, [[0, 7, 0, 0]] * 4, lambda sup: 7 == DEF[0] - 1)
    add("depth-at-min", 8, 7, [[0, 7, 0, 0]] * 4, lambda sup: 8 == DEF[0])
    add("depth-below-min-20", 19, 15, [[0, 0, 12, 0]], lambda sup: True, opt=(20, 4, 25))
    add("depth-at-min-20", 20, 15, [[0, 0, 12, 0]], lambda sup: True, opt=(20, 4, 25))
    # every base tie: pairs, triples, all four; a later letter that is larger
    for mask in range(1, 16):
        s = [[5 if mask >> k & 1 else 2 for k in range(4)]] * 4
        add("tie-%s" % "".join("ACGT"[k] for k in range(4) if mask >> k & 1), 30, 16, s, lambda sup: True)
    add("later-letter-larger", 30, 16, [[3, 4, 5, 6]] * 4, lambda sup: True)
    add("all-words-zero", 30, 16, [[0, 0, 0, 0]] * 4, lambda sup: sup == [0] * 4)
    add("n_ins-zero", 30, 0, [[0, 0, 0, 0]] * 4, lambda sup: True)
    # len == K, and K + 1 would have passed too; a gap in the middle ends the allele
    for K in KS:
        add("K%d-full" % K, 30, 20, [[0, 0, 0, 11]] * K, lambda sup, K=K: all(2 * v > 20 for v in sup) and len(sup) == K)
    add("gap-in-column-2", 30, 20, [[11, 0, 0, 0], [11, 0, 0, 0], [10, 0, 0, 0], [11, 0, 0, 0]], lambda sup: 2 * sup[2] == 20 < 2 * sup[3])
    add("column-0-fails", 30, 20, [[10, 0, 0, 0], [11, 0, 0, 0]], lambda sup: 2 * sup[0] == 20 < 2 * sup[1])
    # products past 2^32, and a support that wraps
    big = 3_000_000_000
    add("64-bit-sup-on", 4_000_000_000, big, [[big // 2, 0, 0, 0]], lambda sup: 2 * sup[0] == big > 2**31)
    add("64-bit-sup-above", 4_000_000_000, big, [[big // 2, 1, 0, 0]], lambda sup: 2 * sup[0] == big + 2)
    add("64-bit-enters-on", 4_000_000_000, 2_000_000_000, [[2**31, 0, 0, 0]], lambda sup: 2 * 2_000_000_000 == 4_000_000_000 > 2**31)
    add("64-bit-enters-above", 4_000_000_000, 2_000_000_001, [[2**31, 0, 0, 0]], lambda sup: 2 * 2_000_000_001 == 4_000_000_002)
    add("64-bit-enters-product-past-2^32", 4_000_000_000, big, [[2**31, 0, 0, 0]], lambda sup: 2 * big > 2**32 and (2 * big) % 2**32 < 4_000_000_000)
    add("sup-wraps", 30, 16, [[2**31, 2**31, 5, 4]], lambda sup: sup[0] == 9)
    return out


ALLELES = build_alleles()

# ---------------------------------------------------------------------------------------------------------
# the polished sequence: (col, text byte, s[8][4]) per position.  col: (depth, n_eq, x_a, x_c, x_g, x_t, n_del, n_ins)
# ---------------------------------------------------------------------------------------------------------
def polish_positions():
    """-> (cols, text bytes, words (n, 8, 4), what the run is meant to hold)"""
    eq, dele = (20, 20, 0, 0, 0, 0, 0, 0), (20, 4, 0, 0, 0, 0, 16, 0)
    ins8 = [[0, 0, 12, 0]] * 8                                          # eight columns of G
    none = [[0, 0, 0, 0]] * 8
    pos = []
    pos += [(eq, "A", none)] * 3
    pos += [(dele, "C", none)]                                          # '-' next to a 9-byte position
    pos += [((20, 20, 0, 0, 0, 0, 0, 12), "T", ins8)]                   # 1 + 8 bytes
    pos += [(dele, "G", none)]
    pos += [((20, 4, 0, 0, 0, 0, 16, 12), "C", ins8)]                   # a deleted position that carries an insertion: 8 bytes
    pos += [((3, 3, 0, 0, 0, 0, 0, 0), "A", none)]                      # 'N': below min_depth
    pos += [((3, 3, 0, 0, 0, 0, 0, 3), "A", ins8)]                      # 'N' stays, and nothing enters below min_depth
    pos += [((20, 20, 0, 0, 0, 0, 0, 10), "G", ins8)]                   # 2 * n_ins == depth: the letter alone
    pos += [((20, 14, 0, 6, 0, 0, 0, 11), "a", [[6, 0, 0, 0], [0, 6, 0, 0], [0, 0, 5, 0]] + [[0, 0, 0, 0]] * 5)]    # two bases of three
    pos += [(eq, "N", none), (eq, "t", none)]
    cols = [p[0] for p in pos]
    text = "".join(p[1] for p in pos).encode()
    words = np.array([p[2] for p in pos], dtype=np.uint32)
    return cols, text, words


# options that the host entries refuse: (min_depth, min_count, min_pct, reserved)
REFUSED = [(0, 0, 101, 0), (0, 0, 0, 1)]
