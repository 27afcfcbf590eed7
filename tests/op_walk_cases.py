"""Constructed rows for the walk the stream kernels over op bytes share (op_rows.h: alignment summary, difference events,
pileup): rows of more than two step pairs, so that the second turn of the pair loop, the carry from one pair into the next
and the step from the last pair into the tail are reached.  Columns 2048 (a pair edge), 3072 (a step edge inside the second
pair) and 4096 (in a row of 4097 columns: the edge between the last pair and the tail) carry the runs.  The cases are
pileup_cases.Case tuples; every one carries a predicate that it reaches the edge it is named after
(tests/test_op_walk_cpu.py asserts them all)."""
import numpy as np

import pileup_cases as K
from pileup_cases import Case, put

LO, HI = 20000, 32000              # the pileup window: every row lies inside it
LENGTHS = (4095, 4096, 4097, 6145)
EDGES = (2048, 3072, 4096)
ROW = 4097                         # the rows the runs are put into: two pairs and a tail of one column


def base_row(m):
    return ((b"=" * 7 + b"X") * (m // 8 + 1))[:m]


def steps_of(m):
    """-> (turns of the pair loop, tail steps) of a row of m columns"""
    pairs = m // 2048
    return pairs, -(-(m - 2048 * pairs) // 1024)


def build():
    rng = np.random.default_rng(4097)
    cases = []

    def add(name, ops, reaches, score=5, meta_r=1, n_ops=None):
        k = len(cases)
        cases.append(Case(name, ops, K._read_for(ops, rng), LO + 100 + (37 * k) % 4500, score, meta_r, 60, n_ops, False, reaches))

    for m in LENGTHS:
        add("base-%d" % m, base_row(m), lambda m=m: steps_of(m)[0] >= 1 and steps_of(m) == {4095: (1, 2), 4096: (2, 0), 4097: (2, 1), 6145: (3, 1)}[m])
        ops = bytes(rng.choice(K.ALPHABET, size=m))
        add("random-%d" % m, ops, lambda ops=ops, m=m: len(ops) == m and set(ops) == set(b"=XIDS"))
    base = base_row(ROW)
    assert steps_of(ROW) == (2, 1)
    for e in EDGES:
        for kind in b"XDI":
            for at, ln, rel in ((e - 3, 3, "ends-on"), (e, 3, "starts-on"), (e - 2, 4, "straddles")):
                ln = min(ln, ROW - at)                                   # (the tail of these rows is column 4096 alone)
                ops = put(put(base, at - 1, b"="), at, bytes([kind]) * ln)
                if at + ln < len(ops):
                    ops = put(ops, at + ln, b"=")

                def reaches(ops=ops, kind=kind, at=at, ln=ln, e=e, rel=rel):
                    run = ops[at:at + ln] == bytes([kind]) * ln and ops[at - 1] != kind and (at + ln == len(ops) or ops[at + ln] != kind)
                    return run and {"ends-on": at + ln == e, "starts-on": at == e, "straddles": at < e < at + ln}[rel]
                add("%s-run-%s-%d" % (chr(kind), rel, e), ops, reaches)
        for piece in (b"DI", b"ID", b"DN", b"NI"):                       # the second byte sits on the edge
            ops = put(base, e - 1, piece[:ROW - (e - 1)])
            add("%s-across-%d" % (piece.decode(), e), ops,
                lambda ops=ops, piece=piece, e=e: ops[e - 1:e + 1] == piece and len(ops) > e)
    # a long run over the first column of a third pair
    long_base = base_row(6145)
    for kind in b"XDI":
        ops = put(long_base, 4096 - 17, b"=" + bytes([kind]) * 34 + b"=")
        add("%s-run-over-the-third-pair-edge" % chr(kind), ops,
            lambda ops=ops, kind=kind: ops[4080:4114] == bytes([kind]) * 34 and ops[4079] != kind != ops[4114] and steps_of(len(ops))[0] == 3)
    for c in b"=XIDS":
        ops = bytes([c]) * ROW
        add("only-%s-%d" % (chr(c), ROW), ops, lambda ops=ops, c=c: len(ops) == ROW and set(ops) == {c})
    # among live rows: a row whose store row goes on behind n_ops, and a row without an alignment
    live = bytes(rng.choice(K.ALPHABET, size=6145))
    add("live-a", live, lambda: True)
    add("n_ops-4097-of-6145-stored", live, lambda live=live: len(live) > 4097 and set(live[4097:]) == set(b"=XIDS"), n_ops=4097)
    add("dead-meta_r-0", b"D" * ROW, lambda: True, meta_r=0)
    add("live-b", live[:4096], lambda: True)
    return cases


CASES = build()
