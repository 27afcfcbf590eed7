"""Constructed rows for the pileup (docs/GACT_SPEC.md, "Pileup"): (ops, read, loc, score, meta_r, mapq[, n_ops]) at every
edge of the kernel's lanes (16 columns), steps (1024) and step pairs (2048), of the window and of the filter.  Every case
carries a predicate that it reaches the edge it is named after; tests/test_pileup_cpu.py asserts them all."""
from collections import namedtuple

import numpy as np

LO, HI = 5000, 12000               # the window of the constructed cases: 7000 positions, more than three read-back tiles
MIN_MAPQ = 7
N_OPS = [0, 1, 15, 16, 17, 63, 64, 1023, 1024, 1025, 2049]
EDGES = (16, 1024, 2048)
ALPHABET = np.frombuffer(b"=XIDS", dtype=np.uint8)
KNOWN = set(b"=XIDS")

# n_ops: None = len(ops); otherwise what the n_ops array says while the store row holds all of ops.  last: the row goes to
# the end of the batch and its read ends on the last byte of the read buffer.
Case = namedtuple("Case", "name ops read loc score meta_r mapq n_ops last reaches")


def walk(ops):
    """-> [(t, q)] before every column"""
    out, t, q = [], 0, 0
    for o in ops:
        out.append((t, q))
        t += o in b"=XD"
        q += o in b"=XIS"
    return out


def span(ops):
    return sum(ops.count(c) for c in b"=XD")


def qlen(ops):
    return sum(ops.count(c) for c in b"=XIS")


def put(row, at, piece):
    assert 0 <= at and at + len(piece) <= len(row)
    return row[:at] + piece + row[at + len(piece):]


def _read_for(ops, rng, letters=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), size=qlen(ops)))


def effective_ops(c):
    return c.ops if c.n_ops is None else c.ops[:max(c.n_ops, 0)]


def build():
    rng = np.random.default_rng(20240)
    cases = []

    def add(name, ops, reaches, read=None, loc=None, score=5, meta_r=1, mapq=60, n_ops=None, last=False):
        k = len(cases)
        read = _read_for(ops, rng) if read is None else read
        loc = LO + 100 + (37 * k) % 4500 if loc is None else loc   # inside the window, every residue mod 16
        cases.append(Case(name, ops, read, loc, score, meta_r, mapq, n_ops, last, reaches))

    # lengths either side of a lane, a step and a step pair; rows of a single kind
    for m in N_OPS:
        for tag, p in (("mostly-eq", [0.6, 0.1, 0.1, 0.1, 0.1]), ("uniform", None)):
            ops = bytes(rng.choice(ALPHABET, size=m, p=p))
            add("n_ops-%d-%s" % (m, tag), ops, lambda ops=ops, m=m: len(ops) == m)
        for c in b"=XIDS":
            ops = bytes([c]) * m
            add("only-%s-%d" % (chr(c), m), ops, lambda ops=ops, c=c, m=m: len(ops) == m and set(ops) <= {c})
    base = ((b"=" * 7 + b"X") * 257)[:2049]
    # runs that end on, start on and straddle a lane edge, a step edge and a step-pair edge
    for e in EDGES:
        for kind in b"XDI":
            for at, ln, rel in ((e - 3, 3, "ends-on"), (e, 3, "starts-on"), (e - 2, 4, "straddles"), (e - 17, 34, "straddles-long"),
                                (e - 1, 1, "last-before"), (e, 1, "first-behind")):
                if at < 0 or at + ln > len(base):
                    continue
                ops = put(put(base, max(at - 1, 0), b"="), at, bytes([kind]) * ln)
                if at + ln < len(ops):
                    ops = put(ops, at + ln, b"=")

                def reaches(ops=ops, kind=kind, at=at, ln=ln, e=e, rel=rel):
                    run = ops[at:at + ln] == bytes([kind]) * ln and (at == 0 or ops[at - 1] != kind) and (at + ln == len(ops) or ops[at + ln] != kind)
                    where = {"ends-on": at + ln == e, "starts-on": at == e, "straddles": at < e < at + ln, "straddles-long": at < e - 16 and e + 16 < at + ln,
                             "last-before": at + ln == e, "first-behind": at == e}[rel]
                    return run and where
                add("%s-run-%s-%d" % (chr(kind), rel, e), ops, reaches)
        for piece in (b"DI", b"ID", b"IXI", b"ISI", b"DDII", b"IIDD"):
            for at in range(e - len(piece), e + 1):
                if at < 0 or at + len(piece) > len(base):
                    continue
                ops = put(base, at, piece)
                add("%s-at-%d-across-%d" % (piece.decode(), at, e), ops,
                    lambda ops=ops, piece=piece, at=at, e=e: ops[at:at + len(piece)] == piece and at <= e <= at + len(piece))
    # 'I' runs with no target column before them: counted nowhere
    ops = b"III" + b"=" * 40 + b"I" + b"=" * 9
    add("I-run-at-column-0", ops, lambda ops=ops: ops[0] == ord("I") and walk(ops)[0][0] == 0)
    ops = b"S" * 21 + b"II" + b"=" * 30 + b"XDI="
    add("I-run-behind-leading-S", ops, lambda ops=ops: ops[21] == ord("I") and ops[20] == ord("S") and walk(ops)[21] == (0, 21))
    # an 'X' as its lane's first and 16th column, q shifted off t by 'I' / 'S' columns in front of it
    for col in (16, 31, 1024 + 16, 1024 + 31, 2048):
        ops = put(put(b"=" * 2100, 0, b"SSSSS"), 9, b"III")
        ops = put(ops, col, b"X")
        add("X-lane-column-%d" % col, ops,
            lambda ops=ops, col=col: ops[col] == ord("X") and col % 16 in (0, 15) and walk(ops)[col][1] == walk(ops)[col][0] + 8)
    # sixteen 'X' in one lane behind an 'I': the lane's 16 query bytes start off a 16-byte boundary
    ops = b"=" * 15 + b"I" + b"X" * 16 + b"=" * 20
    add("X-whole-lane", ops, lambda ops=ops: ops[16:32] == b"X" * 16 and walk(ops)[16] == (15, 16))
    # a foreign byte between runs: it advances neither count and it ends an 'I' run
    ops = b"=" * 10 + b"DDNDD" + b"=" * 5 + b"IINII" + b"=" * 5 + b"XNX" + b"=" * 12 + b"\x00=" + b"I\xffI="
    add("foreign-bytes", ops, lambda ops=ops: not set(ops) <= KNOWN and ops.count(b"INI") == 1 and ops.count(b"DND") == 1)
    # read bytes lower case, and N
    ops = (b"=X" * 40) + b"IX" * 5
    add("read-lower-case", ops, lambda: True, read=_read_for(ops, rng, b"acgt"))
    add("read-N-and-others", ops, lambda: True, read=_read_for(ops, rng, b"NnRYacgtACGT-\x00"))
    # a read shorter than its ops ask for: the bytes behind its end count as `other`, and are never read
    add("read-shorter-than-its-ops", b"=" * 20 + b"X" * 20, lambda: True, read=b"ACGT" * 6)
    # the window's edges
    ops = b"=" * 30 + b"X" + b"=" * 9
    add("ends-exactly-at-lo", ops, lambda ops=ops: (LO - 40) + span(ops) == LO, loc=LO - 40)
    add("starts-exactly-at-hi", ops, lambda: True, loc=HI)
    add("straddles-lo", ops, lambda ops=ops: LO - 20 < LO < LO - 20 + span(ops), loc=LO - 20)
    add("straddles-hi", ops, lambda ops=ops: HI - 20 < HI < HI - 20 + span(ops), loc=HI - 20)
    add("ends-exactly-at-hi", ops, lambda ops=ops: HI - 40 + span(ops) == HI, loc=HI - 40)
    add("starts-exactly-at-lo", ops, lambda: True, loc=LO)
    ops = bytes(rng.choice(ALPHABET, size=HI - LO + 900, p=[0.8, 0.06, 0.02, 0.1, 0.02]))
    add("straddles-both", ops, lambda ops=ops: LO - 200 + span(ops) > HI, loc=LO - 200)
    for kind in b"XD":
        for edge, name in ((LO, "lo"), (HI, "hi")):
            ops = b"=" * 8 + bytes([kind]) * 2 + b"=" * 8                  # the two columns at edge - 1 and at edge
            add("%s-at-%s-1-and-%s" % (chr(kind), name, name), ops,
                lambda ops=ops, kind=kind, edge=edge: [edge - 9 + walk(ops)[c][0] for c in (8, 9)] == [edge - 1, edge] and ops[8] == kind == ops[9],
                loc=edge - 9)
    for edge, name in ((LO, "lo"), (HI, "hi")):
        for d in (-1, 0):                                                   # the run opens behind position edge + d
            ops = b"=" * 8 + b"II" + b"=" * 8
            add("ins-at-%s%+d" % (name, d), ops, lambda ops=ops, edge=edge, d=d: (edge + d - 7) + walk(ops)[8][0] - 1 == edge + d, loc=edge + d - 7)
    ops = b"II" + b"=" * 12
    add("ins-at-loc-1-is-lo-1", ops, lambda ops=ops: ops[0] == ord("I") and walk(ops)[0][0] == 0, loc=LO)
    # rows without an alignment between live rows: their store rows hold op bytes all the same
    live = bytes(rng.choice(ALPHABET, size=1500))
    add("live-a", live, lambda: True)
    add("dead-meta_r-0", b"D" * 2000, lambda: True, meta_r=0)
    add("live-b", live, lambda: True)
    add("dead-score--1", b"X" * 2000, lambda: True, score=-1)
    add("live-c", live, lambda: True, score=0)
    add("dead-n_ops-0", b"X" * 2000, lambda: True, n_ops=0)
    add("live-d", live[:777], lambda: True)
    add("dead-n_ops--1", b"D" * 40, lambda: True, n_ops=-1)
    add("live-shorter-than-its-store-row", b"X" * 100, lambda: True, n_ops=37)
    # the filter
    ops = b"=" * 20 + b"XDI" + b"=" * 20
    add("mapq-below", ops, lambda: True, mapq=MIN_MAPQ - 1)
    add("mapq-at", ops, lambda: True, mapq=MIN_MAPQ)
    add("mapq-0", ops, lambda: True, mapq=0)
    # the read buffer's last byte: an 'X' on the read's last base, the row placed last
    ops = b"=" * 50 + b"IIS" + b"=" * 10 + b"X"
    add("X-on-the-last-read-byte", ops, lambda ops=ops: ops[-1] == ord("X") and walk(ops)[-1][1] == qlen(ops) - 1, last=True)
    cases.sort(key=lambda c: c.last)                                         # stable: the `last` row goes last
    return cases


CASES = build()
