"""Constructed alignments for the extension kernels: every case is built to reach one edge of docs/GACT_SPEC.md and
carries a predicate on tests/gact_ref.py's trace that says so.

A case is a dict(name, family, q, d, T, O, W, pred); pred(score, ops, trace) must hold on the reference's answer
(tests/test_gact_constructed_cpu.py checks it), so a case that no longer hits its edge after a constant changes fails
instead of going quiet.  Nothing here runs an aligner: the module only builds inputs.

    cases()                    the named cases, all families
    exhaustive_square()        every (q, d), m = n: {A,C} up to 7 bases, {A,C,G,T} up to 3
    exhaustive_ragged()        every (q, d), m != n, {A,C}, 1 .. 6 bases each
    EXHAUSTIVE_PARAMS          the (T, O, W) the exhaustive sets run at
    batch_of(pairs)            square pairs laid end to end as an index text + reads + best[] keys (batch path)
    packing_batch()            one window at every locus residue mod 64, both strands, sequence ends, fenced windows
"""
import itertools
import zlib

import numpy as np

import constructed

BS_K = 32                                   # anti-diagonals per traceback block of the bit-sliced kernel
EXHAUSTIVE_PARAMS = [(16, 0, 2), (16, 0, 4), (16, 8, 8), (16, 15, 16), (320, 120, 128)]
TILES = [(320, 120), (512, 120), (320, 0), (100, 99), (64, 16), (33, 7), (16, 0), (512, 0), (256, 120)]


def rnd(n, *key):
    """n random bases, a function of the key alone."""
    rng = np.random.default_rng([zlib.crc32(repr(key).encode()), n])
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])


def other(c, k=1):
    """A base different from c (the k-th next one in ACGT)."""
    return b"ACGT"[(b"ACGT".index(c) + k) % 4]


def _words(alphabet, n):
    return [bytes(t) for t in itertools.product(alphabet, repeat=n)]


def exhaustive_square():
    return ([(q, d) for n in range(1, 8) for q in _words(b"AC", n) for d in _words(b"AC", n)] +
            [(q, d) for n in range(1, 4) for q in _words(b"ACGT", n) for d in _words(b"ACGT", n)])


def exhaustive_ragged():
    return [(q, d) for n in range(1, 7) for m in range(1, 7) if n != m for q in _words(b"AC", n) for d in _words(b"AC", m)]


def _case(out, family, name, q, d, T, O, W, pred):
    out.append(dict(name="%s/%s@%d,%d,%d" % (family, name, T, O, W), family=family, q=bytes(q), d=bytes(d), T=T, O=O, W=W,
                    pred=pred))


# ---------------------------------------------------------------------------------------------------------------------
# predicates
# ---------------------------------------------------------------------------------------------------------------------
def _always(score, ops, trace):
    return True


def _has_tie(score, ops, trace):
    return any(len(t) > 1 for t in trace.union("ties"))


def _ops_are(want):
    return lambda score, ops, trace: ops == want


def _stop_near(col):
    """A 'keep' stop of a non-final tile lies within one read column of col."""
    return lambda score, ops, trace: any("keep" in t["rule"] and abs(t["i"] + t["stop"][0] - col) <= 1 for t in trace)


def _both(*preds):
    return lambda score, ops, trace: all(p(score, ops, trace) for p in preds)


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------
def _ties(out):
    for T, O, W in ((320, 120, 128), (64, 16, 32), (16, 0, 4), (320, 120, 1024)):
        n = 450 if T > 64 else 150
        for dm in sorted({0, 1, -1, W // 2, -(W // 2)}):
            if n + dm > 0 and abs(dm) < n:
                _case(out, "ties", "A%d-A%+d" % (n, dm), b"A" * n, b"A" * (n + dm), T, O, W, _always)
        _case(out, "ties", "AC-CA", b"AC" * (n // 2), b"CA" * (n // 2), T, O, W, _has_tie)
        _case(out, "ties", "A-C", b"A" * n, b"C" * n, T, O, W, _has_tie)
        _case(out, "ties", "ACG-CGA", b"ACG" * (n // 3), b"CGA" * (n // 3), T, O, W, _always)
        _case(out, "ties", "ACG-GAC", b"ACG" * (n // 3), b"GAC" * (n // 3), T, O, W, _always)
        for L in (10, 31, 32, 33, 64, 200):
            for dl in (-2, -1, 1, 2):
                left, right = rnd(40, "hl", L), rnd(300 if T > 64 else 60, "hr", L)
                left, right = left[:-1] + b"C", b"G" + right[1:]
                _case(out, "ties", "run%d%+d" % (L, dl), left + b"A" * L + right, left + b"A" * (L + dl) + right, T, O, W,
                      _always)


def _band(out):
    for W in (2, 4, 20, 32, 64, 66, 128, 256, 1024):
        T, O = (320, 120) if W <= 128 else (512, 120)
        half = W // 2
        for tile in ((0, 1) if W <= 128 else (0,)):
            at = 20 + tile * (T - O)
            head, rest = rnd(at, "bh", W), rnd(T + 60, "br", W)
            plain = head + rest
            # the gap run is made of a base its neighbours are not: the run has one place to go
            for kind, edge in (("del", half - 1), ("ins", half)):
                lengths = (half - 1, half, half + 1) if W < 1024 else (200,)
                for L in lengths:
                    junk = bytes(other(c, 2) for c in rest[:L]) if L else b""
                    gapped = head + junk + rest
                    q, d = (plain, gapped) if kind == "del" else (gapped, plain)
                    fits = L <= edge

                    def pred(score, ops, trace, kind=kind, L=L, fits=fits, tile=tile, W=W):
                        lo = min(t["dmin"] for t in trace)
                        hi = max(t["dmax"] for t in trace)
                        if hi > W // 2 - 1 or lo < -(W // 2):
                            return False
                        if fits:                # the walk goes out to the planted drift, and the answer is the planted one
                            return score == L and (hi if kind == "del" else -lo) == L
                        return score > L        # forced off the true path: it pays more than the run
                    _case(out, "band", "%s%d-tile%d" % (kind, L, tile), q, d, T, O, W, pred)
    # net drift spread over a tile, 2 insertions to 1 deletion (PacBio CLR): out to the positive edge, then back and out to
    # the negative edge just before the walk stop
    T, O = 320, 120
    for W in (16, 32):
        half = W // 2
        base = rnd(700, "drift", W)
        del_at = {10 + 4 * k for k in range(half - 1)}
        ins_at = {4 * half + 12 + 3 * k for k in range(2 * half - 1)}
        q = bytearray()
        for k, c in enumerate(base):
            if k in del_at:
                continue
            q.append(c)
            if k in ins_at:
                q.append(next(x for x in b"ACGT" if x not in (c, base[k + 1])))
        _case(out, "band", "drift2to1", bytes(q), base, T, O, W,
              lambda score, ops, trace, half=half: (trace[0]["dmin"], trace[0]["dmax"]) == (-half, half - 1) and
              "keep" in trace[0]["rule"] and score == 3 * half - 2)


def _with_subs(s, every=37):
    s = bytearray(s)
    for k in range(every // 2, len(s), every):
        s[k] = other(s[k])
    return bytes(s)


def _tile_edges(out):
    for T, O in TILES:
        keep = T - O
        for W in ((128,) if (T, O) != (320, 120) else (128, 320)):
            lengths = sorted({k * keep + e for k in (1, 2, 3) for e in (-1, 0, 1)} | {T - 1, T, T + 1, 2 * keep - 1, 2 * keep + 1})
            for n in lengths:
                if n < 1:
                    continue
                d = rnd(n, "len", T, O)
                q = _with_subs(d)
                want = bytes(ord("=") if x == y else ord("X") for x, y in zip(q, d))
                _case(out, "tile", "len%d" % n, q, d, T, O, W, _ops_are(want))
            # one X, I or D on the columns around the first and the second walk stop
            n = keep + T + 10
            base = rnd(n + 1, "straddle", T, O)
            for stop in (1, 2):
                for dc in (-1, 0, 1):
                    c = stop * keep + dc
                    sub = base[:c] + bytes([other(base[c])]) + base[c + 1:n]
                    ins_base = next(x for x in b"ACGT" if x not in (base[c - 1], base[c]))
                    _case(out, "tile", "X@%d-stop%d" % (c, stop), sub, base[:n], T, O, W, _both(_stop_near(stop * keep), lambda s, o, t: s == 1))
                    _case(out, "tile", "I@%d-stop%d" % (c, stop), base[:c] + bytes([ins_base]) + base[c:n - 1], base[:n], T, O, W,
                          _both(_stop_near(stop * keep), lambda s, o, t: 1 <= s <= 3 and b"I" in o))
                    _case(out, "tile", "D@%d-stop%d" % (c, stop), base[:c] + base[c + 1:n + 1], base[:n], T, O, W,
                          _both(_stop_near(stop * keep), lambda s, o, t: 1 <= s <= 3 and b"D" in o))
            # an insertion run that starts ON the walk stop and is too long for what is left of the tile to justify: the
            # tile that stops there must leave the decision to the next one, which sees the run's far side
            if (T, O) in ((64, 16), (33, 7)):
                L = O - 2
                junk = bytes(base[keep + k] if k % 2 == 1 else other(base[keep + k]) for k in range(L))
                _case(out, "tile", "run-on-the-stop", base[:keep] + junk + base[keep:n - L], base[:n], T, O, W,
                      lambda sc, o, t, keep=keep, L=L: t[0]["stop"] == (keep, keep) and o[keep:keep + 1] == b"I" and sc == L)
            # the final tile: cut by a + b < 2(T-O) and continued in another tile, or just finishing
            if 0 < O and keep + 1 <= T:
                s = rnd(T, "cap", T, O)
                _case(out, "tile", "final-just-finishes", s[:keep], s[:keep], T, O, W,
                      lambda sc, o, t: len(t) == 1 and t[0]["rule"] == {"read", "text", "cap"})
                _case(out, "tile", "final-one-short", s[:keep - 1], s[:keep - 1], T, O, W,
                      lambda sc, o, t: len(t) == 1 and t[0]["rule"] == {"read", "text"}) if keep > 1 else None
                _case(out, "tile", "final-cut", s[:keep + 1], s[:keep + 1], T, O, W,
                      lambda sc, o, t: len(t) == 2 and t[0]["last"] and t[0]["rule"] == {"cap"} and t[1]["stop"] == (1, 1))
            # clipped on one side only
            if T >= 64:
                s = rnd(T + 40, "clip", T, O)
                short = T - 30
                _case(out, "tile", "text-clipped", s[:T + 40], s[:short], T, O, W,
                      lambda sc, o, t: t[0]["tt"] < t[0]["tq"] and not t[0]["last"])
                _case(out, "tile", "read-clipped", s[:short], s[:T + 40], T, O, W,
                      lambda sc, o, t: t[0]["tq"] < t[0]["tt"] and t[0]["last"])


def _exhaustion(out):
    for T, O, W in ((320, 120, 128), (64, 16, 32), (320, 120, 256)):
        keep = T - O
        n = 2 * T + 37
        s = rnd(n, "exh", T)
        for m in (n - 1, n - 7, n // 2, 1):
            _case(out, "exhaustion", "m=%d" % m, s, s[:m], T, O, W,
                  lambda sc, o, t, tail=n - m: t.tail == tail and o == b"=" * (len(o) - tail) + b"I" * tail)
        # deletions first: the text runs out earlier and the trailing run is longer than n - m
        gap = bytes(other(c, 2) for c in s[30:34])
        _case(out, "exhaustion", "deletions-first", s, (s[:30] + gap + s[30:])[:n - 7], T, O, W,
              lambda sc, o, t: t.tail == 11 and o.count(b"D") == 4)
        _case(out, "exhaustion", "n=1", s[:1], s, T, O, W, lambda sc, o, t: o == b"=" and len(t) == 1)
        _case(out, "exhaustion", "n=1-mismatch", bytes([other(s[0])]), s, T, O, W, lambda sc, o, t: len(o) == 1 and sc == 1)
        _case(out, "exhaustion", "m=1-mismatch", s, bytes([other(s[0])]), T, O, W, lambda sc, o, t, n=n: t.tail >= n - 1 and sc == n)
        _case(out, "exhaustion", "at-walk-stop", s, s[:keep], T, O, W,
              lambda sc, o, t: len(t) == 1 and t[0]["rule"] == {"text", "keep"} and t.tail == len(o) - t[0]["stop"][0])
        _case(out, "exhaustion", "at-second-walk-stop", s, s[:2 * keep], T, O, W,
              lambda sc, o, t: len(t) == 2 and "text" in t[1]["rule"] and "keep" in t[1]["rule"])


def _blocks(out):
    for T, O, W in ((320, 120, 128), (64, 16, 32), (512, 0, 128)):
        lim = 2 * (T - O)
        marks = sorted({x for x in (31, 32, 33, 63, 64, 65, (lim - 1) // BS_K * BS_K, (lim - 1) // BS_K * BS_K - 1,
                                    (lim - 1) // BS_K * BS_K + 1, lim - 1, lim - 2) if 2 < x < lim})
        s = rnd(T - 2, "blk", T)                                 # one final tile: its walk may go on to anti-diagonal lim
        for x in marks:
            if x // 2 + 2 > len(s):
                continue
            # an insertion on anti-diagonal x: after x / 2 matches, or after a leading deletion and (x - 1) / 2 matches
            lead = x % 2
            c = (x - lead) // 2
            d = (bytes([other(s[0], 2)]) if lead else b"") + s
            ins_base = next(b for b in b"ACGT" if b not in (s[c - 1], s[c]))
            q = s[:c] + bytes([ins_base]) + s[c:]
            _case(out, "blocks", "indel@%d" % x, q, d, T, O, W, lambda sc, o, t, x=x: x in t[0]["anti"])
            # the walk of a final tile ending on anti-diagonal x (clean read; an odd x needs one deletion)
            n = (x - lead) // 2
            if n >= 4:
                d2 = (s[:2] + bytes([other(s[2], 2)]) + s[2:]) if lead else s
                _case(out, "blocks", "end@%d" % x, s[:n], d2[:n + lead], T, O, W,
                      lambda sc, o, t, x=x: len(t) == 1 and sum(t[0]["stop"]) == x)
        for n in (15, 16, 17, 31, 32, 33, 47, 48, 49):          # k and k + 1 blocks
            _case(out, "blocks", "len%d" % n, _with_subs(s[:n], 11), s[:n], T, O, W,
                  lambda sc, o, t, n=n, keep=T - O: sum(t[0]["stop"]) == 2 * min(n, keep))


def _mutate(rng, s, sub, ins, dele):
    out = bytearray()
    for c in s:
        x = rng.random()
        if x < dele:
            continue
        if x < dele + sub:
            c = rng.choice([b for b in b"ACGT" if b != c])
        out.append(c)
        if rng.random() < ins:
            out.append(rng.choice(list(b"ACGT")))
    return bytes(out)


def _random_fill(out):
    rng = np.random.default_rng(11)
    for T, O, W in ((320, 120, 128), (64, 16, 32), (128, 32, 256), (320, 120, 20)):
        for n in (65, 321, 1000, 2500):
            for prof in ((0.04, 0.03, 0.03), (0.015, 0.09, 0.045), (0.2, 0.1, 0.1)):
                ref = rnd(n + 40, "fill", n)
                q = _mutate(rng, ref[:n], *prof) or b"C"
                _case(out, "random", "n%d-%s" % (n, "/".join(str(x) for x in prof)), q, ref[:len(q)], T, O, W, _always)
                if n < 2500:
                    _case(out, "random", "n%d-%s-ragged" % (n, "/".join(str(x) for x in prof)), q, ref[:max(1, len(q) - 7)],
                          T, O, W, _always)


def cases():
    out = []
    for family in (_ties, _band, _tile_edges, _exhaustion, _blocks, _random_fill):
        family(out)
    out = [c for c in out if c is not None]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), "case names are unique"
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the batch path: an index text, reads and best[] keys written by the test
# ---------------------------------------------------------------------------------------------------------------------
def key_of(start, seq_len, pos, n, strand):
    """best[].key that resolves to the window [pos, pos + n) of the forward sequence at text offset `start`: the forward
    strand is addressed directly, the reverse strand by the mirrored position in the sequence's second half."""
    return (start + pos if strand == 0 else start + 2 * seq_len - pos - n) & constructed.U64


def batch_of(pairs, order=None):
    """Square pairs as a batch: the text is the d's laid end to end (one sequence), read k points at the start of d_k.
    -> dict(seqs, reads [bytes], keys [int], windows [bytes], lens)."""
    seq = b"".join(d for _, d in pairs)
    pos = np.concatenate([[0], np.cumsum([len(d) for _, d in pairs])])
    reads, keys, windows = [], [], []
    for k, (q, d) in enumerate(pairs):
        assert len(q) == len(d)
        reads.append(q)
        keys.append(int(pos[k]))
        windows.append(d)
    return dict(seqs=[seq], reads=reads, keys=keys, windows=windows)


def read_matrix(reads, stride=None):
    stride = stride or max(len(r) for r in reads) + 1
    arr = np.zeros((len(reads), stride), dtype=np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return arr, np.array([len(r) for r in reads], dtype=np.uint32)


def packing_batch(seed=3):
    """Three sequences; in the first, a 200-, a 321- and a 1000-base window planted (constructed.plant) at 64 consecutive
    starts each -- whatever the planar text's word size, every residue occurs -- and read on both strands; windows on the
    first and last base of each sequence (the reverse-strand key of the last sequence's first window ends on the text's last
    base), and windows one base beyond either end of a sequence, which the lookup refuses.

    -> dict(seqs, reads, keys, windows (None: fenced), strand, seq_id, pos): read r, after the product has reverse-
    complemented it when strand is 1, is expected to align against windows[r] = seqs[seq_id][pos : pos + len]."""
    lens = (200, 321, 1000)
    wins = {n: _with_subs(rnd(n, "pack", n), 53) for n in lens}
    spec, at = [], 7
    for n in lens:
        for r in range(64):
            spec.append(dict(name=(n, r), seq=rnd(n, "pack", n), at=at))
            at += n + 40 + (1 - (n + 40)) % 64                  # the next start is one residue mod 64 further
    pl = constructed.plant(spec, seed=seed, k=20, tries=4)
    seq0 = pl.seq
    seq1 = rnd(777, "pack-seq1")
    seq2 = rnd(64 * 9 + 31, "pack-seq2")
    seqs = [seq0, seq1, seq2]
    starts = np.concatenate([[0], np.cumsum([2 * len(s) for s in seqs])])
    out = dict(seqs=seqs, reads=[], keys=[], windows=[], strand=[], seq_id=[], pos=[])

    def add(sid, pos, q, strand, fenced=False):
        n = len(q)
        out["reads"].append(constructed.revcomp(q) if strand else q)
        out["keys"].append(key_of(int(starts[sid]), len(seqs[sid]), pos, n, strand))
        out["windows"].append(None if fenced else seqs[sid][pos:pos + n])
        out["strand"].append(strand)
        out["seq_id"].append(sid)
        out["pos"].append(pos)

    for n in lens:
        for r in range(64):
            p = pl.where[(n, r)][0]
            for strand in (0, 1):
                add(0, p, wins[n], strand)
    # read lengths around the word sizes, at a start of every residue class that matters, both strands
    for n in (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129):
        for p in (0, 1, 31, 32, 33, 63, 64, len(seq2) - n, len(seq2) - n - 1):
            for strand in (0, 1):
                add(2, p, _with_subs(seq2[p:p + n], 13), strand)
    # first and last base of every sequence; the last window of the last sequence ends on the text's last forward base
    for sid, s in enumerate(seqs):
        for n in (1, 2, 40, 200):
            for strand in (0, 1):
                add(sid, 0, _with_subs(s[:n], 17), strand)
                add(sid, len(s) - n, _with_subs(s[len(s) - n:], 17), strand)
                add(sid, len(s) - n - 1, _with_subs(s[len(s) - n - 1:len(s) - 1], 17), strand)
                if n > 1:                 # one base beyond either end: neither strand's half holds the window
                    add(sid, len(s) - n + 1, s[len(s) - n:] + b"A", strand, fenced=True)
                    add(sid, -1, b"A" + s[:n - 1], strand, fenced=True)
    return out
