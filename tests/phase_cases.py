"""Constructed reads that pin EVERY seed phase and the loop over the phase results (alnmain.c:340-404), from first principles.

Pure numpy / Python on top of tests/constructed.py: nothing here touches an FM index, the oracle or the device library.

    phase_hits(read, p, ...)   the hit stream of phase p by brute force (constructed.phase0_hits is phase 0 of it)
    decide_ref(read, ...)      the reference's loop over the phases, restated with vote_top2 for both histograms
    kill(read, [(w, c)])       one substituted base of class c in window w
    cases()                    the text and the cases, each with the property it is named for as a predicate
    derive(case, cen, rank)    everything the device must return for a case's read, from brute force alone

Throughout S = 20, P = S + 1 = 21; a WINDOW is P consecutive read bases, window q = read[21 q : 21 q + 21].

The kill rule.  Read position x = 21 q + c (class c of window q) lies inside the seed (p, q) -- phase p, j = p + 21 q -- iff
p <= c < p + 20, and inside the seed (p, q - 1) iff c <= p - 2.  It is outside every seed of exactly one phase,
p = c + 1 (mod 21): one substituted base kills one seed in each of the other 20 phases and spares that phase.

A read is a chimera of segments, each a whole number of windows copied from a planted locus (its diagonal: text position
minus read offset), each with its own kills; seeds across two segments have no occurrence; windows of random bases
("dead") pad a read.  Seed (p, q) of a segment survives iff window q has no kill of class >= p and window q + 1 (same
segment) none of class <= p - 2 -- in particular an ISLAND of two windows with kills a (first) and b (second) votes once
in each of the phases a + 1 .. b + 1 and in no other (a = None: from phase 0 on), given 1 <= b <= 19.
"""
import functools

import numpy as np

import constructed as K
import mapq_ref
import rival_ref

S, P, THRES = 20, 21, 300
U64 = K.U64


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def phase_hits(read, p, S, thres, cen, sa_rank):
    """The hit stream of phase p of `read` from first principles: the seeds j = p, p + S + 1, ... while j < len - S
    (alnmain.c:353) contribute, when 0 < count < thres, the keys pos - j (mod 2^64) of their occurrences in the order of their
    suffix-array rows (sa_rank[pos]: the row of the suffix at pos, the inverse of a suffix array check_sa has accepted)."""
    keys = []
    read = bytes(read)
    for j in range(p, max(len(read) - S, 0), S + 1):
        pos = cen.positions(read[j:j + S])
        if 0 < len(pos) < thres:
            for x in sorted(pos, key=lambda x: sa_rank[x]):
                keys.append((x - j) & U64)
    return keys


def decide_ref(read, S, thres, cen, sa_rank):
    """The reference's loop over the phases (alnmain.c:349-403) -> (best = (key, val, bucket), d, phases run, [(v, top two)] of
    every phase that was voted).  d: the phase the loop broke on, S when it ran out.

    num_seeds = len / (S + 1) (:371); with num_seeds == 0 no phase is voted at all and the winner of the empty second
    histogram -- zeros -- comes out.  A phase passes when (double) v / num_seeds > 0.6 (:375-378).  That is 5 v > 3 num_seeds
    exactly: when 5 v == 3 num_seeds the quotient is the real number 3/5, its correctly rounded double IS the literal 0.6, and
    the comparison is false; when 5 v > 3 num_seeds the quotient exceeds 3/5 by at least 1 / (5 num_seeds), many orders of
    magnitude above half an ulp for any read length.  The integer form has no rounding to argue about.
    A phase that does not pass adds its winner -- if it has one (:386) -- to the second histogram; the loop variable is S
    after a break on the last phase and S + 1 after running out, and in both cases (:400) the second histogram's winner
    replaces whatever the break assigned."""
    read = bytes(read)
    n_phases = S + 1
    num_seeds = len(read) // (S + 1)
    best, ot, tops = (0, 0, 0), [], []
    it = 0
    while it < n_phases:
        keys = phase_hits(read, it, S, thres, cen, sa_rank)
        if num_seeds > 0:
            v, top = K.vote_top2(keys)
            tops.append((v, top))
            if 5 * v > 3 * num_seeds:
                best = top[0]
                break
            if top[0][1] != 0:
                ot.append(top[0][0])
        it += 1
    if it >= n_phases - 1:
        best = K.vote_top2(ot)[1][0]
    d = min(it, n_phases - 1)
    return best, d, d + 1, tops


# ---------------------------------------------------------------------------------------------------------------------
# reads
# ---------------------------------------------------------------------------------------------------------------------
def kill(read, kills):
    """`read` with one substituted base per (window, class) pair: position 21 * window + class gets the next base of ACGT."""
    b = bytearray(read)
    for w, c in kills:
        assert 0 <= c < P
        x = P * w + c
        b[x] = b"CGTA"[b"ACGT".index(b[x])]
    return bytes(b)


def dead(rng, k):
    """k windows of random bases: no seed inside them, or across their edges, occurs in the text (the predicates check)."""
    return K._filler(rng, P * k)


def seg(locus, w0, k, kills=()):
    """Windows w0 .. w0 + k - 1 of a locus string with kills (window counted inside the segment)."""
    assert P * (w0 + k) <= len(locus)
    return kill(locus[P * w0:P * (w0 + k)], kills)


def island(locus, a, b, w0=0):
    """Two windows that vote once in each phase a + 1 .. b + 1 (a None: 0 .. b + 1) and in no other."""
    assert 1 <= b <= 19 and (a is None or 0 <= a <= b)
    return seg(locus, w0, 2, ([] if a is None else [(0, a)]) + [(1, b)])


def steer(locus, k, d, h):
    """k windows of a locus whose first h carry the kill that spares phase d only."""
    return seg(locus, 0, k, [(w, (d - 1) % P) for w in range(h)])


# ---------------------------------------------------------------------------------------------------------------------
# the text
# ---------------------------------------------------------------------------------------------------------------------
# name -> windows.  One text for every case.
_LOCI = dict(W12=12, C7=7, Wb=2, W8=8, S1a=4, S1b=4, S2a=4, S2b=4, T2=4, T1=4, T3=3, MA=2, MB=2, EA=2, EB=2, L=20,
             # (planted one after the other: the two loci of a case lie far more than a window radius apart)
             TA=2, VA=7, UA=6, DA=13, RTC=8, SA=12, WA=14, CA=40, TB=2, VB=6, UB=14, DB=7, RTB=8, CB=25,
             EpA=12, EpB=8, EqA=12, EqB=8, EmB=8, EmA=12, EnB=8, EnA=12, RA=12, RB=8, RTA=12)
MINKEY_D, EDGE_D, SUB_X = 11264, 11776, 9316          # diagonals at chosen places in their 16-wide buckets
STAG1, STAG0 = 4096, 6144 + 512                       # a multiple of 2 R, and one of 2 R plus R (R = 512)
_FIXED = [("W12", 7), ("C7", 278), ("Wb", 445), ("W8", 500),
          ("S1a", STAG1 - 2 + 252), ("S1b", STAG1 + 2 + 336), ("S2a", STAG0 - 2 + 252), ("S2b", STAG0 + 2 + 336),
          ("T2", SUB_X + 252), ("T1", SUB_X + 3 + 336), ("T3", SUB_X + 40 + 420),
          ("MA", MINKEY_D + 3), ("MB", MINKEY_D + 63), ("EA", EDGE_D + 15), ("EB", EDGE_D + 16 + 63)]
_AFTER = dict(EpB=("EpA", 0, 252 + 512), EqB=("EqA", 0, 252 + 513), EmA=("EmB", 0, 168 + 512), EnA=("EnB", 0, 168 + 513),
              RB=("RA", 0, 252 + 600))
L_AT = 12288                                          # the 20 windows of the locus L
REPEAT_TOTALS = (255, 256, 257)


def _flank(i):
    return b"ACGT"[(i + 1) % 4:(i + 1) % 4 + 1]


@functools.lru_cache(maxsize=None)
def cases(seed=7):
    """-> (seqs, cases).  seqs: the forward sequence(s) of the index text; cases: a list of dict(name, read, thres, aim,
    predicate).  aim: what the construction prescribes (best key / val, the deciding phase, ...); predicate(r) takes what
    derive() makes of the read by brute force and asserts that the case reaches the edge it is named for."""
    rng = np.random.default_rng(seed)
    loc = {name: K._filler(rng, P * w) for name, w in _LOCI.items()}
    spec = [dict(name=name, seq=loc[name], at=at) for name, at in _FIXED]
    spec.append(dict(name="L", seq=loc["L"], at=L_AT))
    fixed = {name for name, _ in _FIXED} | {"L"}
    for name in _LOCI:
        if name not in fixed:
            spec.append(dict(name=name, seq=loc[name], after=_AFTER.get(name)))
    # walk chunks: 64 repeat k-mers per total, planted once as the read itself (one diagonal) and scattered besides, with a
    # base on either side that differs from the read's spacers there (no seed of another phase gains an occurrence)
    rk = {}
    scattered = []
    for total in REPEAT_TOTALS:
        rk[total] = K.kmers(rng, 64)
        spec.append(dict(name="block%d" % total, seq=K.read_of(rk[total])))
        for i, km in enumerate(rk[total]):
            copies = 3 + (total - 256 if i == 17 else 0)
            scattered += [dict(name="r%d.%d" % (total, i), seq=_flank(i) + km + _flank(i))] * copies
    spec += [scattered[i] for i in rng.permutation(len(scattered))]
    pl = K.plant(spec, seed=seed, gap=(25, 45))
    at = {name: pl.where[name][0] for name in list(_LOCI) + ["block%d" % t for t in REPEAT_TOTALS]}
    out = []

    def add(name, read, aim, predicate, thres=THRES):
        out.append(dict(name=name, read=bytes(read), thres=thres, aim=aim, predicate=predicate))

    def votes(r, p):
        return [(t[0], t[1]) for t in r["tops"][p][1]]

    # ---- the decision loop ------------------------------------------------------------------------------------------
    for d in range(P):
        # 20 windows of L; the first ten carry the kill that spares phase d: every other phase keeps 9 or 10 seeds, phase d
        # all 20 (d = 0) or 19
        def pred(r, d=d):
            assert r["d"] == d and r["phases"] == d + 1 and len(r["tops"]) == d + 1
            assert all(0 < r["tops"][p][1][0][1] <= 10 and r["tops"][p][0] <= 12 for p in range(d))
            assert r["tops"][d][0] == (20 if d == 0 else 19)
            if d < P - 1:
                assert r["best"] == (at["L"], r["tops"][d][0], at["L"] >> 4)
            else:       # the break on the last phase is undone: L won every phase
                assert r["best"] == (at["L"], P - 1, at["L"] >> 4)
        add("break-at-%d" % d, steer(loc["L"], 20, d, 10), dict(key=at["L"], d=d), pred)

    def exact(r):
        assert [t[0] for t in r["tops"]] == [12] * P and r["d"] == P - 1 and r["phases"] == P
        assert r["best"] == (at["L"], P, at["L"] >> 4)
    add("threshold-exact", kill(seg(loc["L"], 0, 13), [(0, 1)]) + dead(rng, 7), dict(key=at["L"], val=P, d=P - 1), exact)

    def exact_twin(r):
        assert [t[0] for t in r["tops"]] == [12, 13] and r["d"] == 1 and r["best"] == (at["L"], 13, at["L"] >> 4)
    add("threshold-exact-twin-13", kill(seg(loc["L"], 0, 13), [(0, 0)]) + dead(rng, 7), dict(key=at["L"], val=13, d=1), exact_twin)

    dB = at["VB"] - 147

    def val2(r):
        assert votes(r, 0) == [(at["VA"], 7), (dB, 6)] and r["d"] == 0 and r["best"] == (at["VA"], 7, at["VA"] >> 4)
    add("val2-counts", loc["VA"] + loc["VB"] + dead(rng, 7), dict(key=at["VA"], val=7, d=0), val2)

    def val2_twin(r):
        assert votes(r, 0) == [(at["VA"], 7), (dB, 5)] and r["d"] == P - 1 and r["best"] == (at["VA"], P, at["VA"] >> 4)
        assert all(t[0] <= 12 for t in r["tops"])
    add("val2-counts-twin-5", loc["VA"] + seg(loc["VB"], 0, 5) + dead(rng, 8), dict(key=at["VA"], val=P, d=P - 1), val2_twin)

    kB = at["UB"] - 126

    def undone(r):
        assert r["d"] == P - 1 and r["phases"] == P and len(r["tops"]) == P
        assert all(votes(r, p) == [(at["UA"], 6 if p < 2 else 5), (0, 0)] for p in range(P - 1))
        assert votes(r, P - 1) == [(kB, 13), (at["UA"], 5)]                   # phase 20 passes with B on top ...
        assert r["best"] == (at["UA"], P - 1, at["UA"] >> 4)                  # ... and A, the winner of 20 phases, comes out
    # (the seed (2, 5) has ONE base in B's first window, which happens to continue A in the text as well: the kill of class 0
    #  there touches that seed and no living one)
    add("last-phase-break-undone", loc["UA"] + seg(loc["UB"], 0, 14, [(0, 0)] + [(w, 19) for w in range(14)]),
        dict(key=at["UA"], val=P - 1, d=P - 1), undone)

    # islands at windows 0-1 and 3-4 of 20
    def two_islands(x, y):
        return x + dead(rng, 1) + y + dead(rng, 15)
    kA, kTB = at["TA"], at["TB"] - 63
    kA2, kTB0 = at["TA"] - 63, at["TB"]

    def winners(r):
        return [r["tops"][p][1][0][:2] for p in range(P)]

    def tie_a(r):
        assert winners(r) == [(kA, 1)] * 10 + [(kTB, 1)] * 10 + [(0, 0)] and r["best"] == (kA, 10, kA >> 4) and r["d"] == P - 1
    add("ot-tie-first-seen-A", two_islands(island(loc["TA"], None, 8), island(loc["TB"], 9, 18)), dict(key=kA, val=10, d=P - 1), tie_a)

    def tie_b(r):
        assert winners(r) == [(kTB0, 1)] * 10 + [(kA2, 1)] * 10 + [(0, 0)] and r["best"] == (kTB0, 10, kTB0 >> 4)
        # the same two loci in the other order: no fixed order of keys or of suffix-array rows gives both twins
        assert (kA < kTB) == (kA2 < kTB0)
    add("ot-tie-first-seen-B", two_islands(island(loc["TB"], None, 8), island(loc["TA"], 9, 18)), dict(key=kTB0, val=10, d=P - 1), tie_b)

    def count_beats(r):
        assert winners(r) == [(kA, 1)] * 10 + [(kTB, 1)] * 11 and r["best"] == (kTB, 11, kTB >> 4)
    add("ot-count-beats-first-seen", two_islands(island(loc["TA"], None, 8), island(loc["TB"], 9, 19)), dict(key=kTB, val=11, d=P - 1), count_beats)

    def min_key(r):
        D = MINKEY_D
        assert D % 16 == 0 and winners(r) == [(D + 3, 1)] * 10 + [(D, 1)] * 10 + [(0, 0)]
        assert r["best"] == (D, 20, D >> 4)
    add("ot-minimum-key", two_islands(island(loc["MA"], None, 8), island(loc["MB"], 9, 18)), dict(key=MINKEY_D, val=20, d=P - 1), min_key)

    def bucket_edge(r):
        D = EDGE_D
        assert D % 16 == 0 and winners(r) == [(D + 15, 1)] * 10 + [(D + 16, 1)] * 11
        assert r["best"] == (D + 16, 11, (D >> 4) + 1)                          # one bucket would have been (D + 15, 21)
    add("ot-bucket-edge", two_islands(island(loc["EA"], None, 8), island(loc["EB"], 9, 19)), dict(key=EDGE_D + 16, val=11, d=P - 1), bucket_edge)

    k1, k2 = (7 - 42) & U64, (at["Wb"] - 483) & U64

    def wrapped(r):
        assert k1 == U64 + 1 - 35 and k2 == U64 + 1 - 38 and k1 >> 4 == k2 >> 4
        assert winners(r) == [(k1, 1)] * 10 + [(k2, 1)] * 10 + [(0, 0)] and r["best"] == (k2, 20, k2 >> 4)
    add("wrapped", dead(rng, 2) + island(loc["W12"], None, 8) + dead(rng, 19) + island(loc["Wb"], 9, 18) + dead(rng, 2),
        dict(key=k2, val=20, d=P - 1), wrapped)

    def single_hit(r):
        assert [t[0] for t in r["tops"]] == [0] * 7 + [1] + [0] * 13 and r["best"] == (kA, 1, kA >> 4) and r["d"] == P - 1
    add("one-hit-in-one-phase", island(loc["TA"], 6, 6) + dead(rng, 2), dict(key=kA, val=1, d=P - 1), single_hit)

    def all_empty(r):
        assert [t[0] for t in r["tops"]] == [0] * P and r["best"] == (0, 0, 0) and r["rec"][:6] == (0, 0, 0, 0, 0, 0)
    add("all-phases-empty", dead(rng, 20), dict(key=0, val=0, d=P - 1), all_empty)

    for ln, val in ((20, 0), (21, 1), (41, 1), (42, 2), (62, 2), (63, 3)):
        def lengths(r, ln=ln, val=val):
            if val == 0:        # num_seeds == 0: no phase is voted
                assert r["tops"] == [] and r["best"] == (0, 0, 0) and r["phases"] == P
            else:
                assert r["d"] == 0 and r["tops"][0][0] == val and r["best"] == (at["L"], val, at["L"] >> 4)
        add("length-%d" % ln, loc["L"][:ln], dict(key=at["L"] if val else 0, val=val, d=0 if val else P - 1), lengths)

    def len42(r):
        assert [t[0] for t in r["tops"]] == [1] * P and r["best"] == (at["L"], P, at["L"] >> 4)      # 5 * 1 > 3 * 2 is false
    add("length-42-one-seed-killed", kill(loc["L"][:42], [(0, 0)]), dict(key=at["L"], val=P, d=P - 1), len42)

    # ---- the evidence of MAPQ and of the rival ----------------------------------------------------------------------
    def pair(a, b, first_b=False):
        """12 windows of locus a and 8 of locus b: phase 0 passes with 12 + 8 of 20."""
        return (loc[b] + loc[a]) if first_b else (loc[a] + loc[b])

    for name, a, b, first_b, delta in (("window-edge-plus-512", "EpA", "EpB", False, 512), ("window-edge-plus-513", "EqA", "EqB", False, 513),
                                       ("window-edge-minus-512", "EmA", "EmB", True, -512), ("window-edge-minus-513", "EnA", "EnB", True, -513)):
        ka = at[a] - (168 if first_b else 0)
        kb = at[b] - (0 if first_b else 252)

        def edge(r, ka=ka, kb=kb, delta=delta):
            assert kb - ka == delta and r["best"] == (ka, 12, ka >> 4) and r["d"] == 0 and r["rec"][2] == 512
            if abs(delta) == 512:
                assert r["rec"][:2] == (20, 0) and r["rec"][3] == 60 and r["rival"] == (0, 0, 0)
            else:
                assert r["rec"][:2] == (12, 8) and r["rival"] == (kb, 8, kb >> 4)
        add(name, pair(a, b, first_b), dict(key=ka, val=12, d=0), edge)

    kra, krb = at["RA"], at["RB"] - 252
    for ln, R in ((4096, 512), (4097, 1024)):
        def radius(r, R=R):
            assert krb - kra == 600 and r["best"][0] == kra and r["rec"][2] == R and r["d"] == P - 1
            assert (r["rec"][1] == 0) == (R == 1024) and (r["rival"] == (0, 0, 0)) == (R == 1024)
            if R == 512:
                assert r["rival"][0] == krb
        body = pair("RA", "RB")
        add("radius-step-%d" % ln, body + K._filler(rng, ln - len(body)), dict(key=kra, d=P - 1), radius)

    for name, a, b, m, whole in (("staggered-around-2R", "S1a", "S1b", STAG1, 1), ("staggered-around-2R-plus-R", "S2a", "S2b", STAG0, 0)):
        def stagger(r, m=m, whole=whole):
            ksa = at["SA"]
            assert r["best"] == (ksa, 12, ksa >> 4) and r["d"] == 0 and r["rec"][:3] == (12, 8, 512)
            ks = [k for k in r["evidence"] if k != ksa]
            assert sorted(ks) == [m - 2] * 4 + [m + 2] * 4
            for h in (0, 1):        # the whole cluster is in ONE bucket of histogram `whole` and in two of the other
                assert len({mapq_ref.bucket(k, 9, h) for k in ks}) == (1 if h == whole else 2)
            assert r["rival"] == (m - 2, 4, (m - 2) >> 4)       # two sub-buckets of 4: the smaller index
        add(name, loc["SA"] + loc[a] + loc[b], dict(key=at["SA"], val=12, d=0), stagger)

    kda, kdb = at["DA"], at["DB"] - 273

    def stops(r):
        assert r["d"] == 3 and r["best"][0] == kda and abs(kdb - kda) > 1024
        assert all(len(h) > 0 for h in r["hits"][4:]) and r["rec_all"][:2] != r["rec"][:2]
        assert r["rec"][0] == sum(h.count(kda) for h in r["hits"][:4]) and r["rec"][1] == sum(h.count(kdb) for h in r["hits"][:4])
        assert r["rival"][0] == kdb
    add("evidence-stops-at-d", steer(loc["DA"], 13, 3, 7) + steer(loc["DB"], 7, 3, 3), dict(key=kda, d=3), stops)

    kwa, kw8 = at["WA"], (500 - 525) & U64

    def wrap_rival(r):
        assert r["best"] == (kwa, 14, kwa >> 4) and r["d"] == 0 and r["rec"][:2] == (14, 8)
        assert kw8 >> 32 == (1 << 32) - 1 and r["rival"] == (kw8, 8, kw8 >> 4)
    add("wrapped-rival", loc["WA"] + dead(rng, 11) + loc["W8"], dict(key=kwa, val=14, d=0), wrap_rival)

    kw12 = (7 - 21) & U64

    def spans_zero(r):
        assert r["best"] == (kw12, 12, kw12 >> 4) and r["hits"][0].count(5) == 7 and r["rec"][:4] == (19, 0, 512, 60)
    add("window-spans-zero", dead(rng, 1) + loc["W12"] + loc["C7"], dict(key=kw12, val=12, d=0), spans_zero)

    krta, krtb, krtc = at["RTA"], at["RTB"] - 252, at["RTC"] - 420

    def pair_tie(r):
        assert r["best"] == (krta, 12, krta >> 4) and r["rec"][:2] == (12, 8)
        assert krtc < krtb and krtb - krtc > 2048 and min(abs(krta - krtb), abs(krta - krtc)) > 2048
        assert r["hits"][0].index(krtb) < r["hits"][0].index(krtc)            # the pair seen later has the smaller bucket
        assert r["rival"] == (krtc, 8, krtc >> 4)
    add("rival-pairs-tie", loc["RTA"] + loc["RTB"] + loc["RTC"], dict(key=krta, val=12, d=0), pair_tie)

    def sub_bucket(r):
        X = SUB_X
        assert X % 16 <= 12 and X >> 10 == (X + 40) >> 10 and (X + 40) >> 4 != X >> 4
        ks = [k for k in r["hits"][0] if k != krta]
        assert sorted(ks) == [X] * 4 + [X + 3] * 4 + [X + 40] * 3 and r["rec"][:2] == (12, 11)
        assert r["rival"] == (X, 8, X >> 4)             # the fullest sub-bucket, its smallest key, its count
    add("rival-entry-of-the-sub-bucket", loc["RTA"] + loc["T2"] + loc["T1"] + loc["T3"], dict(key=krta, val=12, d=0), sub_bucket)

    for nb in (24, 25):
        def survivors(r, nb=nb):
            assert len(r["survivors"][0]) == 40 + nb and set(r["survivors"][0]) == {1} and r["d"] == 0
            assert r["rec"][:2] == (40, nb) and r["rival"][:2] == (at["CB"] - 840, nb)
        add("evidence-phase-of-%d-survivors" % (40 + nb), loc["CA"] + seg(loc["CB"], 0, nb) + dead(rng, 20), dict(key=at["CA"], val=40, d=0), survivors)

    for total in REPEAT_TOTALS:
        kb_ = at["block%d" % total]

        def repeats(r, total=total, kb_=kb_):
            assert len(r["survivors"][0]) == 64 and sum(r["survivors"][0]) == total and min(r["survivors"][0]) >= 3
            assert r["d"] == 0 and r["best"] == (kb_, 64, kb_ >> 4) and len(r["hits"][0]) == total and r["rec"][0] >= 64
        add("repeat-chunk-of-%d-hits" % total, K.read_of(rk[total]), dict(key=kb_, val=64, d=0), repeats)
    return [pl.seq], out


def derive(case, cen, sa_rank):
    """Everything the seed stage, the mapping-quality stage and the rival stage must return for the read of `case`, by brute
    force: best, d, phases, tops (decide_ref); hits: the hit stream of ALL S + 1 phases; survivors: per phase the hit counts
    of its surviving seeds in seed order; evidence: the hits of phases 0 .. d; rec / rival: the records over the evidence;
    rec_all: the record over all phases."""
    read, thres = case["read"], case["thres"]
    best, d, phases, tops = decide_ref(read, S, thres, cen, sa_rank)
    hits = [phase_hits(read, p, S, thres, cen, sa_rank) for p in range(P)]
    surv = [[n for n in (len(cen.positions(read[j:j + S])) for j in range(p, max(len(read) - S, 0), P)) if 0 < n < thres]
            for p in range(P)]
    evidence = [k for h in hits[:d + 1] for k in h]
    rival, rec = rival_ref.rival_of_hits_scalar(evidence, best, len(read))
    rec = mapq_ref.record_of_hits(evidence, best, len(read), d)
    assert rec[:4] == rival_ref.rival_of_hits(evidence, best, len(read))[1][:4]
    rec_all = mapq_ref.record_of_hits([k for h in hits for k in h], best, len(read), d)
    return dict(best=best, d=d, phases=phases, tops=tops, hits=hits, survivors=surv, evidence=evidence, rec=rec, rival=rival,
                rec_all=rec_all)
