"""Constructed votes at workgroup scale: the ranking edges of tests/test_gpu_vote_rank.py, lifted with ballast onto the
workgroup forms of the vote kernels (vote_kernels.hip: vote_fast_block_kernel, vote_item_block), with BOTH entries of the
per-phase record expected from brute force (constructed.py: census + vote_top2) and cross-checked against the oracle's trace.

The path model.  With c = the phase-0 survivors of a read and H = their hits (both read from the oracle's trace):

    fast run, c <= 192                wavefront form of the fast kernel            (test_gpu_vote_rank.py)
    fast run, 193 <= c <= 1536        vote_fast_block_kernel
    fast run, c >= 1537               exact kernel
    exact kernel, H <= 192            wavefront tier
    exact kernel, H > 192             workgroup tier: passes = ceil(H / 768); keys cached iff passes > 2 and H <= 16384;
                                      the table in global memory iff H > 16384 and no debug limits are set; with debug
                                      limits (L, slots) passes = ceil(H / L), no global table, the cache rule unchanged

Placement: survivor s of an item is held by thread s mod 256, in wavefront (s mod 256) // 64, of chunk s // 256 (in the fast
workgroup form: register slot s // 256 of that thread); hit h of a chunk's staged repeat hits by thread h mod 256.

lift: a small ranking case becomes a read of TOKENS -- its loci at chosen survivor indices, unique ballast seeds (each
planted once) that raise c and repeat ballast k-mers (each planted `copies` times at scattered places) that raise H.  Ballast
buckets collide by chance; no predicate assumes how far: every one MEASURES the largest ballast bucket of the read and
asserts that it lies below the second planted count.

tests/models/vote_hash_harness.c (the kernels' own bucket_hash, through csrc/vote_hash.h) says in which pass a bucket is
admitted and which sketch counter it lands on.  It is used for predicates, for choosing a case among candidates and a debug
limit L among a few -- never for an expected vote result.
"""
import ctypes as C
import functools
import os
import subprocess
import zlib

import numpy as np

import constructed as K

S, P, THRES, HLEN = 20, 21, 300, 8
U64 = K.U64
T1_LIMIT, FAST_LIST, FAST_COUNTERS = 192, 64, 1024             # wavefront forms: survivors / hits, list entries, sketch counters
FB_LIMIT, FB_LIST, FB_COUNTERS = 1536, 512, 4096               # vote_fast_block_kernel
T3_LIMIT, T3_CHUNK, KC_CAP = 768, 256, 16384                   # vote_item_block: hits per pass, survivors per chunk, key scratch
LIMITS = (100, 512)                                            # the debug limits of a case that does not choose its own
L_CHOICES = [100] + [x for d in range(1, 41) for x in (100 - d, 100 + d)]      # ... and the pass limits one may choose from

HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(HERE, "models", "vote_hash_harness.c")
_HDR = os.path.join(HERE, "..", "longreadmapper_amd", "csrc", "vote_hash.h")
_LIB = os.path.join(HERE, "models", "libvote_hash_harness.so")


# ---------------------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def harness():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", _LIB, _SRC])
    so = C.CDLL(_LIB)
    so.vh_hash.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    so.vh_pass.argtypes = so.vh_counter.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
    for f in (so.vh_hash, so.vh_pass, so.vh_counter):
        f.restype = None
    return so


def _call(fn, buckets, *extra):
    b = np.ascontiguousarray(np.array([int(x) & U64 for x in buckets], dtype=np.uint64))
    out = np.zeros(len(b), dtype=np.uint32)
    if len(b):
        fn(b.ctypes.data, len(b), *extra, out.ctypes.data)
    return [int(x) for x in out]


def bucket_hashes(buckets):
    return _call(harness().vh_hash, buckets)


def bucket_passes(buckets, passes):
    """The pass of each bucket in a vote of `passes` passes (vote_admit)."""
    return _call(harness().vh_pass, buckets, passes)


def sketch_counters(buckets, counters):
    """The sketch counter of each bucket in a sketch of `counters` counters (fast_hits)."""
    return _call(harness().vh_counter, buckets, counters - 1)


# ---------------------------------------------------------------------------------------------------------------------
# the path model
# ---------------------------------------------------------------------------------------------------------------------
def fast_path(c):
    """Where a fast run takes a phase item of c survivors first."""
    return "none" if c == 0 else "fast-wave" if c <= T1_LIMIT else "fast-block" if c <= FB_LIMIT else "exact"


def exact_path(H, limits=(0, 0)):
    """How the exact kernel votes an item of H hits: tier, passes, whether the keys are cached, where the table lies."""
    if H <= T1_LIMIT:
        return dict(tier="wave", passes=1, cache=False, table="lds")
    in_global = H > KC_CAP and not limits[0]
    passes = 1 if in_global else -(-H // (limits[0] or T3_LIMIT))
    return dict(tier="block", passes=passes, cache=passes > 2 and H <= KC_CAP, table="global" if in_global else "lds")


def thread(s):
    return s % 256


def wave(s):
    return (s % 256) // 64


def chunk(s):
    return s // 256


def settles(hits, rrs):
    """Whether the fast kernels settle a phase item, from its hits and the kernels' documented rule (vote_kernels.hip, "fast
    path", A - C): the table holds the buckets of the unique seeds; a repeat seed's hit in one of them goes on the list, any
    other on a sketch counter; the item is settled iff the list holds its entries and the largest counter M lies below the
    table's second count.  -> (settled, why); the sketch counter of a bucket is the harness's."""
    c = len(rrs)
    form = fast_path(c)
    if form == "exact":
        return False, "more than %d survivors" % FB_LIMIT
    cap, counters = (FAST_LIST, FAST_COUNTERS) if form == "fast-wave" else (FB_LIST, FB_COUNTERS)
    table = {}
    for key, s, q, t in hits:
        if rrs[s] == 1:
            table[key >> 4] = 0
    n_list, alone = 0, []
    for key, s, q, t in hits:
        if key >> 4 in table:
            table[key >> 4] += 1
            n_list += rrs[s] > 1
        else:
            alone.append(key >> 4)
    if n_list > cap:
        return False, "list: %d entries" % n_list
    if all(r == 1 for r in rrs):
        return True, "no repeat seed"
    t2 = sorted(table.values())[-2] if len(table) >= 2 else 0
    per_bucket = {}
    for b in alone:
        per_bucket[b] = per_bucket.get(b, 0) + 1
    if per_bucket and max(per_bucket.values()) >= t2:
        return False, "counting: a repeat-only bucket of %d >= %d" % (max(per_bucket.values()), t2)
    if len(alone) < t2:
        return True, "counting: %d repeat-only hits < %d" % (len(alone), t2)
    count = {}
    for x in sketch_counters(alone, counters):
        count[x] = count.get(x, 0) + 1
    M = max(count.values())
    return M < t2, "sketch: M = %d against %d" % (M, t2)


# ---------------------------------------------------------------------------------------------------------------------
# texts and reads
# ---------------------------------------------------------------------------------------------------------------------
def _spacer(i):
    """The base a read carries behind ballast seed i of a pool: never T, the base on either side of every ballast copy in the
    text -- no seed of another phase that reaches across a ballast seed's edge gains an occurrence."""
    return b"ACG"[i % 3:i % 3 + 1]


class Text:
    """A text under construction: loci (strings planted in the order they are named, the first one at `beyond`, past every
    read's length so that no ordinary diagonal wraps), front loci (below `beyond`: wrapped keys) and ballast.  Reads are
    written down as tokens and made once the text is planted (build): a ballast seed whose hit would fall into a bucket of
    one of the read's loci -- known from the planted positions alone -- is passed over for the next of its pool, so the planted
    counts of a read are exact."""

    def __init__(self, name, beyond, gap=(40, 90), ready=None):
        """ready: (forward sequence, {read name: bases}) of a text made elsewhere -- nothing is planted, its reads are not tokens."""
        self.name, self.beyond, self.gap, self.ready = name, beyond, gap, ready
        self.seed = zlib.crc32(name.encode())
        self.rng = np.random.default_rng(self.seed)
        self.front, self.loci, self.scatter = [], [], []
        self.piece = {}                  # name -> the bases a read carries for it
        self.pool = dict(u=[], r=[])
        self.tokens, self.reads, self.pl = {}, {}, None

    def segment(self, n):
        return K.segment(self.rng, n)

    def locus(self, name, seq, at=None, after=None, front=False, piece=None):
        (self.front if front else self.loci).append(dict(name=name, seq=seq, at=at, after=after))
        self.piece[name] = seq if piece is None else piece
        assert len(self.piece[name]) % P == 0
        return seq

    def ballast(self, n_uniq, reps=()):
        """n_uniq unique ballast seeds; reps: (n, copies) -- n repeat ballast k-mers of `copies` scattered copies each (one
        value of `copies` per text: a read's H does not depend on which of them it takes)."""
        assert len({c for _, c in reps}) <= 1
        self.pool["u"] = K.kmers(self.rng, n_uniq)
        self.scatter += [dict(name="bu%d" % i, seq=b"T" + k + b"T") for i, k in enumerate(self.pool["u"])]
        for n, copies in reps:
            for k in K.kmers(self.rng, n):
                self.scatter += [dict(name="br%d" % len(self.pool["r"]), seq=b"T" + k + b"T")] * copies
                self.pool["r"].append(k)

    def scattered(self, name, seq):
        assert name not in self.piece
        self.scatter.append(dict(name=name, seq=seq))

    def read(self, name, *tokens):
        """A read of tokens: a locus name (its piece), ("L", name, a, b) (seeds a .. b - 1 of its piece), ("u", n) / ("r", n)
        (the next n unique / repeat ballast seeds of the pools, counted from the start in every read)."""
        toks = [("L", t, 0, len(self.piece[t]) // P) if isinstance(t, str) else t for t in tokens]
        assert all(t[0] == "L" or t[1] >= 0 for t in toks), (name, toks)
        self.tokens[name] = toks
        return name

    def _make(self, name):
        """who[q]: the token seed q came from."""
        toks, where = self.tokens[name], self.pl.where
        core, q = set(), 0
        for t in toks:                                  # the buckets of the read's loci: seed q of the read at seed k of a copy
            if t[0] == "L":
                for k in range(t[2], t[3]):
                    core |= {((x + P * (k - q)) & U64) >> 4 for x in where[t[1]]}
                    q += 1
            else:
                q += t[1]
        out, who, cur = [], [], dict(u=0, r=0)
        for t in toks:
            if t[0] == "L":
                out.append(self.piece[t[1]][P * t[2]:P * t[3]])
                who += [t[1]] * (t[3] - t[2])
                continue
            kind, n = t
            for _ in range(n):
                while True:
                    i = cur[kind]
                    assert i < len(self.pool[kind]), (name, kind, "pool used up")
                    cur[kind] += 1
                    if not any(((x + 1 - P * len(who)) & U64) >> 4 in core for x in where["b%s%d" % (kind, i)]):
                        break
                out.append(self.pool[kind][i] + _spacer(i))
                who.append(kind)
        return dict(name=name, seq=b"".join(out), who=who)

    def small(self, name):
        """The small case a read was lifted from: the read cut behind its last locus (the ballast in front of and between its
        loci stays: it places them)."""
        toks = self.tokens[name]
        last = max(i for i, t in enumerate(toks) if t[0] == "L")
        self.tokens[name + "/small"] = toks[:last + 1]
        try:
            return self._make(name + "/small")
        finally:
            del self.tokens[name + "/small"]

    def build(self):
        if self.ready is not None:
            self.pl = K.Planted(self.ready[0], {}, [])
            self.reads = {nm: dict(name=nm, seq=seq, who=["core"] * (len(seq) // P)) for nm, seq in self.ready[1].items()}
            return self.pl
        n_max = max(sum(t[3] - t[2] if t[0] == "L" else t[1] for t in toks) for toks in self.tokens.values())
        assert P * n_max + 64 <= self.beyond, "a read reaches the first locus"
        loci = [dict(it) for it in self.loci]
        if loci and loci[0]["at"] is None and loci[0]["after"] is None:
            loci[0]["at"] = self.beyond
        order = np.random.default_rng([self.seed, 1]).permutation(len(self.scatter))
        self.pl = K.plant(self.front + loci + [self.scatter[i] for i in order], seed=self.seed % (1 << 31), gap=self.gap)
        self.reads = {name: self._make(name) for name in self.tokens}
        return self.pl


def hit_list(read, cen, sa_rank, phase=0):
    """The hits of one phase (default: phase 0) of a read with their places: [(key, survivor index s, seed ordinal q, suffix-array offset t)] in
    arrival order -- the order key of a hit is (q, t) --, and the hit count of every survivor."""
    hits, rrs = [], []
    read = bytes(read)
    for q, j in enumerate(range(phase, max(len(read) - S, 0), P)):
        pos = cen.positions(read[j:j + S])
        if 0 < len(pos) < THRES:
            for t, x in enumerate(sorted(pos, key=lambda x: sa_rank[x])):
                hits.append(((x - j) & U64, len(rrs), q, t))
            rrs.append(len(pos))
    return hits, rrs


def buckets_of(hits):
    """bucket -> dict(n, first: the hit seen first, low: the hit with the smallest key (the first of them), hits)."""
    out = {}
    for h in hits:
        e = out.setdefault(h[0] >> 4, dict(n=0, first=h, low=h, hits=[]))
        e["n"] += 1
        e["hits"].append(h)
        if h[0] < e["low"][0]:
            e["low"] = h
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the groups: one text each, with its reads and its cases
# ---------------------------------------------------------------------------------------------------------------------
# case: dict(name, group, reads: names, or pick(world) -> (names, limits), prop(world, [derived read], limits))
LIFTS = ("one-pass", "two-pass", "three-pass")
_WANT_PASSES = {"one-pass": 1, "two-pass": 2, "three-pass": 3}


def _tail(lift, uniq_before, rep_before=0):
    """Ballast behind a layout of uniq_before unique-hit seeds and rep_before repeat ballast seeds: repeat ballast first, so
    that one pass, two passes, three passes are reached at 470, 600 and 700 survivors."""
    nr, c = {"one-pass": (30, 470), "two-pass": (100, 600), "three-pass": (200, 700)}[lift]
    return [("u", 1), ("r", nr - rep_before), ("u", c - uniq_before - nr - 1)]


def _lifted(reads, lift):
    for r in reads:
        x = exact_path(r["H"])
        assert fast_path(r["c"]) == "fast-block" and x["tier"] == "block" and x["passes"] == _WANT_PASSES[lift], (r["name"], r["c"], r["H"])
        assert x["cache"] == (lift == "three-pass") and x["table"] == "lds"
        assert exact_path(r["H"], LIMITS)["passes"] == -(-r["H"] // 100) > 2


def _clear_of_ballast(reads):
    for r in reads:
        assert r["ballast_max"] < r["top"][1][1], (r["name"], r["ballast_max"], r["top"])


TIE_PAIRS = {"same-wavefront": (10, 40), "other-wavefront": (10, 100), "other-chunk": (10, 300),
             "thread-order-opposite": (250, 260), "both-in-chunk-1": (300, 420)}


def _g_ties():
    t = Text("ties", 16000)
    x, y = t.segment(10), t.segment(10)
    t.locus("y", y)
    t.locus("x", x, at=16000 + 7000)                    # further apart than 21 seeds x the widest pair: the key order turns with the read
    t.ballast(720, [(220, 8)])
    cases = []
    for label, (p1, p2) in TIE_PAIRS.items():
        for lift in LIFTS:
            names = [t.read("tie-%s-%s-%s" % (label, lift, a + b), ("u", p1), a, ("u", p2 - p1 - 10), b, *_tail(lift, p2 + 10))
                     for a, b in (("x", "y"), ("y", "x"))]

            def prop(w, reads, limits, p1=p1, p2=p2, label=label, lift=lift):
                _lifted(reads, lift)
                _clear_of_ballast(reads)
                for r, (a, b) in zip(reads, (("x", "y"), ("y", "x"))):
                    ka, kb = w["pl"].where[a][0] - P * p1, w["pl"].where[b][0] - P * p2
                    assert r["top"] == [(ka, 10, ka >> 4), (kb, 10, kb >> 4)]                      # the tie exists: first seen wins
                    assert r["buckets"][ka >> 4]["first"][1] == p1 and r["buckets"][kb >> 4]["first"][1] == p2
                # the same two loci in the other order: no fixed order of keys or of rows gives both
                assert (reads[0]["top"][0][0] < reads[0]["top"][1][0]) != (reads[1]["top"][0][0] < reads[1]["top"][1][0])
                assert {"same-wavefront": wave(p1) == wave(p2) and chunk(p1) == chunk(p2),
                        "other-wavefront": wave(p1) != wave(p2) and chunk(p1) == chunk(p2),
                        "other-chunk": chunk(p1) != chunk(p2),
                        "thread-order-opposite": p1 < p2 and thread(p1) > thread(p2),
                        "both-in-chunk-1": chunk(p1) == chunk(p2) == 1}[label]
            cases.append(dict(name="tie-%s-%s" % (label, lift), reads=names, prop=prop))

    # ---- the pass edges, on the three-pass reads: chosen among the ten of them by where the harness puts their top two
    cands = ["tie-%s-three-pass-%s" % (label, o) for label in TIE_PAIRS for o in ("xy", "yx")]

    def pass_case(name, want, chunk1=False):
        def pick(w):
            for nm in cands:
                r = w["read"](nm)
                if chunk1 and chunk(r["buckets"][r["top"][0][2]]["first"][1]) != 1:
                    continue
                for L in L_CHOICES:
                    pd, pl_ = exact_path(r["H"])["passes"], exact_path(r["H"], (L, 512))["passes"]
                    a, b = bucket_passes([r["top"][0][2], r["top"][1][2]], pd), bucket_passes([r["top"][0][2], r["top"][1][2]], pl_)
                    if want(*a) and want(*b):
                        return [nm], (L, 512)
            raise AssertionError("no candidate of %s" % name)

        def prop(w, reads, limits):
            r = reads[0]
            x = exact_path(r["H"])
            assert x["passes"] == 3 and x["cache"] and exact_path(r["H"], limits)["cache"]
            assert r["top"][0][1] == r["top"][1][1] == 10 and r["ballast_max"] < 10
            for ps in (3, exact_path(r["H"], limits)["passes"]):
                assert want(*bucket_passes([r["top"][0][2], r["top"][1][2]], ps)), (name, ps)
            if chunk1:          # the winner's first hit -- its key and order -- is a unique seed's of chunk 1, read back from the scratch
                f = r["buckets"][r["top"][0][2]]["first"]
                assert chunk(f[1]) == 1 and r["rrs"][f[1]] == 1
                assert sum(r["rrs"][:256]) > 0 and r["rrs"][256:f[1]].count(1) > 0               # kbase > 0 and urank > 0 at that seed
        cases.append(dict(name=name, pick=pick, prop=prop))

    pass_case("passes-top-two-in-the-same-pass", lambda a, b: a == b)
    pass_case("passes-tie-winner-in-the-earlier-pass", lambda a, b: a < b)
    pass_case("passes-tie-first-seen-in-the-later-pass", lambda a, b: a > b)
    pass_case("scratch-unique-seed-of-chunk-1-decides-in-a-later-pass", lambda a, b: a >= 1, chunk1=True)
    return t, cases


def _g_second_tie():
    """(test_gpu_vote_rank._second_tie has this edge at counts 1 and 3.  Lifted, neither clears the ballast: the largest ballast
    bucket measured on these reads is 3 -- at count 1 every ballast bucket ties, at 3 some do -- so the tie is planted at 8.)
    Three buckets tied at the second count (8), their first hits in three different wavefronts; `big` (16) in the fourth."""
    t = Text("second-tie", 16000)
    big = t.segment(16)
    th = [t.segment(8) for _ in range(3)]
    t.locus("t2", th[2])
    t.locus("big", big)
    t.locus("t1", th[1])
    t.locus("t0", th[0])
    t.ballast(720, [(220, 8)])
    cases = []
    orders = (("t0", "t1", "t2"), ("t2", "t1", "t0"), ("t1", "t2", "t0"))

    def layout(o, shift=0):
        return [("u", 20 + shift), o[0], ("u", 62), o[1], ("u", 62), o[2], ("u", 32 - shift), "big"]       # first hits: 20, 90, 160 (+ shift); big at 200

    def check(w, r, o, shift=0):
        kb = w["pl"].where["big"][0] - P * 200
        k0 = w["pl"].where[o[0]][0] - P * (20 + shift)
        assert r["top"] == [(kb, 16, kb >> 4), (k0, 8, k0 >> 4)] and r["ballast_max"] < 8
        tied = sorted((e["first"][1], b) for b, e in r["buckets"].items() if e["n"] == 8)
        assert [s for s, _ in tied] == [20 + shift, 90 + shift, 160 + shift] and len({wave(s) for s, _ in tied}) == 3
        assert wave(200) not in {wave(s) for s, _ in tied}
        return [b for _, b in tied]

    for lift in LIFTS:
        names = [t.read("second-tie-%s-%s" % (lift, "".join(x[1] for x in o)), *layout(o), *_tail(lift, 216)) for o in orders]

        def prop(w, reads, limits, lift=lift):
            _lifted(reads, lift)
            for r, o in zip(reads, orders):
                check(w, r, o)
        cases.append(dict(name="three-tied-at-the-second-count-%s" % lift, reads=names, prop=prop))
    # three passes, and the three tied buckets in three different ones: chosen among layouts shifted by whole seeds
    cands = [(t.read("second-tie-shift%d-%s" % (sh, "".join(x[1] for x in o)), *layout(o, sh), *_tail("three-pass", 216)), o, sh)
             for sh in range(1, 9) for o in orders]

    def pick(w):
        for nm, o, sh in cands:
            r = w["read"](nm)
            tied = check(w, r, o, sh)
            if sorted(bucket_passes(tied, 3)) != [0, 1, 2]:
                continue
            for L in L_CHOICES:
                if len(set(bucket_passes(tied, exact_path(r["H"], (L, 512))["passes"]))) == 3:
                    return [nm], (L, 512)
        raise AssertionError("no candidate")

    def prop3(w, reads, limits):
        r = reads[0]
        nm, o, sh = next(c for c in cands if c[0] == r["name"])
        tied = check(w, r, o, sh)
        assert exact_path(r["H"])["passes"] == 3 and sorted(bucket_passes(tied, 3)) == [0, 1, 2]
        assert len(set(bucket_passes(tied, exact_path(r["H"], limits)["passes"]))) == 3
    cases.append(dict(name="passes-three-tied-at-the-second-count-in-three-passes", pick=pick, prop=prop3))
    return t, cases


def _lowers_set(t, tag, n, qr, A, v_first=True):
    """The loci of test_gpu_vote_rank._repeat_hit_lowers for a read that has r at seed qr, v behind it and u behind v: one copy
    of the repeat seed r lies at A + 21 qr, on the diagonal A (A % 16 == 0), and u on the diagonal A + 3 -- the same bucket."""
    r = K.kmers(t.rng, 1)[0]
    v, u = t.segment(n + 1), t.segment(n)
    assert A % 16 == 0
    if v_first:
        t.locus("v" + tag, v)
    t.locus("r" + tag, r, at=A + P * qr, piece=r + b"C")
    t.locus("u" + tag, u, after=("r" + tag, 0, P * (n + 2) + 3))
    if not v_first:
        t.locus("v" + tag, v)
    t.scattered("r" + tag + "~", b"G" + r + b"A")                 # the second copy, in a bucket of its own
    return ["r" + tag, "v" + tag, "u" + tag]


def _check_lowers(w, r, tag, n, qr, A):
    """r's hit on the diagonal A holds the bucket's smallest key and its earliest order; v ties with the bucket and is seen
    before every unique hit of it: that order alone decides.  -> the deciding hit"""
    kv = w["pl"].where["v" + tag][0] - P * (qr + 1)
    assert r["top"] == [(A, n + 1, A >> 4), (kv, n + 1, kv >> 4)] and r["ballast_max"] < n + 1
    e = r["buckets"][A >> 4]
    assert e["first"] == e["low"] and e["first"][0] == A and e["first"][2] == qr and r["rrs"][e["first"][1]] == 2
    rest = [h for h in e["hits"] if h is not e["first"]]
    assert len(rest) == n and all(h[0] == A + 3 and r["rrs"][h[1]] == 1 and h[2] > qr + n + 1 for h in rest)
    assert r["buckets"][kv >> 4]["first"][2] == qr + 1
    # without the repeat seed's hits v would win, and the bucket's key would be A + 3
    assert K.vote_top2([h[0] for h in r["hits"] if h[2] != qr])[1][:2] == [(kv, n + 1, kv >> 4), (A + 3, n, A >> 4)]
    return e["first"]


def _choose_A(lo, passes):
    """The first multiple of 16 from lo on whose bucket is admitted in a pass >= 1 of every one of `passes`."""
    A = (lo + 15) // 16 * 16
    while not all(bucket_passes([A >> 4], ps)[0] >= 1 for ps in passes):
        A += 16
    return A


def _g_lowers():
    """(a): the repeat seed in chunk 0 (seed 5).  (b): in chunk 2 (seed 520) behind two chunks that hold unique and repeat seeds
    both, and behind unique and repeat seeds of its own chunk; the set of (a) is part of these reads too, so that the fast
    form's list has an entry of chunk 0 in front of the one chunk 2 appends."""
    t = Text("lowers", 16000)
    na, nb, qa, qb = 9, 12, 5, 520
    t.ballast(720, [(250, 8)])
    # (b): tokens in front of seed 520, and the tails; H is planned, so that the bucket of A can be chosen by its pass
    head_b = [("u", 5), "ra", "va", "ua", ("u", 125), ("r", 10), ("u", 96), ("u", 100), ("r", 10), ("u", 146), ("u", 4), ("r", 2), ("u", 2)]
    tails_b = {"one-pass": [("u", 10)], "two-pass": [("u", 10), ("r", 60)], "three-pass": [("u", 10), ("r", 180)]}
    tails_a = {lift: _tail(lift, 5 + 1 + 2 * na + 1) for lift in LIFTS}
    # (every r token is 8 hits, every other seed 1, ra / rb 2)
    count = lambda toks: sum(8 * x[1] if isinstance(x, tuple) and x[0] == "r" else x[1] if isinstance(x, tuple) else 0 for x in toks)
    Ha = {lift: count([("u", 5)] + tails_a[lift]) + 2 + 2 * na + 1 for lift in LIFTS}
    Hb = {lift: count(head_b + tails_b[lift]) + (2 + 2 * na + 1) + (2 + 2 * nb + 1) for lift in LIFTS}
    Aa = _choose_A(16000 + 2000, [3, -(-Ha["three-pass"] // 100)])
    set_a = _lowers_set(t, "a", na, qa, Aa)
    Ab = _choose_A(Aa + P * 600, [3, -(-Hb["three-pass"] // 100)])
    set_b = _lowers_set(t, "b", nb, qb, Ab)
    assert sum(x[1] if isinstance(x, tuple) else {"ra": 1, "va": na + 1, "ua": na}[x] for x in head_b) == qb
    cases = []
    for lift in LIFTS:
        na_, nb_ = t.read("lowers-a-" + lift, ("u", 5), *set_a, *tails_a[lift]), t.read("lowers-b-" + lift, *head_b, *set_b, *tails_b[lift])

        def prop(w, reads, limits, lift=lift):
            _lifted(reads, lift)
            ra, rb = reads
            assert (ra["H"], rb["H"]) == (Ha[lift], Hb[lift])
            fa = _check_lowers(w, ra, "a", na, qa, Aa)
            fb = _check_lowers(w, rb, "b", nb, qb, Ab)
            assert chunk(fa[1]) == 0 and chunk(fb[1]) == 2 and fb[1] == qb
            # (b): chunks 0 and 1 hold unique and repeat seeds, and so does chunk 2 in front of the repeat seed: in the key
            # scratch kbase, nuni, urank and the index of the hit among the chunk's repeat hits are all non-zero
            for k in (0, 1):
                part = rb["rrs"][256 * k:256 * k + 256]
                assert min(part) == 1 and max(part) > 1
            assert 1 in rb["rrs"][512:qb] and sum(x for x in rb["rrs"][512:qb] if x > 1) > 0
            # the fast form's list: the entry of (a)'s repeat hit comes from chunk 0, this one from chunk 2
            ea = rb["buckets"][Aa >> 4]["first"]
            assert rb["rrs"][ea[1]] == 2 and chunk(ea[1]) == 0
            if lift == "three-pass":                 # the deciding hit's bucket is voted in a pass >= 1: read back from the scratch
                for r, A in ((ra, Aa), (rb, Ab)):
                    for lim in ((0, 0), limits):
                        x = exact_path(r["H"], lim)
                        assert x["cache"] and x["passes"] >= 3 and bucket_passes([A >> 4], x["passes"])[0] >= 1
        cases.append(dict(name="repeat-hit-lowers-key-and-order-" + lift, reads=[na_, nb_], prop=prop))
    return t, cases


def _g_min_key():
    """The smallest key of a bucket held by a hit of another wavefront than its first hit; low four bits 0 and 15.  Read `far`:
    W = w1 (diagonal D + 15, survivors 10 ..) + w2 (D, survivors 140 ..), Z = z1 (E + 15, 70 ..) + z2 (E, 200 ..).  Read `near`:
    w1 and z1 alone -- every key of either bucket ends in 15."""
    t = Text("min-key", 16000)
    D, E = 16000, 16000 + 8192
    nw, nz = 8, 7
    t.locus("w1", t.segment(nw), at=D + 15 + P * 10)
    t.locus("w2", t.segment(nw), at=D + P * 140)
    t.locus("z1", t.segment(nz), at=E + 15 + P * 70)
    t.locus("z2", t.segment(nz), at=E + P * 200)
    t.ballast(720, [(220, 8)])
    cases = []
    for lift in LIFTS:
        far = t.read("min-key-far-" + lift, ("u", 10), "w1", ("u", 60 - nw), "z1", ("u", 70 - nz), "w2", ("u", 60 - nw), "z2", *_tail(lift, 200 + nz))
        near = t.read("min-key-near-" + lift, ("u", 10), "w1", ("u", 60 - nw), "z1", *_tail(lift, 70 + nz))

        def prop(w, reads, limits, lift=lift):
            _lifted(reads, lift)
            _clear_of_ballast(reads)
            f, n = reads
            assert D % 16 == 0 and E % 16 == 0
            assert f["top"] == [(D, 2 * nw, D >> 4), (E, 2 * nz, E >> 4)]
            for b, s_first, s_low in ((D >> 4, 10, 140), (E >> 4, 70, 200)):
                e = f["buckets"][b]
                assert e["first"][1] == s_first and e["first"][0] & 15 == 15 and e["low"][1] == s_low and e["low"][0] & 15 == 0
                assert wave(s_first) != wave(s_low) and chunk(s_first) == chunk(s_low) == 0
            assert n["top"] == [(D + 15, nw, D >> 4), (E + 15, nz, E >> 4)]
        cases.append(dict(name="minimum-key-from-another-wavefront-" + lift, reads=[far, near], prop=prop))

    # ---- the pass edges with different counts (8 against 7): the top two in two different passes, the winner's in the earlier
    # and in the later one, seen first and seen second -- by three passes and by the chosen limit alike.  Candidates: w1 and z1
    # in either order, shifted by whole seeds (the loci stay where they are, so every shift has diagonals of its own).
    cands = []
    for sh in range(12):
        cands.append((t.read("unequal-wz-%d" % sh, ("u", 10 + sh), "w1", ("u", 52), "z1", *_tail("three-pass", 77 + sh)), "w1"))
        cands.append((t.read("unequal-zw-%d" % sh, ("u", 10 + sh), "z1", ("u", 53), "w1", *_tail("three-pass", 78 + sh)), "z1"))

    def unequal(name, seen_first, want):
        def facts(w, nm):
            r = w["read"](nm)
            ids = [b for _, _, b in r["top"]]
            return r, ids, [t.reads[nm]["who"][r["buckets"][b]["first"][2]] for b in ids], [r["buckets"][b]["first"][1] for b in ids]

        def pick(w):
            for nm, first in cands:
                if (first == "w1") != seen_first:
                    continue
                r, ids, _, _ = facts(w, nm)
                for L in L_CHOICES:
                    if want(*bucket_passes(ids, 3)) and want(*bucket_passes(ids, exact_path(r["H"], (L, 512))["passes"])):
                        return [nm], (L, 512)
            raise AssertionError("no candidate of %s" % name)

        def prop(w, reads, limits):
            r, ids, loci, first = facts(w, reads[0]["name"])
            _lifted(reads, "three-pass")
            assert [x[1] for x in r["top"]] == [nw, nz] and loci == ["w1", "z1"] and r["ballast_max"] < nz
            assert (first[0] < first[1]) == seen_first                       # the winner is seen first / second
            for ps in (3, exact_path(r["H"], limits)["passes"]):
                assert want(*bucket_passes(ids, ps)), (name, ps)
        cases.append(dict(name=name, pick=pick, prop=prop))

    for seen_first in (True, False):
        for label, want in (("earlier", lambda a, b: a < b), ("later", lambda a, b: a > b)):
            unequal("passes-winner-seen-%s-in-the-%s-pass" % ("first" if seen_first else "second", label), seen_first, want)
    return t, cases


def _g_wrapped():
    """test_gpu_vote_rank._wrapped: w at text position 7 behind three seeds of the read -- its keys wrap around 2^64 -- ties with
    the plain bucket b, in both orders."""
    t = Text("wrapped", 16000)
    a, w, b = t.segment(3), t.segment(10), t.segment(10)
    t.locus("w", w, at=7, front=True)
    t.locus("b", b)
    t.locus("a", a)
    t.ballast(720, [(220, 8)])
    cases = []
    for lift in LIFTS:
        names = [t.read("wrapped-%s-%s" % (lift, o[1] + o[2]), *o, *_tail(lift, 23)) for o in (("a", "w", "b"), ("a", "b", "w"))]

        def prop(w_, reads, limits, lift=lift):
            _lifted(reads, lift)
            _clear_of_ballast(reads)
            kw0, kw1 = (7 - P * 3) & U64, (7 - P * 13) & U64
            kb0, kb1 = w_["pl"].where["b"][0] - P * 13, w_["pl"].where["b"][0] - P * 3
            assert kw0 >> 63 == 1 and kw1 >> 63 == 1
            assert reads[0]["top"] == [(kw0, 10, kw0 >> 4), (kb0, 10, kb0 >> 4)]
            assert reads[1]["top"] == [(kb1, 10, kb1 >> 4), (kw1, 10, kw1 >> 4)]
        cases.append(dict(name="wrapped-beside-plain-" + lift, reads=names, prop=prop))
    return t, cases


N_LIST, N_LIST_U, N_LIST_W = FB_LIST + 1, 30, 40


def _g_list():
    """test_gpu_vote_rank._list_case at the list of the fast workgroup form: 513 repeat seeds in front of the unique segment u,
    planted with it as one string -- each has one hit in u's bucket and one in a bucket of its own --, w the second bucket.
    Read `513` is the whole; read `512` leaves the first repeat seed out."""
    t = Text("list", 16000)
    rk = K.kmers(t.rng, N_LIST)
    R, u, w = K.read_of(rk), t.segment(N_LIST_U), t.segment(N_LIST_W)
    t.locus("Ru", R + u, at=16000)
    t.locus("w", w)
    for i in np.random.default_rng(t.seed).permutation(N_LIST):
        f = b"ACGT"[(i + 1) % 4:(i + 1) % 4 + 1]               # (differs from the read's spacers on either side, as in _list_case)
        t.scattered("r%d~" % i, f + rk[i] + f)
    full = t.read("list-513", "Ru", "w")
    less = t.read("list-512", ("L", "Ru", 1, N_LIST + N_LIST_U), "w")
    # a list entry beyond the first 256 decides: 300 repeat seeds of Ru (with u: the top bucket, 330) fill the list in chunks 0
    # and 1; then, at seed 520, the set of _repeat_hit_lowers, whose bucket (45 + 1) is the SECOND entry by its repeat hit alone
    n_l, q_l = 45, 520
    t.ballast(q_l - 330 + 20)
    A = (16000 + P * (N_LIST + N_LIST_U) + 4000) // 16 * 16
    lowers = _lowers_set(t, "l", n_l, q_l, A, v_first=False)
    late = t.read("list-late-entry", ("L", "Ru", N_LIST - 300, N_LIST + N_LIST_U), ("u", q_l - 330), *lowers)

    def prop_late(w_, reads, limits):
        r = reads[0]
        d = 16000 + P * (N_LIST - 300)
        kv = w_["pl"].where["vl"][0] - P * (q_l + 1)
        assert r["c"] == q_l + 1 + 2 * n_l + 1 and r["H"] == r["c"] + 301 and fast_path(r["c"]) == "fast-block"
        assert r["top"] == [(d, 330, d >> 4), (A, n_l + 1, A >> 4)] and r["ballast_max"] < n_l and r["settles"][0]
        e, ev = r["buckets"][A >> 4], r["buckets"][kv >> 4]
        assert e["first"] == e["low"] and e["first"][2] == q_l and r["rrs"][q_l] == 2 and chunk(q_l) == 2
        assert all(h[0] == A + 3 and h[2] > q_l + n_l + 1 for h in e["hits"][1:])
        assert ev["n"] == n_l + 1 and ev["first"][2] == q_l + 1           # v ties with the bucket and is seen before its unique hits
        # its list entry lies behind 300 others, all of earlier chunks: in the second register slot of the list's ranks
        table = {h[0] >> 4 for h in r["hits"] if r["rrs"][h[1]] == 1}
        before = [h for h in r["hits"] if r["rrs"][h[1]] > 1 and h[0] >> 4 in table and h[1] < q_l]
        assert sum(1 for h in before if h[0] == d) == 300 >= 256 and max(chunk(h[1]) for h in before) == 1

    def prop(w_, reads, limits):
        for r, n in zip(reads, (N_LIST, N_LIST - 1)):
            d = 16000 if n == N_LIST else 16000 + P
            assert d % 16 != 15 and r["c"] == n + N_LIST_U + N_LIST_W and r["H"] == 2 * n + N_LIST_U + N_LIST_W
            assert fast_path(r["c"]) == "fast-block" and exact_path(r["H"])["passes"] == 2
            assert r["top"][0] == (d, n + N_LIST_U, d >> 4) and r["top"][1][1] == N_LIST_W
            in_table = [h for h in r["hits"] if r["rrs"][h[1]] == 2 and h[0] >> 4 == d >> 4]
            assert len(in_table) == n and {chunk(h[1]) for h in in_table} == set(range(-(-n // 256)))      # the list entries, appended chunk by chunk
            assert r["repeat_only_max"] < N_LIST_W
            assert r["settles"][0] == (n <= FB_LIST), r["settles"]
        assert reads[0]["settles"][1].startswith("list") and reads[1]["settles"][1].startswith(("sketch", "counting"))
    return t, [dict(name="list-at-512-and-513", reads=[full, less], prop=prop),
               dict(name="list-entry-beyond-256-decides", reads=[late], prop=prop_late)]


BOUNDARY_C = (193, 256, 257, 768, 769, 1536, 1537)


def _g_boundaries():
    """Items of c unique survivors, H = c hits: the survivor limits of the fast forms (193, 256 / 257: one and two register
    slots, 1536 / 1537) and the pass limits of the exact tier (768 / 769: one and two passes, 1536 / 1537: two passes and three
    with the key scratch), with different counts on the two entries.  No repeat seed: no sketch is cleared or scanned."""
    t = Text("boundaries", 1537 * P + 64)
    t.locus("y", t.segment(10))
    t.locus("x", t.segment(12))
    t.ballast(1537 - 22 + 40)
    names = [t.read("survivors-%d" % c, "x", "y", ("u", c - 22)) for c in BOUNDARY_C]

    def prop(w, reads, limits):
        for r, c in zip(reads, BOUNDARY_C):
            kx, ky = w["pl"].where["x"][0], w["pl"].where["y"][0] - P * 12
            assert r["c"] == r["H"] == c and set(r["rrs"]) == {1}
            assert r["top"] == [(kx, 12, kx >> 4), (ky, 10, ky >> 4)]
            assert r["ballast_max"] < 10 and r["settles"] == ((c <= FB_LIMIT), "no repeat seed" if c <= FB_LIMIT else "more than 1536 survivors")
            assert fast_path(c) == ("fast-block" if c <= FB_LIMIT else "exact")
            x = exact_path(c)
            assert (x["passes"], x["cache"]) == {193: (1, False), 256: (1, False), 257: (1, False), 768: (1, False), 769: (2, False),
                                                 1536: (2, False), 1537: (3, True)}[c]
    return t, [dict(name="survivor-and-pass-boundaries", reads=names, prop=prop)]


SKETCH_A, SKETCH_B = 20, 10


def _g_sketch():
    """A repeat-only bucket of count m, seen first (the block rb of m seeds is planted twice: two such buckets), against the
    table's second count b = 10, at c >= 193: m = b - 1, b, b + 1.  With m = b the item's true second entry is the repeat-only
    bucket: a kernel that settled it would write the wrong key2 / bucket2."""
    t = Text("sketch", 8000)
    ms = (SKETCH_B - 1, SKETCH_B, SKETCH_B + 1)
    t.locus("ub", t.segment(SKETCH_B))
    for m in ms:
        t.locus("rb%d" % m, t.segment(m))
    t.locus("ua", t.segment(SKETCH_A))
    for m in ms:
        t.locus("rb%d" % m, t.piece["rb%d" % m])
    t.ballast(220)
    names = [t.read("sketch-m=%d" % m, "rb%d" % m, "ua", "ub", ("u", 200)) for m in ms]

    def prop(w, reads, limits):
        for r, m in zip(reads, ms):
            assert r["c"] == m + 230 and r["H"] == r["c"] + m and fast_path(r["c"]) == "fast-block" and exact_path(r["H"])["passes"] == 1
            ka, kb = w["pl"].where["ua"][0] - P * m, w["pl"].where["ub"][0] - P * (m + SKETCH_A)
            alone = sorted(w["pl"].where["rb%d" % m], key=lambda x: r["keys"].index(x))            # the two copies, in arrival order
            assert r["top"][0] == (ka, SKETCH_A, ka >> 4) and r["ballast_max"] < SKETCH_B - 1
            assert all(r["buckets"][k >> 4]["n"] == m and r["buckets"][k >> 4]["first"][1] == 0 for k in alone)
            if m >= SKETCH_B:          # seen first, it is the second entry; counting decides: a repeat-only bucket >= b
                assert r["top"][1] == (alone[0], m, alone[0] >> 4)
                assert r["settles"][0] is False and r["settles"][1].startswith("counting")
            else:                      # 2 m >= b repeat-only hits: counting does not decide, the harness's sketch counters do
                assert r["top"][1] == (kb, SKETCH_B, kb >> 4) and 2 * m >= SKETCH_B
                assert r["settles"] == (True, "sketch: M = %d against %d" % (m, SKETCH_B))
            # every phase is voted (30 votes of 240 seeds decide none), so the read's redo items are known phase by phase: in phase
            # 0 m = b - 1 hands on nothing, m = b and b + 1 one item each; the later phases (the loci lose a seed at either end,
            # not all in the same phase) follow the same rule on their own brute-force hits
            assert len(r["redo_items"]) == P and r["redo_items"][0] == (0 if m < SKETCH_B else 1), (m, r["redo_items"])
    return t, [dict(name="sketch-against-the-second-count", reads=names, prop=prop)]


def _g_no_unique():
    """constructed.vote_case("no-unique-seed") at 200 survivors: r1 (120 seeds, two copies) and r2 (80 seeds, three copies).  The
    fast table stays empty, there is no second count to compare the sketch with, and the item goes to the exact kernel."""
    c = K.vote_case("no-unique-seed", 20)
    t = Text("no-unique", len(c["read"]) + 64, ready=(c["seq"], {"no-unique-seed-200": c["read"]}))

    def prop(w, reads, limits):
        r = reads[0]
        assert r["c"] == 200 and r["H"] == 120 * 2 + 80 * 3 and min(r["rrs"]) >= 2 and r["top"][0][1] == 120
        assert fast_path(r["c"]) == "fast-block" and exact_path(r["H"])["passes"] == 1
        assert r["settles"] == (False, "counting: a repeat-only bucket of 120 >= 0")
    return t, [dict(name="no-unique-seed-at-200-survivors", reads=["no-unique-seed-200"], prop=prop)]


G_REP, G_COPIES, G_TOP = 60, 270, 40


def _g_global():
    """Items around and beyond the key scratch's 16384 hits: 60 repeat ballast k-mers of 270 scattered copies each and top twos
    planted at 40.  Above 16384 hits the exact kernel votes in one pass into a table in global memory; under debug limits in
    ceil(H / 100) passes over the LDS table, with neither scratch nor global table."""
    n = G_TOP
    t = Text("global", 8192, gap=(10, 30))
    a, w = t.segment(3), t.segment(n)
    t.locus("w", w, at=7, front=True)
    t.locus("y", t.segment(n))
    t.locus("x", t.segment(n))
    t.locus("b", t.segment(n))
    t.locus("a", a)
    t.ballast(160, [(G_REP + 15, G_COPIES)])
    hits_r = G_REP * G_COPIES
    A = _choose_A(8192 + 8192, [2])
    lowers = _lowers_set(t, "g", n, 5, A, v_first=False)
    cases = []

    def all_clear(reads):
        _clear_of_ballast(reads)
        for r in reads:
            assert fast_path(r["c"]) == "fast-block", r["c"]

    # the tie of `ties`, first hits at survivors 10 and 100, at H = 16384 (22 passes, the scratch full to its last entry),
    # 16385 (the first item of the global table) -- and in the other arrival order
    u_tail = KC_CAP - hits_r - (10 + n + 50 + n)
    ties = [t.read("global-tie-xy-16384", ("u", 10), "x", ("u", 50), "y", ("u", u_tail), ("r", G_REP)),
            t.read("global-tie-xy-16385", ("u", 10), "x", ("u", 50), "y", ("u", u_tail + 1), ("r", G_REP)),
            t.read("global-tie-yx-16385", ("u", 10), "y", ("u", 50), "x", ("u", u_tail + 1), ("r", G_REP))]

    def prop_tie(w_, reads, limits):
        all_clear(reads)
        assert [r["H"] for r in reads] == [KC_CAP, KC_CAP + 1, KC_CAP + 1]
        assert exact_path(KC_CAP) == dict(tier="block", passes=22, cache=True, table="lds")
        assert exact_path(KC_CAP + 1) == dict(tier="block", passes=1, cache=False, table="global")
        assert exact_path(KC_CAP + 1, limits) == dict(tier="block", passes=164, cache=False, table="lds")
        for r, (p, q) in zip(reads, (("x", "y"), ("x", "y"), ("y", "x"))):
            kp, kq = w_["pl"].where[p][0] - P * 10, w_["pl"].where[q][0] - P * 100
            assert r["top"] == [(kp, n, kp >> 4), (kq, n, kq >> 4)]
            assert r["buckets"][kp >> 4]["first"][1] == 10 and r["buckets"][kq >> 4]["first"][1] == 100
    cases.append(dict(name="global-table-tie-at-16384-and-16385", reads=ties, prop=prop_tie))

    low = t.read("global-lowers", ("u", 5), *lowers, ("u", 100), ("r", G_REP))

    def prop_low(w_, reads, limits):
        all_clear(reads)
        r = reads[0]
        assert exact_path(r["H"])["table"] == "global" and exact_path(r["H"], limits)["table"] == "lds"
        _check_lowers(w_, r, "g", n, 5, A)
    cases.append(dict(name="global-table-repeat-hit-lowers-key-and-order", reads=[low], prop=prop_low))

    wr = [t.read("global-wrapped-" + o[1] + o[2], *o, ("u", 120), ("r", G_REP)) for o in (("a", "w", "b"), ("a", "b", "w"))]

    def prop_wr(w_, reads, limits):
        all_clear(reads)
        kw0, kw1 = (7 - P * 3) & U64, (7 - P * (3 + n)) & U64
        kb0, kb1 = w_["pl"].where["b"][0] - P * (3 + n), w_["pl"].where["b"][0] - P * 3
        assert all(exact_path(r["H"])["table"] == "global" for r in reads)
        assert reads[0]["top"] == [(kw0, n, kw0 >> 4), (kb0, n, kb0 >> 4)] and reads[1]["top"] == [(kb1, n, kb1 >> 4), (kw1, n, kw1 >> 4)]
    cases.append(dict(name="global-table-wrapped-beside-plain", reads=wr, prop=prop_wr))
    return t, cases


GROUPS = {"ties": _g_ties, "second-tie": _g_second_tie, "lowers": _g_lowers, "min-key": _g_min_key, "wrapped": _g_wrapped,
          "list": _g_list, "boundaries": _g_boundaries, "sketch": _g_sketch, "no-unique": _g_no_unique, "global": _g_global}


@functools.lru_cache(maxsize=None)
def group(name):
    t, cases = GROUPS[name]()
    for c in cases:
        c["group"] = name
    return t, cases


def _names():
    out = []
    for g in GROUPS:
        out += [(g, c["name"]) for c in group(g)[1]]
    return out


CASES = _names()                                      # (group, case name)
MAX_TEXT = 1_200_000


# ---------------------------------------------------------------------------------------------------------------------
# the CPU side: the text's index, and per read everything the device must return
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(gname):
    """The group's text with its index, the census and the oracle; w["read"](name): the derived read, computed once."""
    import orc
    from longreadmapper_amd import index
    t, cases = group(gname)
    pl = t.build()
    assert len(pl.seq) <= MAX_TEXT, len(pl.seq)
    hi = index.HostIndex.build([np.frombuffer(bytes(pl.seq), dtype=np.uint8)], hlen=HLEN)
    assert bytes(hi.content()) == K.index_text([pl.seq])
    K.check_sa(hi.content(), hi.sa())
    cen = K.census(hi.content(), S)
    sa = hi.sa().astype(np.int64)
    rank = np.empty(len(sa), dtype=np.int64)
    rank[sa] = np.arange(len(sa))
    oi = orc.OracleIndex.from_host_index(hi)
    derived = {}

    def read(name):
        if name not in derived:
            derived[name] = _derive(t.reads[name], cen, rank, oi)
        return derived[name]
    return dict(text=t, pl=pl, hi=hi, cen=cen, rank=rank, oi=oi, read=read, cases={c["name"]: c for c in cases})


def _derive(rd, cen, rank, oi):
    """Phase 0 by brute force, every phase the oracle runs from its trace (the two agree on phase 0), c and H from the trace."""
    seq = rd["seq"]
    hits, rrs = hit_list(seq, cen, rank)
    keys = [h[0] for h in hits]
    assert keys == K.phase0_hits(seq, S, THRES, cen, rank)
    top = K.vote_top2(keys)[1]
    tr = oi.seed_read(bytes(seq), S, THRES, trace=True)
    rec = tr["phase_recs"][0]
    assert rec["iter"] == 0 and [rec["top1"], rec["top2"]] == top, (rd["name"], rec, top)
    surv = [rr for j, rr, _, _ in sorted(tr["seeds"]) if j % P == 0 and 0 < rr < THRES]
    assert surv == rrs                                           # the path model's inputs come from the trace
    bk = buckets_of(hits)
    who = rd["who"]
    ballast = [e["n"] for e in bk.values() if all(who[h[2]] in ("u", "r") for h in e["hits"])]
    alone = [e["n"] for e in bk.values() if all(rrs[h[1]] > 1 for h in e["hits"])]
    # the items of the read the fast kernels hand to the exact kernel, phase by phase.  The device votes phase 0 of every read
    # and the later phases of a read that phase 0 does not decide; a later phase without a repeat seed (and with at most 1536
    # survivors) settles whatever it holds, one with repeat seeds is put to the same rule as phase 0 (settles) on its
    # brute-force hits.  redo_items is None where the oracle stops between phase 1 and the last: rounds may vote further.
    st0 = settles(hits, rrs)
    recs = tr["phase_recs"]
    redo_items = [0 if st0[0] else 1]
    if len(recs) == P and not recs[0]["decided"]:
        for p in range(1, P):
            prr = [rr for j, rr, _, _ in sorted(tr["seeds"]) if j % P == p and 0 < rr < THRES]
            if not prr:
                redo_items.append(0)
            elif max(prr) == 1:
                redo_items.append(0 if len(prr) <= FB_LIMIT else 1)
            else:
                ph, prr2 = hit_list(seq, cen, rank, p)
                assert prr2 == prr
                redo_items.append(0 if settles(ph, prr2)[0] else 1)
    elif not (len(recs) == 1 and recs[0]["decided"]):
        redo_items = None
    return dict(name=rd["name"], seq=seq, hits=hits, keys=keys, rrs=rrs, c=len(surv), H=sum(surv), top=top, trace=tr, buckets=bk,
                ballast_max=max(ballast, default=0), repeat_only_max=max(alone, default=0), settles=st0, redo_items=redo_items)


def top_loci(hits, who):
    """The top two of a hit stream by brute force, as [(count, the tokens its hits come from)]."""
    top = K.vote_top2([h[0] for h in hits])[1]
    bk = buckets_of(hits)
    return [(n, sorted({who[h[2]] for h in bk[b]["hits"]})) for _, n, b in top if n]


def words(rec_or_top):
    """The six words of a phase record: key, count, bucket of the first and of the second entry."""
    return np.array([x for e in rec_or_top for x in e], dtype=np.uint64)


def expected(r):
    """What the device must leave for a derived read: {phase: six words} (phase 0 from brute force, the later phases from the
    oracle's trace) and best."""
    out = {rec["iter"]: words([rec["top1"], rec["top2"]]) for rec in r["trace"]["phase_recs"]}
    out[0] = words(r["top"])
    return out, r["trace"]["best"]


def resolve(gname, cname):
    """The case ready for a test: dict(name, reads: derived, limits, prop: the predicate, redo: the (read, phase) items the fast
    kernels must hand to the exact kernel (_derive; None where the oracle's phases do not say which phases the device votes))."""
    w = world(gname)
    c = w["cases"][cname]
    names, limits = c["pick"](w) if "pick" in c else (c["reads"], LIMITS)
    reads = [w["read"](n) for n in names]

    def predicate():
        c["prop"](w, reads, limits)
    redo = None if any(r["redo_items"] is None for r in reads) else sum(sum(r["redo_items"]) for r in reads)
    return dict(name=cname, group=gname, reads=reads, limits=limits, predicate=predicate, redo=redo)
