"""The fast vote kernels' count-only table and rank step (vote_kernels.hip: FastTable, "the rank step") on constructed items.

Every case is a small planted text and a few reads whose phase-0 hit stream is known by construction.  What the vote
kernels leave per (read, phase) -- key, count and bucket of BOTH entries (lrm_debug_vote_results) -- is compared

  * through the fast kernels against the exact kernel alone (vote_exact_only = 1),
  * and both against the CPU oracle's trace of every phase it executes, and in phase 0 against the brute-force
    reference of tests/constructed.py (census + vote_top2), which knows nothing of either.

Before anything runs on the device, the CPU side checks that each case has the property it is named for (the tie exists,
the repeat hit really has the smaller key and the earlier order, the list really overflows, ...)."""
import numpy as np
import pytest

import constructed as K
import orc
from longreadmapper_amd import index, mapper

pytestmark = pytest.mark.gpu

S, THRES = 20, 300
T1_LIMIT = 192          # LRM_VOTE_T1_LIMIT: survivors of the largest item of the wavefront form
FAST_LIST = 64          # LRM_VOTE_FAST_LIST: repeat-seed hits in table buckets the wavefront form keeps per item


def _rows(reads):
    arr = np.zeros((len(reads), max(len(r) for r in reads) + 1), dtype=np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return arr, np.array([len(r) for r in reads], dtype=np.uint32)


def _tie(rng):
    """Two buckets of 10 votes each; read 0 meets x first, read 1 meets y first.  y lies first in the text."""
    x, y, z = K.segment(rng, 10), K.segment(rng, 10), K.segment(rng, 3)
    reads = [x + y + z, y + x + z]
    pl = K.plant([dict(name="y", seq=y, at=len(reads[0]) + 64), dict(name="z", seq=z), dict(name="x", seq=x)], seed=1)

    def prop(tops, streams):
        assert [t[1] for t in tops[0]] == [10, 10] and [t[1] for t in tops[1]] == [10, 10]
        assert tops[0][0][0] == pl.where["x"][0] and tops[0][1][0] == pl.where["y"][0] - len(x)
        assert tops[1][0][0] == pl.where["y"][0] and tops[1][1][0] == pl.where["x"][0] - len(y)
    return pl.seq, reads, prop, None


def _second_tie(rng):
    """Three buckets tied at the second count: count 1 (read 0) and count 3 (read 1); the first seen is the second."""
    big = K.segment(rng, 8)
    ones = [K.segment(rng, 1) for _ in range(3)]
    threes = [K.segment(rng, 3) for _ in range(3)]
    reads = [big + b"".join(ones), threes[0] + big + threes[1] + threes[2]]
    spec = [dict(name="o2", seq=ones[2], at=len(reads[1]) + 64), dict(name="t2", seq=threes[2]), dict(name="big", seq=big),
            dict(name="t1", seq=threes[1]), dict(name="o0", seq=ones[0]), dict(name="t0", seq=threes[0]), dict(name="o1", seq=ones[1])]
    pl = K.plant(spec, seed=2)

    def prop(tops, streams):
        assert [t[1] for t in tops[0]] == [8, 1] and tops[0][1][0] == pl.where["o0"][0] - len(big)
        assert sorted(K.vote_top2(streams[0][9:])[1][i][1] for i in range(2)) == [1, 1]        # ... and two more behind it
        assert [t[1] for t in tops[1]] == [8, 3] and tops[1][1][0] == pl.where["t0"][0]
        rest = [k for k in streams[1] if k >> 4 not in (tops[1][0][2], tops[1][1][2])]
        assert [t[1] for t in K.vote_top2(rest)[1]] == [3, 3]
    return pl.seq, reads, prop, None


def _repeat_hit_lowers(rng):
    """The repeat seed r opens the read; one of its two copies lies 3 below the diagonal of the unique segment u, in u's
    bucket: that hit has the bucket's smallest key and its earliest order.  v ties with that bucket at 6 votes and is seen
    before every unique hit of u, so the repeat hit's order alone decides."""
    n = 5
    r = K.kmers(rng, 1)[0]
    v, u = K.segment(rng, n + 1), K.segment(rng, n)
    read = r + b"C" + v + u
    A = 2048
    ju = 21 + len(v)
    pl = K.plant([dict(name="v", seq=v, at=len(read) + 64), dict(name="r", seq=r, at=A), dict(name="u", seq=u, after=("r", 0, ju + 3)),
                  dict(name="r", seq=r)], seed=3)

    def prop(tops, streams):
        keys = streams[0]
        assert sorted(keys[:2]) == sorted(pl.where["r"]) and keys[2:2 + n + 1] == [pl.where["v"][0] - 21] * (n + 1)
        assert keys[2 + n + 1:] == [A + 3] * n and A % 16 == 0
        assert tops[0] == [(A, n + 1, A >> 4), (pl.where["v"][0] - 21, n + 1, (pl.where["v"][0] - 21) >> 4)]
        # without the repeat seed's hits v would win, and the bucket's key would be A + 3
        assert K.vote_top2(keys[2:])[1] == [tops[0][1], (A + 3, n, A >> 4)]
    return pl.seq, [read], prop, None


def _list_case(n_rep):
    def make(rng):
        """n_rep repeat seeds in front of the unique segment u, planted with it as one string: each has one hit in u's bucket
        and one in a bucket of its own (its second copies are scattered).  w is the second bucket, far above any
        repeat-only bucket, so the item settles in the fast kernel if and only if the list holds its n_rep entries."""
        rk = K.kmers(rng, n_rep)
        R, u, w = K.read_of(rk), K.segment(rng, 5), K.segment(rng, 6)
        read = R + u + w
        spec = [dict(name="Ru", seq=R + u, at=len(read) + 64 - (len(read) + 64) % 16), dict(name="w", seq=w)]
        # (the second copies carry a base on either side that differs from the read's spacers there, so that no seed of
        #  another phase -- a k-mer across a spacer -- gains a second occurrence)
        flank = lambda i: b"ACGT"[(i + 1) % 4:(i + 1) % 4 + 1]
        spec += [dict(name="r%d" % i, seq=flank(i) + rk[i] + flank(i)) for i in rng.permutation(n_rep)]
        pl = K.plant(spec, seed=4)

        def prop(tops, streams):
            d = pl.where["Ru"][0]
            assert tops[0][0] == (d, n_rep + 5, d >> 4) and tops[0][1][1] == 6
            in_table = [k for k in streams[0][:2 * n_rep] if k >> 4 == d >> 4]
            assert len(in_table) == n_rep                          # the list entries of the item
            alone = [k for k in streams[0][:2 * n_rep] if k >> 4 != d >> 4]
            assert K.vote_top2(alone)[1][0][1] <= 3                # repeat-only buckets stay far below w's 6 votes
        return pl.seq, [read], prop, (0 if n_rep <= FAST_LIST else 1)
    return make


def _wrapped(rng):
    """w lies at text position 7 behind three seeds of the read: its keys wrap around 2^64.  c votes for key 5 (bucket 0),
    b ties with w and is seen later.  Wrapped and plain buckets side by side."""
    a, w, b, c = K.segment(rng, 3), K.segment(rng, 5), K.segment(rng, 5), K.segment(rng, 4)
    reads = [a + w + b + c, a + b + w + c]
    jc = len(a + w + b)
    pl = K.plant([dict(name="w", seq=w, at=7), dict(name="c", seq=c, at=jc + 5), dict(name="b", seq=b, at=len(reads[0]) + 64),
                  dict(name="a", seq=a)], seed=5)

    def prop(tops, streams):
        kw = (7 - len(a)) & K.U64
        assert kw >> 63 == 1 and 5 in streams[0] and 5 in streams[1]
        assert tops[0][0] == (kw, 5, kw >> 4) and tops[0][1][1] == 5 and tops[0][1][0] == pl.where["b"][0] - len(a + w)
        kw1 = (7 - len(a + b)) & K.U64
        assert tops[1][0][0] == pl.where["b"][0] - len(a) and tops[1][1] == (kw1, 5, kw1 >> 4)
    return pl.seq, reads, prop, None


def _limit(rng):
    """Items of exactly T1_LIMIT survivors (the wavefront form) and of one more (the workgroup form); twelve of them are
    repeat seeds."""
    x, y, y1, rb = K.segment(rng, 100), K.segment(rng, T1_LIMIT - 112), K.segment(rng, 1), K.segment(rng, 12)
    reads = [x + rb + y, x + rb + y + y1]
    pl = K.plant([dict(name="y", seq=y + y1, at=len(reads[1]) + 64), dict(name="rb", seq=rb), dict(name="x", seq=x),
                  dict(name="rb", seq=rb)], seed=6)

    def prop(tops, streams):
        assert [t[1] for t in tops[0]] == [100, T1_LIMIT - 112] and [t[1] for t in tops[1]] == [100, T1_LIMIT - 111]

    def survivors(surv):
        assert [len(x) for x in surv] == [T1_LIMIT, T1_LIMIT + 1]
    return pl.seq, reads, prop, None, survivors


def _second_chunk(rng):
    """102 survivors: 64 unique seeds fill the first chunk of 64, the 24 repeat seeds (two hits each) follow in the second,
    then 14 unique ones -- 126 hits, one item of the wavefront tier.  The first chunk stages nothing, so the repeat seeds
    are staged by the second call of the chunk loop and the third rewrites the terminator behind them (appending behind
    an earlier chunk's repeat seeds is "list-overflow": 64 in the first chunk, the 65th in the second).
    The bucket w gets 12 votes: one hit each of ra (5 seeds, diagonal A + 3; ra[0] is survivor 64, the bucket's first hit)
    and of rb (5 seeds, diagonal A: the bucket's smallest key) and two unique seeds (A + 5).  x ties with it at 12 unique votes and is first seen at survivor 90: w wins by ra[0]'s order alone, with rb's key."""
    c = [K.segment(rng, 8) for _ in range(8)]
    ra, rb, rc = K.kmers(rng, 5), K.kmers(rng, 5), K.kmers(rng, 14)
    w, x = K.segment(rng, 2), K.segment(rng, 12)
    Ra, Rb, Rc = K.read_of(ra), K.read_of(rb), K.read_of(rc)
    read = b"".join(c) + Ra + Rc + Rb + w + x
    ja = len(b"".join(c))
    jb, jw = ja + len(Ra + Rc), ja + len(Ra + Rc + Rb)
    A = 4096
    assert A > len(read) + 64 and A % 16 == 0
    # (second copies as in _list_case: a base on either side that differs from the read's spacers there)
    flank = lambda i: b"ACGT"[(i + 1) % 4:(i + 1) % 4 + 1]
    spec = [dict(name="c%d" % i, seq=c[i], at=64 if i == 0 else None) for i in range(8)]
    spec += [dict(name="x", seq=x, at=3000), dict(name="Ra", seq=Ra, at=A + 3 + ja), dict(name="Rb", seq=Rb, at=A + jb), dict(name="w", seq=w, at=A + 5 + jw)]
    spec += [dict(name="r%d" % i, seq=flank(i) + k + flank(i), copies=1 if i < 10 else 2) for i, k in enumerate(ra + rb + rc)]
    pl = K.plant(spec, seed=8)

    def prop(tops, streams):
        assert len(streams[0]) == 78 + 2 * 24
        kx = pl.where["x"][0] - (jw + len(w))
        assert tops[0] == [(A, 12, A >> 4), (kx, 12, kx >> 4)]
        in_w = [(i, k) for i, k in enumerate(streams[0]) if k >> 4 == A >> 4]
        assert len(in_w) == 12 and in_w[0][1] == A + 3 and 64 <= in_w[0][0] < 66        # first seen: a hit of ra[0], survivor 64
        assert sorted(k for _, k in in_w) == [A] * 5 + [A + 3] * 5 + [A + 5] * 2
        # without the repeat seeds' hits x would win
        assert K.vote_top2([k for k in streams[0] if k >> 4 != A >> 4 or k == A + 5])[1][0] == (kx, 12, kx >> 4)

    def survivors(surv):
        assert len(surv[0]) == 102 and sum(surv[0]) == 126 and 126 <= T1_LIMIT
        assert [i for i, rr in enumerate(surv[0]) if rr > 1] == list(range(64, 88))    # every repeat seed in the second chunk
        assert all(rr == 2 for rr in surv[0][64:88])
    return pl.seq, [read], prop, 0, survivors


def _no_repeat(rng):
    x, y, z = K.segment(rng, 6), K.segment(rng, 4), K.segment(rng, 4)
    read = x + y + z
    pl = K.plant([dict(name="z", seq=z, at=len(read) + 64), dict(name="x", seq=x), dict(name="y", seq=y)], seed=7)

    def prop(tops, streams):
        assert len(streams[0]) == 14 and len(set(streams[0])) == 3 and [t[1] for t in tops[0]] == [6, 4]
    return pl.seq, [read], prop, 0


def _only_repeats(rng):
    c = K.vote_case("no-unique-seed")

    def prop(tops, streams):
        assert len(streams[0]) == 6 * 2 + 4 * 3 and tops[0][0][1] == 6
    return c["seq"], [c["read"]], prop, "some"


CASES = {"tie-both-arrival-orders": _tie, "three-tied-at-the-second-count": _second_tie,
         "repeat-hit-lowers-key-and-order": _repeat_hit_lowers, "list-at-capacity": _list_case(FAST_LIST),
         "list-overflow": _list_case(FAST_LIST + 1), "wrapped-next-to-plain": _wrapped, "t1-limit-and-one-more": _limit,
         "no-repeat-seed": _no_repeat, "only-repeat-seeds": _only_repeats, "repeat-seeds-in-the-second-chunk": _second_chunk}


def _cpu_side(name):
    """The case with its references, computed once: brute force in phase 0, the oracle's trace in every phase it runs."""
    import zlib
    seq, reads, prop, redo, *survivors = CASES[name](np.random.default_rng(zlib.crc32(name.encode())))
    hi = index.HostIndex.build([np.frombuffer(bytes(seq), dtype=np.uint8)], hlen=8)
    assert bytes(hi.content()) == K.index_text([seq])
    K.check_sa(hi.content(), hi.sa())
    cen = K.census(hi.content(), S)
    sa = hi.sa()
    rank = np.empty(len(sa), dtype=np.int64)
    rank[sa.astype(np.int64)] = np.arange(len(sa))
    oi = orc.OracleIndex.from_host_index(hi)
    streams = [K.phase0_hits(r, S, THRES, cen, rank) for r in reads]
    tops = [K.vote_top2(s)[1] for s in streams]
    traces = [oi.seed_read(bytes(r), S, THRES, trace=True) for r in reads]
    for t, tr in zip(tops, traces):
        rec = tr["phase_recs"][0]
        assert rec["iter"] == 0 and [rec["top1"], rec["top2"]] == t          # the two references agree
    prop(tops, streams)
    for check in survivors:                  # the hit counts of the phase-0 survivors of every read, in seed order
        check([[rr for j, rr, _, _ in sorted(tr["seeds"]) if j % (S + 1) == 0 and 0 < rr < THRES] for tr in traces])
    return dict(hi=hi, reads=reads, tops=tops, traces=traces, redo=redo)


_cache = {}


def _vote(di, gpu, reads, exact, with_best=False):
    """-> the six words of every (read, phase), vote_redo_items; with_best: best[] of the same call between them"""
    import torch
    arr, lens = _rows(reads)
    di.set_map_options(vote_exact_only=exact)
    dm = mapper.DeviceMapper(di, len(reads), int(lens.max()), S, THRES, device=gpu)
    try:
        dev = torch.device("cuda", gpu)
        dm.seed(torch.from_numpy(arr).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev))
        torch.cuda.synchronize(dev)
        votes, redo = dm.debug_vote_results(len(reads)), dm.stats()["vote_redo_items"]
        if with_best:
            return votes, dm.best[:len(reads)].cpu().numpy().reshape(-1).view(mapper.ENTRY_DT), redo
        return votes, redo
    finally:
        dm.close()


@pytest.mark.parametrize("name", list(CASES))
def test_vote_rank(gpu, name):
    if name not in _cache:
        _cache[name] = _cpu_side(name)
    c = _cache[name]
    di = index.DeviceIndex.upload(c["hi"], gpu)
    try:
        fast, redo = _vote(di, gpu, c["reads"], 0)
        exact, redo_exact = _vote(di, gpu, c["reads"], 1)
    finally:
        di.close()
    assert redo_exact == 0
    for i, (top, tr) in enumerate(zip(c["tops"], c["traces"])):
        want0 = np.array([x for e in top for x in e], dtype=np.uint64)
        for what, got in (("fast", fast), ("exact", exact)):
            assert np.array_equal(got[i, 0], want0), (name, what, i, got[i, 0].tolist(), want0.tolist())
            for rec in tr["phase_recs"]:
                want = np.array(list(rec["top1"]) + list(rec["top2"]), dtype=np.uint64)
                assert np.array_equal(got[i, rec["iter"]], want), (name, what, i, rec["iter"], got[i, rec["iter"]].tolist(), want.tolist())
    # items the fast kernels handed to the exact one: none, the one phase-0 item the case is about, or (a read made of
    # repeats: every phase of it) at least one
    if c["redo"] == "some":
        assert redo >= 1
    elif c["redo"] is not None:
        assert redo == c["redo"], (name, redo)


def test_keys_beyond_the_32_bit_identity(gpu):
    """The index format holds suffix-array values up to 2^40.  With those of the tie case shifted by 2^35 (a multiple of 16:
    every key and bucket moves along, counts and order stay) no key has a 32-bit bucket name any more: the fast kernels
    must leave every such item to the exact kernel, and the result is the shifted one."""
    if "tie-both-arrival-orders" not in _cache:
        _cache["tie-both-arrival-orders"] = _cpu_side("tie-both-arrival-orders")
    c = _cache["tie-both-arrival-orders"]
    shift = 1 << 35
    seq = bytes(c["hi"].content())[:(len(c["hi"].content()) - 1) // 2]
    hi = index.HostIndex.build([np.frombuffer(seq, dtype=np.uint8)], hlen=8)
    raw = hi.sa_raw()
    raw += np.uint64(shift)
    assert int(hi.sa().min()) >= shift
    oi = orc.OracleIndex.from_host_index(hi)
    want = [np.array([x for key, n, bucket in top for x in (key + shift, n, (key + shift) >> 4)], dtype=np.uint64) for top in c["tops"]]
    for r, w in zip(c["reads"], want):
        rec = oi.seed_read(bytes(r), S, THRES, trace=True)["phase_recs"][0]
        assert rec["iter"] == 0 and list(rec["top1"]) + list(rec["top2"]) == w.tolist()
    di = index.DeviceIndex.upload(hi, gpu)
    try:
        fast, redo = _vote(di, gpu, c["reads"], 0)
        exact, _ = _vote(di, gpu, c["reads"], 1)
    finally:
        di.close()
    for i, w in enumerate(want):
        assert np.array_equal(fast[i, 0], w) and np.array_equal(exact[i, 0], w), (i, fast[i, 0].tolist(), exact[i, 0].tolist(), w.tolist())
    assert redo >= len(want)
