"""The oracle's FM index / lchash / histo half against brute force, on constructed texts and reads.

tests/constructed.py knows nothing of FM indexes: it counts S-mers by sorting packed codes, proves a suffix array by
comparing adjacent suffixes, and votes with a dict.  Here every seed the oracle evaluates on the constructed workloads
must report the census count and, through the (proved) suffix array, the census positions; and the oracle's phase-0
vote must be vote_top2 of the hit stream the construction prescribes.  The GPU file (test_gpu_constructed.py) then
holds the device to the same references."""
import numpy as np
import pytest

import constructed as K
import orc
from longreadmapper_amd import capi, index, synth

KAT = b"ACGTACGATTAGCCGTAACG$"
KAT_SA = [20, 16, 17, 4, 0, 10, 7, 12, 18, 5, 13, 1, 19, 6, 11, 14, 2, 15, 3, 9, 8]


# ---- the option structs refuse what they do not have ----------------------------------------------------------------
def test_index_options_refuse_a_misspelt_name():
    assert capi.index_options(seed_table_share=2).seed_table_share == 2
    assert capi.index_options(seed_table_share=None).seed_table_share == capi.index_options().seed_table_share
    for bad in ("seed_table_shares", "seedtable_share", "lc_lonng"):
        with pytest.raises(AttributeError):
            capi.index_options(**{bad: 2})
        with pytest.raises(AttributeError):
            capi.index_options(**{bad: None})


def test_map_options_refuse_a_misspelt_name():
    assert capi.map_options(vote_exact_only=1).vote_exact_only == 1
    with pytest.raises(AttributeError):
        capi.map_options(vote_exact_onyl=1)


# ---- the helpers on known answers ------------------------------------------------------------------------------------
def test_census_known_answers_and_the_last_base_quirk():
    text = np.frombuffer(KAT, dtype=np.uint8)
    c = K.census(text, 3)
    assert c.count(b"ACG") == 2 and c.positions(b"ACG") == [0, 4]            # the third, at 17, ends on the last base
    assert K.census(text, 3, last_base_quirk=False).positions(b"ACG") == [0, 4, 17]
    assert c.count(b"CGT") == 2 and c.count(b"TTT") == 0
    assert c.at[17] == 2 and c.at[0] == 2 and len(c.at) == 18
    c7 = K.census(text, 7)
    assert c7.count(b"CGTAACG") == 0 and c7.at[13] == 0                       # unique and on the last base: absent
    assert int(c.counts.sum()) == 17
    # against str.count-like brute force on a text with overlapping repeats
    t = b"AAAAACAAAAAGAAAAA$"
    c = K.census(np.frombuffer(t, dtype=np.uint8), 4)
    assert c.positions(b"AAAA") == [0, 1, 6, 7, 12] and c.at.tolist()[:2] == [5, 5] and c.at[13] == 5


def test_check_sa_accepts_the_suffix_array_and_nothing_else():
    text = np.frombuffer(KAT, dtype=np.uint8)
    assert K.check_sa(text, np.array(KAT_SA, dtype=np.uint64))
    bad = KAT_SA[:]
    bad[3], bad[4] = bad[4], bad[3]                      # ACGATT.. before ACGTAC..: swapped
    with pytest.raises(AssertionError):
        K.check_sa(text, np.array(bad, dtype=np.uint64))
    bad = KAT_SA[:]
    bad[5] = bad[6]
    with pytest.raises(AssertionError):
        K.check_sa(text, np.array(bad, dtype=np.uint64))
    # long common prefixes (several chunks) and brute force by sorting, on a tandem text
    t = b"ACGT" * 60 + b"ACGA" + b"ACGT" * 50 + b"$"
    sa = sorted(range(len(t)), key=lambda i: t[i:])
    assert K.check_sa(np.frombuffer(t, dtype=np.uint8), np.array(sa, dtype=np.uint64), chunk=16)
    sa[10], sa[11] = sa[11], sa[10]
    with pytest.raises(AssertionError):
        K.check_sa(np.frombuffer(t, dtype=np.uint8), np.array(sa, dtype=np.uint64), chunk=16)


def test_vote_top2_known_answers():
    assert K.vote_top2([100, 101, 5000]) == (3, [(100, 2, 6), (5000, 1, 312)])
    assert K.vote_top2([]) == (0, [(0, 0, 0), (0, 0, 0)])
    # stable: of equal counts the first seen wins, also for the second place; the key is the bucket's minimum
    assert K.vote_top2([47, 16, 32, 17, 64, 65])[1] == [(32, 2, 2), (16, 2, 1)]
    assert K.vote_top2([(-3) & K.U64, 5, (-16) & K.U64])[1] == [(K.U64 - 15, 2, K.U64 >> 4), (5, 1, 0)]


def test_plant_places_and_verifies():
    a, b = b"ACGTTGCAAGGCTTAACCGA", b"TTGACCATGCAAGTCCATGA"
    pl = K.plant([dict(name="a", seq=a, at=0), dict(name="b", seq=b, copies=3), dict(name="a", seq=a, after=("b", 2, 40)),
                  dict(name="b", seq=b, at=-20)], seed=1, length=2000)
    assert len(pl.seq) == 2000 and pl.where["a"][0] == 0 and pl.where["a"][1] == pl.where["b"][2] + 40
    assert pl.where["b"][3] == 1980 and pl.seq.endswith(b)
    cen = K.census(np.frombuffer(K.index_text([pl.seq]), dtype=np.uint8), 20)
    assert cen.positions(a) == pl.where["a"] and cen.positions(b) == pl.where["b"]
    assert cen.count(K.revcomp(a)) == 1      # of its two, the one opposite position 0 ends on the last base
    assert cen.count(K.revcomp(b)) == 4
    # a spec whose own strings overlap the place of another is refused; so is filler that cannot avoid a planted k-mer
    with pytest.raises(AssertionError):
        K.plant([dict(name="a", seq=a, at=10), dict(name="b", seq=b, at=20)])
    with pytest.raises(ValueError):
        K.plant([dict(name="a", seq=b"A")], k=1, gap=(200, 201))
    r = K.read_of([a, b, a])
    assert len(r) == 63 and r[0:20] == a and r[21:41] == b and r[42:62] == a


# ---- the oracle against the census ----------------------------------------------------------------------------------
def _index(seqs, hlen=8):
    hi = index.HostIndex.build([np.frombuffer(bytes(s), dtype=np.uint8) for s in seqs], hlen=hlen)
    content = hi.content()
    assert bytes(content) == K.index_text(seqs)
    K.check_sa(content, hi.sa())
    return hi, orc.OracleIndex.from_host_index(hi)


def _check_seeds(oi, hi, cen, read, S):
    """Every seed position of `read` (thres = 0: the oracle never decides, so all phases run): rr is the census count and
    the rows k .. l hold the census positions."""
    sa = hi.sa()
    tr = oi.seed_read(bytes(read), S, 0, trace=True)
    assert len(tr["seeds"]) == max(len(read) - S, 0)
    for j, rr, k, l in tr["seeds"]:
        km = bytes(read[j:j + S])
        pos = cen.positions(km)
        assert rr == len(pos), (j, km, rr, len(pos))
        if rr:
            assert l - k + 1 == rr and sorted(int(x) for x in sa[k:l + 1]) == pos, (j, km)


def _windows(content, S, width=4000):
    return [w for _, w in K.text_windows(content, S, width)]


@pytest.mark.parametrize("S,hlen", [(16, 8), (20, 8), (24, 8), (20, 12)])
def test_oracle_counts_every_smer_of_a_random_text(S, hlen):
    """The text itself as reads: every S-mer the text holds, at every position, also the one on the last base (which the
    census with the quirk makes one occurrence poorer) and A^S at position 0."""
    seq = b"A" * S + b"C" + bytes(synth.reference(30_000, seed=90 + S))
    hi, oi = _index([seq], hlen)
    content = hi.content()
    cen = K.census(content, S)
    assert cen.at[0] == 1 and cen.at[-1] == 0 and cen.at[-2] == 1
    for w in _windows(content, S):
        _check_seeds(oi, hi, cen, w, S)
    # absent S-mers: one substitution at the first base, inside, and at the last base of present ones
    rng = np.random.default_rng(S)
    for p in rng.integers(0, len(content) - 1 - S, size=200):
        for at in (0, 3, S // 2, S - 1):
            km = bytearray(bytes(content[p:p + S]))
            km[at] = b"ACGT"[(b"ACGT".index(km[at]) + 1 + int(rng.integers(0, 3))) % 4]
            r, k, l = oi.lc_aln(bytes(km))
            assert r == cen.count(km)


def test_census_without_the_quirk_disagrees_with_the_oracle():
    """The brute force is independent of the oracle: without the named quirk the two differ exactly on the S-mer that
    ends on the last base."""
    seq = bytes(synth.reference(5_000, seed=3))
    hi, oi = _index([seq])
    content = hi.content()
    tail = bytes(content[-21:-1])
    plain = K.census(content, 20, last_base_quirk=False)
    assert plain.count(tail) == 1 and K.census(content, 20).count(tail) == 0
    assert oi.lc_aln(tail)[0] == 0
    with pytest.raises(AssertionError):
        _check_seeds(oi, hi, plain, bytes(content[-400:-1]) + b"A", 20)


@pytest.fixture(scope="module")
def lowc():
    w = K.low_complexity()
    hi, oi = _index(w["seqs"])
    return w, hi, oi, K.census(hi.content(), 20)


def test_low_complexity_text_is_what_it_claims(lowc):
    w, hi, oi, cen = lowc
    km, pl = w["kmers"], w["planted"]
    n0, n1 = len(w["seqs"][0]), len(w["seqs"][1])
    L = len(hi.content())
    assert L == 2 * (n0 + n1) + 1
    assert cen.count(b"A" * 20) == 16 + 41 and cen.count(b"T" * 20) == 16 + 41
    a60 = pl.where["A60"][0] + 1
    assert cen.positions(b"A" * 20)[16:] == list(range(a60, a60 + 41))
    assert cen.count(b"AC" * 10) == 31 and cen.count(b"CA" * 10) == 30 and cen.count(b"ACG" * 6 + b"AC") == 24
    for name, n in w["copies"].items():
        want = n
        assert cen.count(km[name]) == want, name
        assert cen.positions(km[name]) == pl.where[name]
    assert cen.positions(km["head"]) == [0]
    # the text ends with e3: a fourth occurrence that no search sees; before it, the last S-mer a search can see
    assert bytes(hi.content()[L - 21:L - 1]) == km["e3"] and cen.at[L - 21] == 3
    assert K.census(hi.content(), 20, last_base_quirk=False).count(km["e3"]) == 4
    assert cen.at[L - 22] == 1
    # S-mers across the strand boundary of each sequence and across the sequence boundary
    for edge in (n0, 2 * n0, 2 * n0 + n1):
        assert (cen.at[edge - 19:edge] >= 1).all()


def test_oracle_on_the_low_complexity_text(lowc):
    w, hi, oi, cen = lowc
    content = hi.content()
    for win in _windows(content, 20):
        _check_seeds(oi, hi, cen, win, 20)


def _phase0(oi, hi, cen, read, thres):
    sa = hi.sa()
    rank = np.empty(len(sa), dtype=np.int64)
    rank[sa.astype(np.int64)] = np.arange(len(sa))
    keys = K.phase0_hits(read, 20, thres, cen, rank)
    tr = oi.seed_read(bytes(read), 20, thres, trace=True)
    rec = tr["phase_recs"][0]
    v, top = K.vote_top2(keys)
    assert rec["iter"] == 0 and (rec["v"], [rec["top1"], rec["top2"]]) == (v, top)
    return keys, rec, tr


def _ref_histo(keys):
    lib = orc.ref_histo_lib()
    if lib is None:
        return None
    h = lib.histo_init(300)
    for k in keys:
        lib.histo_add(h, k)
    st = (orc.Entry * 2)()
    v = lib.histo_find_2_max(h, st)
    out = (int(v), [(int(e.key), int(e.val), int(e.bucket)) for e in st])
    lib.histo_destroy(h)
    return out


@pytest.mark.parametrize("thres", [50, 300])
def test_oracle_votes_on_the_low_complexity_reads(lowc, thres):
    """Counts of thres - 1 vote and counts of thres do not, for the small threshold and for the default."""
    w, hi, oi, cen = lowc
    reads, lens = K.lowc_reads(w, hi.content())
    streams = []
    for i in range(len(lens)):
        keys, rec, tr = _phase0(oi, hi, cen, bytes(reads[i, :lens[i]]), thres)
        streams.append(keys)
    km = w["kmers"]
    t = thres
    lo, at_ = ("t-1", "t") if thres == 50 else ("d-1", "d")
    assert len(K.phase0_hits(K.read_of([km[lo]]), 20, t, cen, _rank(hi))) == t - 1
    assert K.phase0_hits(K.read_of([km[at_]]), 20, t, cen, _rank(hi)) == []
    ref = [_ref_histo(s) for s in streams]
    if ref[0] is not None:
        assert ref == [K.vote_top2(s) for s in streams]


def _rank(hi):
    sa = hi.sa()
    rank = np.empty(len(sa), dtype=np.int64)
    rank[sa.astype(np.int64)] = np.arange(len(sa))
    return rank


# ---- constructed votes ---------------------------------------------------------------------------------------------
CASES = [(n, 1) for n in K.VOTE_CASES] + [(n, 30) for n in K.SCALED_CASES]


@pytest.mark.parametrize("name,scale", CASES, ids=["%s-x%d" % c for c in CASES])
def test_oracle_phase0_vote_is_vote_top2(name, scale):
    c = K.vote_case(name, scale)
    hi, oi = _index([c["seq"]])
    cen = K.census(hi.content(), 20)
    read = c["read"]
    _check_seeds(oi, hi, cen, read[:3000], 20)
    keys, rec, tr = _phase0(oi, hi, cen, read, c["thres"])
    key, val = c["expect"]
    assert rec["top1"][1] == val and (key is None or rec["top1"][0] == key), (rec, c["expect"])
    # every case is built so that phase 0 decides: what the device reports is this phase's winner
    assert rec["decided"] == 1 and tr["best"] == rec["top1"]
    ref = _ref_histo(keys)
    if ref is not None:
        assert ref == K.vote_top2(keys)


def test_constructed_votes_say_what_they_are_for():
    """The properties the cases are named after, from the construction alone (census + suffix array + vote_top2)."""
    def top(name, scale=1):
        c = K.vote_case(name, scale)
        hi, oi = _index([c["seq"]])
        cen = K.census(hi.content(), 20)
        keys = K.phase0_hits(c["read"], 20, 300, cen, _rank(hi))
        return c, cen, keys, K.vote_top2(keys)[1]
    # seed order: the winner lies LATER in the text than the bucket it ties with
    c, cen, keys, t = top("tie-by-seed-order")
    assert t[0][1] == t[1][1] == 10 and t[0][0] > t[1][0] and sorted(x[1] for x in K.vote_top2(keys[20:])[1]) == [3, 3]
    # suffix-array order: the first seed has two hits, the later text position comes first, and its bucket wins
    c, cen, keys, t = top("tie-by-sa-order")
    assert keys[0] > keys[1] and t[0][0] == keys[0] and t[1][0] == keys[1] and t[0][1] == t[1][1] == 10
    # d + 15 and d share a bucket, reported with its minimum key although d + 15 came first; d + 16 is the next bucket
    c, cen, keys, t = top("bucket-edges")
    assert keys[0] == 4096 + 15 and keys[3] == 4096 and t == [(4096, 5, 256), (4112, 4, 257)]
    c, cen, keys, t = top("wrapped-first-seen-wins-tie")
    assert t[0][0] > 1 << 63 and t[0][1] == t[1][1] == 5 and t[1][0] < 1 << 40
    c, cen, keys, t = top("wrapped-second-seen-loses-tie")
    assert t[1][0] > 1 << 63 and t[0][1] == t[1][1] == 5 and t[0][0] < 1 << 40
    c, cen, keys, t = top("wrapped-beats-by-count")
    assert t[0][0] > 1 << 63 and (t[0][1], t[1][1]) == (6, 5)
    # the settle rule: the winner moves from the unique-seed bucket to a repeat-only bucket as m passes a
    winners = {}
    for name in K._SETTLE:
        c, cen, keys, t = top(name)
        a, b, m = K._SETTLE[name]
        rep_keys = set(keys[:2 * m])                      # the m repeat seeds come first, two hits each
        assert len(rep_keys) == 2
        winners[name] = (t[0][0] in rep_keys, t[0][1], t[1][0] in rep_keys, t[1][1])
    assert winners["settle-m=b-1"] == (False, 12, False, 6)
    assert winners["settle-m=b"] == (False, 12, True, 6)          # a repeat-only bucket ties the second and was seen first
    assert winners["settle-m=b+1"] == (False, 12, True, 7)
    assert winners["settle-m=a"] == (True, 12, True, 12)
    assert winners["settle-m=a+1"] == (True, 13, True, 13)
    assert winners["settle-m=a=b"] == (True, 8, True, 8)
    assert winners["settle-m=a=b-long"] == (True, 70, True, 70)
    assert winners["settle-survivors-1536"] == (False, 1450, False, 50)
    for name, n in (("settle-survivors-1536", 1536), ("settle-survivors-1537", 1537)):
        c = K.vote_case(name)
        assert len(c["read"]) == 21 * n
