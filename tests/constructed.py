"""Constructed texts and reads, and brute-force references for seed lookup and voting.

Pure numpy / Python: nothing here touches an FM index, the oracle or the device library, so what a test derives from
this module is independent of all three.

    census(content, S)     every distinct S-mer of an index text with its occurrence count and positions
    check_sa(content, sa)  proof from first principles that `sa` is the suffix array of `content`
    vote_top2(keys)        histo_add / histo_find_2_max over a key stream in arrival order
    plant(spec, ...)       a text with prescribed strings at prescribed places between verified random filler
    read_of(kmers, ...)    a read whose phase-0 seeds are exactly the given k-mers
"""
import numpy as np

U64 = (1 << 64) - 1
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def _bytes_arr(s):
    return np.frombuffer(bytes(s), dtype=np.uint8) if not isinstance(s, np.ndarray) else s


def revcomp(s):
    return bytes(_COMP[_bytes_arr(s)][::-1])


def pack(kmer):
    """2 bits per base, first base most significant (the order of the text's suffixes)."""
    v = 0
    for c in bytes(kmer):
        assert _CODE[c] < 4, "not a nucleotide"
        v = (v << 2) | int(_CODE[c])
    return v


def _codes(bases, S):
    """Packed code of the S-mer at every position 0 .. len(bases) - S of an ACGT byte array."""
    c = _CODE[bases].astype(np.uint64)
    n = len(bases) - S + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    out = np.zeros(n, dtype=np.uint64)
    for i in range(S):
        out = (out << np.uint64(2)) | c[i:i + n]
    return out


class Census:
    """codes[i]: packed S-mer i (ascending); counts[i]; its positions (ascending): pos[start[i]:start[i] + counts[i]].
    at[p]: the count of the S-mer that starts at text position p, for EVERY p (0 .. n - S); code_at[p]: its packed code."""

    def __init__(self, S, codes, counts, start, pos, at):
        self.S, self.codes, self.counts, self.start, self.pos, self.at = S, codes, counts, start, pos, at

    def count(self, kmer):
        return int(self.count_codes(np.array([pack(kmer)], dtype=np.uint64))[0])

    def count_codes(self, codes):
        codes = np.asarray(codes, dtype=np.uint64)
        i = np.searchsorted(self.codes, codes)
        i = np.minimum(i, max(len(self.codes) - 1, 0))
        hit = (self.codes[i] == codes) if len(self.codes) else np.zeros(len(codes), dtype=bool)
        return np.where(hit, self.counts[i], 0).astype(np.int64)

    def first_positions(self, codes):
        """The first occurrence of each packed code (-1: absent)."""
        codes = np.asarray(codes, dtype=np.uint64)
        i = np.minimum(np.searchsorted(self.codes, codes), max(len(self.codes) - 1, 0))
        hit = self.codes[i] == codes
        return np.where(hit, self.pos[self.start[i]], -1)

    def positions(self, kmer):
        code = np.uint64(pack(kmer)) if not isinstance(kmer, (int, np.integer)) else np.uint64(kmer)
        i = int(np.searchsorted(self.codes, code))
        if i == len(self.codes) or self.codes[i] != code:
            return []
        return self.pos[self.start[i]:self.start[i] + self.counts[i]].tolist()


def census(content, S, last_base_quirk=True):
    """Occurrence count and positions of every distinct S-mer of an index text (`$` last), by sorting packed codes.

    last_base_quirk: the reference's search starts from the rows [1, L - 1], which leaves the `$` row out, so the one
    occurrence that ENDS ON THE LAST BASE of the text is never reported (test_last_base_occurrence_quirk).
    With the quirk that occurrence (position n - S) is left out of counts and positions; `at` still has an entry for
    it: what a search for the S-mer standing there reports."""
    content = _bytes_arr(content)
    assert content[-1] == ord("$"), "the index text ends with '$'"
    bases = content[:-1]
    assert (_CODE[bases] < 4).all(), "the index text is ACGT"
    assert 1 <= S <= 32
    code = _codes(bases, S)
    n_vis = len(code) - 1 if (last_base_quirk and len(code)) else len(code)
    vis = code[:n_vis]
    order = np.argsort(vis, kind="stable")                  # positions ascending inside a run of equal codes
    sc = vis[order]
    first = np.ones(len(sc), dtype=bool)
    first[1:] = sc[1:] != sc[:-1]
    start = np.nonzero(first)[0]
    counts = np.diff(np.append(start, len(sc)))
    c = Census(S, sc[start], counts.astype(np.int64), start.astype(np.int64), order.astype(np.int64), None)
    c.at = c.count_codes(code)
    c.code_at = code
    return c


def check_sa(content, sa, chunk=32):
    """Asserts that `sa` is the suffix array of `content` (`$` last and smallest): a permutation of 0 .. L - 1 whose
    adjacent suffixes are strictly ascending.  Pairs are compared `chunk` bytes at a time up to their first difference."""
    content = _bytes_arr(content)
    L = len(content)
    assert content[-1] == ord("$") and not (content[:-1] == ord("$")).any()
    assert ord("$") < ord("A")
    sa = np.asarray(sa)
    assert len(sa) == L, "suffix array length"
    assert int(sa.max()) < L
    sa = sa.astype(np.int64)
    assert (np.bincount(sa, minlength=L) == 1).all(), "not a permutation"
    pad = np.concatenate([content, np.zeros(chunk, dtype=np.uint8)])
    a, b = sa[:-1].copy(), sa[1:].copy()
    cols = np.arange(chunk, dtype=np.int64)
    while len(a):
        # ('$' is unique, so two different suffixes differ at or before the first '$': no index passes L - 1 + chunk)
        A, B = pad[a[:, None] + cols], pad[b[:, None] + cols]
        ne = A != B
        decided = ne.any(axis=1)
        col = ne.argmax(axis=1)
        rows = np.nonzero(decided)[0]
        assert (A[rows, col[rows]] < B[rows, col[rows]]).all(), "adjacent suffixes out of order"
        a, b = a[~decided] + chunk, b[~decided] + chunk
    return True


def vote_top2(keys):
    """histo_add over `keys` in arrival order, then histo_find_2_max: a bucket is key >> 4 and keeps its count, its
    minimum key and its place in first-seen order; the top two are "count descending, first seen ascending".
    -> (v, [(key, count, bucket), (key, count, bucket)]), absent places all zero."""
    table = {}                                               # dicts keep insertion order: first seen
    for key in keys:
        key &= U64
        e = table.get(key >> 4)
        if e is None:
            table[key >> 4] = [key, 1]
        else:
            e[0] = min(e[0], key)
            e[1] += 1
    top = [(0, 0, 0), (0, 0, 0)]
    for bucket, (key, n) in table.items():
        if n > top[0][1]:
            top = [(key, n, bucket), top[0]]
        elif n > top[1][1]:
            top[1] = (key, n, bucket)
    return top[0][1] + top[1][1], top


def index_text(seqs):
    """The index text of forward sequences: each followed by its reverse complement, '$' last."""
    return b"".join(bytes(s) + revcomp(s) for s in seqs) + b"$"


class Planted:
    """seq: the forward sequence (bytes); where[name]: start positions of the copies of `name`, in spec order."""

    def __init__(self, seq, where, spans):
        self.seq, self.where, self.spans = seq, where, spans

    def array(self):
        return np.frombuffer(self.seq, dtype=np.uint8)


def _filler(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])


def plant(spec, seed=0, k=20, gap=(40, 90), length=None, tries=16):
    """A forward sequence that holds the strings of `spec` between random filler.

    spec: a list of dicts in text order --
        name    label of the string (where[name] collects its copies)
        seq     the bases
        copies  how many times it is planted here, one after the other with filler between (default 1)
        at      absolute start (>= 0), or start counted from the END of the sequence (< 0; needs `length`);
                without it the string follows the previous one after a random gap of gap[0] .. gap[1] - 1 bases
        after   (name, copy, delta): start = start of that earlier copy + delta
    length: total length (filler to the end; default: a last gap after the last string).

    The filler must not create an occurrence of any planted k-mer: every window of the INDEX text (the sequence and its
    reverse complement, and the junction between them) that contains a filler base is checked against the k-mers of the
    planted strings.  A draw that fails is drawn again (`tries` times), then the spec is refused."""
    err = None
    for t in range(tries):
        rng = np.random.default_rng([seed, t])
        parts, where, spans, cur = [], {}, [], 0
        for it in spec:
            s = bytes(it["seq"])
            for c in range(int(it.get("copies", 1))):
                if it.get("at") is not None and c == 0:
                    at = int(it["at"])
                    if at < 0:
                        assert length is not None, "a start counted from the end needs the total length"
                        at += length
                elif it.get("after") is not None and c == 0:
                    nm, cp, delta = it["after"]
                    at = where[nm][cp] + delta
                else:
                    at = cur + int(rng.integers(gap[0], gap[1]))
                assert at >= cur, "spec item %r starts at %d, before the end of what precedes it (%d)" % (it["name"], at, cur)
                parts.append(_filler(rng, at - cur))
                parts.append(s)
                where.setdefault(it["name"], []).append(at)
                spans.append((at, at + len(s)))
                cur = at + len(s)
        end = length if length is not None else cur + int(rng.integers(gap[0], gap[1]))
        assert end >= cur, "length %d is shorter than the planted content (%d)" % (end, cur)
        parts.append(_filler(rng, end - cur))
        seq = b"".join(parts)
        err = _filler_clash(seq, spans, k)
        if err is None:
            return Planted(seq, where, spans)
    raise ValueError("plant: the filler keeps creating planted %d-mers (%s)" % (k, err))


def _filler_clash(seq, spans, k):
    n = len(seq)
    text = np.frombuffer(seq + revcomp(seq), dtype=np.uint8)
    planted = np.zeros(2 * n, dtype=bool)
    for a, b in spans:
        planted[a:b] = True
        planted[2 * n - b:2 * n - a] = True
    if len(text) < k:
        return None
    code = _codes(text, k)
    csum = np.concatenate([[0], np.cumsum(planted)])
    pure = (csum[k:] - csum[:-k]) == k                       # windows made of planted bases only
    want = np.unique(code[pure])
    bad = np.nonzero(~pure & np.isin(code, want))[0]
    if len(bad):
        p = int(bad[0])
        return "window at %d of the two-strand text: %s" % (p, bytes(text[p:p + k]).decode())
    return None


def read_of(kmers, spacers=None):
    """A read whose phase-0 seeds (j = 0, s + 1, 2 (s + 1), ...) are exactly `kmers` (all of one length s): each is
    followed by one spacer base (default: A, C, G, T in turn), so the read has len(kmers) * (s + 1) bases, the last
    seed position lies below len - s (alnmain.c:353) and num_seeds = len(kmers)."""
    s = len(kmers[0])
    assert all(len(x) == s for x in kmers)
    if spacers is None:
        spacers = [b"ACGT"[i % 4:i % 4 + 1] for i in range(len(kmers))]
    assert len(spacers) == len(kmers) and all(len(x) == 1 for x in spacers)
    return b"".join(bytes(x) + bytes(y) for x, y in zip(kmers, spacers))


def phase0_hits(read, S, thres, cen, sa_rank):
    """The phase-0 hit stream of `read` from first principles: seed j contributes, when 0 < count < thres, the keys
    pos - j (mod 2^64) of its occurrences in the order of their suffix-array rows (sa_rank[pos]: row of the suffix at pos,
    the inverse of a suffix array that check_sa has accepted).  Phase 0 of phase_cases.phase_hits (which builds on this
    module, hence the import here)."""
    from phase_cases import phase_hits
    return phase_hits(read, 0, S, thres, cen, sa_rank)


# ---------------------------------------------------------------------------------------------------------------
# Constructed workloads (texts and reads only: the tests build the indexes)
# ---------------------------------------------------------------------------------------------------------------
def kmers(rng, n, S=20):
    """n random S-mers (bytes)."""
    return [_filler(rng, S) for _ in range(n)]


def segment(rng, n, S=20):
    """A read segment of n seeds: planted at text position P and placed at read offset J (a multiple of S + 1), all its
    phase-0 seeds vote for the diagonal P - J."""
    return read_of(kmers(rng, n, S))


def low_complexity(thres_small=50, seed=5):
    """The low-complexity / threshold text (two sequences, so the index text has a strand boundary inside each and a
    sequence boundary between them) -> dict(seqs, planted (of sequence 0), kmers {name: 20-mer}, copies {name: count})."""
    rng = np.random.default_rng(seed)
    km = {}
    copies = {}
    spec = [dict(name="head", seq=_filler(rng, 20), at=0)]                  # a unique 20-mer at content position 0
    km["head"], copies["head"] = spec[0]["seq"], 1
    runs = [("A35", b"C" + b"A" * 35 + b"G"), ("A60", b"G" + b"A" * 60 + b"C"), ("AC40", b"G" + b"AC" * 40 + b"G"),
            ("ACG30", b"T" + b"ACG" * 30 + b"T"), ("P7x15", b"C" + b"ACGTTGA" * 15 + b"C")]
    for name, s in runs:
        spec.append(dict(name=name, seq=s))
    counted = [("c1", 1), ("c2", 2), ("c3", 3), ("c4", 4), ("e3", 3), ("t-1", thres_small - 1), ("t", thres_small),
               ("t+1", thres_small + 1), ("d-1", 299), ("d", 300), ("d+1", 301)]
    for name, n in counted:
        km[name], copies[name] = _filler(rng, 20), n
    # interleaved, so that the copies of one k-mer are spread over the text
    order = [name for name, n in counted for _ in range(n)]
    order = [order[i] for i in rng.permutation(len(order))]
    for name in order:
        spec.append(dict(name=name, seq=km[name]))
    pl = plant(spec, seed=seed, gap=(25, 45))
    # sequence 1 begins with the reverse complement of e3: the index text then ENDS with e3 -- a fourth occurrence, on
    # the last base, which no search reports
    seq1 = revcomp(km["e3"]) + _filler(rng, 12_000)
    return dict(seqs=[pl.seq, seq1], planted=pl, kmers=km, copies=copies, runs=dict(runs))


def _case(name, seq, read, expect, thres=300):
    return dict(name=name, seq=seq, read=read, expect=expect, thres=thres)


def _beyond(read, spec, first=0):
    """Ordinary loci start beyond the read's length: none of their diagonals wraps by accident."""
    spec[first]["at"] = len(read) + 64
    return spec


def vote_case(name, scale=1, seed=0):
    """One constructed vote: a forward sequence and a read whose phase-0 hit stream is known by construction.
    expect: (key, count) of the phase-0 winner as the construction gives it (the tests derive the full top two from
    census + vote_top2 as well).  scale multiplies the seed counts (items beyond the wavefront tier's 192 hits)."""
    import zlib
    rng = np.random.default_rng([seed, zlib.crc32(name.encode()), scale])
    k = scale
    if name in ("tie-by-seed-order", "tie-by-sa-order"):
        a, b = 10 * k, 3 * k
        zs = [segment(rng, b) for _ in range(3)]
        if name == "tie-by-seed-order":
            # X comes first in the read and LAST in the text; Y ties with it
            x, y = segment(rng, a), segment(rng, a)
            read = x + y + b"".join(zs)
            pl = plant(_beyond(read, [dict(name="z2", seq=zs[2]), dict(name="y", seq=y), dict(name="z1", seq=zs[1]),
                                      dict(name="x", seq=x), dict(name="z0", seq=zs[0])]), seed=seed)
            return _case(name, pl.seq, read, (pl.where["x"][0], a))
        # one repeat seed R opens the read; its two copies start the two tied loci.  The copy that is FIRST in the text is
        # followed by T, the later one by A: in the suffix array the later copy comes first, and with it its bucket
        r = kmers(rng, 1)[0]
        u1, u2 = segment(rng, a - 1), segment(rng, a - 1)
        n1 = len(u1)
        read = r + b"C" + u1 + u2 + b"".join(zs)
        pl = plant(_beyond(read, [dict(name="z0", seq=zs[0]),
                                  dict(name="r", seq=r + b"T"), dict(name="u1", seq=u1, after=("r", 0, 21)), dict(name="z1", seq=zs[1]),
                                  dict(name="r", seq=r + b"A"), dict(name="u2", seq=u2, after=("r", 1, 21 + n1)),
                                  dict(name="z2", seq=zs[2])]), seed=seed)
        return _case(name, pl.seq, read, (pl.where["r"][1], a))
    if name == "bucket-edges":
        # diagonals d + 15, d, d + 16 around a multiple of 16, in this order in the read; dead seeds (absent k-mers) keep
        # the three text segments apart
        d = 4096 * k
        s1, s2, s3 = segment(rng, 3 * k), segment(rng, 2 * k), segment(rng, 4 * k)
        dead = segment(rng, 1)
        j2 = len(s1) + 21
        j3 = j2 + len(s2) + 21
        pl = plant([dict(name="s1", seq=s1, at=d + 15), dict(name="s2", seq=s2, at=d + j2),
                    dict(name="s3", seq=s3, at=d + 16 + j3)], seed=seed)
        return _case(name, pl.seq, s1 + dead + s2 + dead + s3, (d, 5 * k))
    if name.startswith("wrapped"):
        # W sits at text position 7 and behind other seeds in the read: pos < j, its key wraps around 2^64
        w, b = {"wrapped-first-seen-wins-tie": (5, 5), "wrapped-second-seen-loses-tie": (5, 5),
                "wrapped-beats-by-count": (6, 5)}[name]
        w, b = w * k, b * k
        sa_, sw, sb = segment(rng, 3), segment(rng, w), segment(rng, b)
        pl = plant(_beyond(sa_ + sw + sb, [dict(name="w", seq=sw, at=7), dict(name="b", seq=sb), dict(name="a", seq=sa_)], 1), seed=seed)
        if name == "wrapped-first-seen-wins-tie":
            read, jw = sa_ + sw + sb, len(sa_)
            exp = ((7 - jw) & U64, w)
        else:
            read, jw, jb = sa_ + sb + sw, len(sa_) + len(sb), len(sa_)
            exp = ((7 - jw) & U64, w) if w > b else (pl.where["b"][0] - jb, b)
        return _case(name, pl.seq, read, exp)
    if name.startswith("settle"):
        # unique-seed buckets with counts a >= b, and two repeat-only buckets of count m (m seeds of two copies each, the
        # block planted twice) that are seen FIRST
        a, b, m = _SETTLE[name]
        a, b, m = a * k, b * k, m * k
        rb, ua, ub = segment(rng, m), segment(rng, a), segment(rng, b)
        read = rb + ua + ub
        pl = plant(_beyond(read, [dict(name="ub", seq=ub), dict(name="rb", seq=rb), dict(name="ua", seq=ua), dict(name="rb", seq=rb)]), seed=seed)
        if m >= a:
            exp = (None, m)                                   # one of the two repeat-only buckets: the suffix array says which
        else:
            exp = (pl.where["ua"][0] - len(rb), a)
        return _case(name, pl.seq, read, exp)
    if name == "no-unique-seed":
        r1, r2 = segment(rng, 6 * k), segment(rng, 4 * k)
        pl = plant(_beyond(r2 + r1, [dict(name="r2", seq=r2), dict(name="r1", seq=r1), dict(name="r2", seq=r2), dict(name="r1", seq=r1),
                                     dict(name="r2", seq=r2)]), seed=seed)
        return _case(name, pl.seq, r2 + r1, (None, 6 * k))
    if name == "one-unique-seed":
        u, r1 = segment(rng, 1), segment(rng, 3 * k)
        pl = plant(_beyond(u + r1, [dict(name="r1", seq=r1), dict(name="u", seq=u), dict(name="r1", seq=r1)]), seed=seed)
        return _case(name, pl.seq, u + r1, (None, 3 * k))
    raise KeyError(name)


_SETTLE = {"settle-m=b-1": (12, 6, 5), "settle-m=b": (12, 6, 6), "settle-m=b+1": (12, 6, 7), "settle-m=a": (12, 6, 12),
           "settle-m=a+1": (12, 6, 13), "settle-m=a=b": (8, 8, 8), "settle-m=a=b-long": (70, 70, 70),
           "settle-survivors-1536": (1450, 50, 36), "settle-survivors-1537": (1450, 50, 37)}

VOTE_CASES = ["tie-by-seed-order", "tie-by-sa-order", "bucket-edges", "wrapped-first-seen-wins-tie",
              "wrapped-second-seen-loses-tie", "wrapped-beats-by-count"] + list(_SETTLE) + ["no-unique-seed", "one-unique-seed"]
# the cases that make sense with more than the wavefront tier's 192 hits per item
SCALED_CASES = ["tie-by-seed-order", "tie-by-sa-order", "bucket-edges", "wrapped-first-seen-wins-tie",
                "wrapped-second-seen-loses-tie", "settle-m=a=b", "settle-m=b", "no-unique-seed"]


def lowc_reads(w, content):
    """(reads, lens): reads made of the planted k-mers, and windows of the text over its runs, its ends and its boundaries."""
    km = w["kmers"]
    n0, n1 = len(w["seqs"][0]), len(w["seqs"][1])
    L = len(content)
    names = ["head", "c1", "c2", "c3", "c4", "e3", "t-1", "t", "t+1", "d-1", "d", "d+1"]
    reads = [read_of([km[x] for x in names]), read_of([km[x] for x in reversed(names)]),
             read_of([km["c2"], km["c1"], km["c2"], km["t-1"]]), read_of([km["d-1"]] * 2 + [km["head"]]),
             read_of([km["t"], km["t+1"], km["d"], km["d+1"]])]
    pl = w["planted"]
    for name in w["runs"]:
        p = pl.where[name][0]
        reads.append(bytes(content[max(p - 150, 0):p + 350]))
    for edge in (n0, 2 * n0, 2 * n0 + n1):
        reads.append(bytes(content[edge - 300:edge + 300]))
    reads.append(bytes(content[:500]))
    reads.append(bytes(content[L - 501:L - 1]))
    arr = np.zeros((len(reads), max(len(r) for r in reads) + 1), dtype=np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return arr, np.array([len(r) for r in reads], dtype=np.uint32)


def text_windows(content, S, width, first=0):
    """The index text cut into reads that together evaluate EVERY S-mer position from `first` on: a read of len bases has
    seeds at j < len - S (alnmain.c:353), so windows overlap by S and the last one gets one base appended -- the S-mer
    that ends on the text's last base is looked up too.  -> [(text position of the read's base 0, read bytes)]"""
    n = len(content) - 1
    out = []
    for p in range(first, n - S + 1, width):
        w = bytes(content[p:min(p + width + S, n)])
        out.append((p, w + b"A" if p + width + S > n else w))
    return out
