"""The device's seed tables and vote kernels against brute force (tests/constructed.py), on constructed inputs.

A. Table census: the text itself is fed as reads, so EVERY S-mer the device entered into its tables is looked up, in
   every role it can have in a shared line, and must come back with the census count (and, where a unique seed carries
   its text position, with that position); one-substitution neighbours that the text does not hold must come back empty.
B. The low-complexity / threshold text: homopolymer and tandem runs, counts of exactly 1 .. 4, thres - 1 .. thres + 1,
   S-mers at position 0, at the last visible position, on the last base, across strand and sequence boundaries.
C. Constructed votes: ties decided by first-seen order (seed ordinal, then suffix-array row), bucket edges, wrapped keys,
   the fast kernel's settle rule on both sides of every comparison it makes.
test_constructed_cpu.py holds the oracle to the same references without a device."""
import ctypes as C

import numpy as np
import pytest

import constructed as K
import orc
from longreadmapper_amd import capi, index, mapper, synth

pytestmark = pytest.mark.gpu

LOC = 1 << 39          # LRM_LOCATED_BIT: the row field of a unique seed holds its text position


def _sd(S=20, share=4, bits=None, cbits=None):
    return dict(seed_table=1, lc_long=13, seed_table_len=S, seed_table_share=share, seed_table_bits=bits,
                seed_table_count_bits=cbits)


# name -> (seed length, index options, what di.tables() must then say)
GEOMETRIES = {
    "lchash": (20, dict(lc_long=0, lc_core=0, seed_table=0), dict(lc_long=0, lc_core=0, seed_table_len=0)),
    "13-plain": (20, dict(lc_long=13, lc_pair=0, lc_core=0, seed_table=0), dict(lc_long=13, lc_pair=0, lc_entry_bytes=8, lc_core=0, seed_table_len=0)),
    "14": (20, dict(lc_long=14, lc_core=0, seed_table=0), dict(lc_long=14, lc_entry_bytes=8, lc_core=0, seed_table_len=0)),
    "15-5byte": (20, dict(lc_long=15, lc_entry_bytes=5, lc_core=0, seed_table=0), dict(lc_long=15, lc_entry_bytes=5, seed_table_len=0)),
    "14-5byte-side": (20, dict(lc_long=14, lc_entry_bytes=5, lc_count_bits=2, lc_core=0, seed_table=0),
                      dict(lc_long=14, lc_entry_bytes=5, seed_table_len=0)),
    "16-core": (20, dict(lc_long=16, lc_core=1, seed_table=0), dict(lc_long=16, lc_core=1, seed_table_len=0)),
    "16-nocore": (20, dict(lc_long=16, lc_core=0, seed_table=0), dict(lc_long=16, lc_core=0, seed_table_len=0)),
    "sd-share4": (20, _sd(), dict(seed_table_len=20, seed_table_share=4, seed_table_slot_bytes=8)),
    "sd-share2": (20, _sd(share=2), dict(seed_table_len=20, seed_table_share=2, seed_table_slot_bytes=6)),
    "sd-share4-crowded": (20, _sd(bits=16), dict(seed_table_len=20, seed_table_share=4, seed_table_bits=16, seed_table_slot_bytes=8)),
    "sd-share2-crowded": (20, _sd(share=2, bits=14), dict(seed_table_len=20, seed_table_share=2, seed_table_bits=14, seed_table_slot_bytes=6)),
    "sd-share4-counts2": (20, _sd(cbits=2), dict(seed_table_len=20, seed_table_share=4, seed_table_count_bits=2)),
    "sd-share2-crowded-counts2": (20, _sd(share=2, bits=14, cbits=2),
                                  dict(seed_table_len=20, seed_table_share=2, seed_table_bits=14, seed_table_count_bits=2)),
    "sd-seed16-share4": (16, _sd(16), dict(seed_table_len=16, seed_table_share=4, seed_table_slot_bytes=8)),
    "sd-seed16-share2": (16, _sd(16, share=2), dict(seed_table_len=16, seed_table_share=2, seed_table_slot_bytes=6)),
    "sd-seed24-share4": (24, _sd(24), dict(seed_table_len=24, seed_table_share=4, seed_table_slot_bytes=8)),
    # (6-byte slots have room for the 46-bit core's tag only with many lines: a small text gets them by hand)
    "sd-seed24-share2": (24, _sd(24, share=2, bits=24), dict(seed_table_len=24, seed_table_share=2, seed_table_bits=24, seed_table_slot_bytes=6)),
}


def _host(seqs):
    hi = index.HostIndex.build([np.frombuffer(bytes(s), dtype=np.uint8) for s in seqs], hlen=8)
    assert bytes(hi.content()) == K.index_text(seqs)
    K.check_sa(hi.content(), hi.sa())
    return hi


@pytest.fixture(scope="module")
def texts():
    cache = {}

    def get(kind, S):
        if (kind, S) not in cache:
            if kind == "random":
                # A^S opens the text: in role 0 its tag is all zeros, and a unique S-mer at position 0 that carried its
                # position along (count code 0) would be an all-zero slot, which means "empty"
                seqs = [b"A" * S + b"C" + bytes(synth.reference(90_000, seed=70 + S))]
            else:
                seqs = K.low_complexity()["seqs"]
            hi = _host(seqs)
            cache[(kind, S)] = (hi, K.census(hi.content(), S))
        return cache[(kind, S)]
    return get


def _device_seeds(di, read, S):
    """lrm_debug_seed_search on one read -> (j, rr, k, l) of its seed positions, by j."""
    buf = np.frombuffer(read, dtype=np.uint8)
    ln = len(buf)
    cap = (ln // (S + 1) + 2) * (S + 1)
    j = np.zeros(cap, dtype=np.int32)
    rr, k, l = (np.zeros(cap, dtype=np.uint64) for _ in range(3))
    n_out = C.c_uint64()
    capi.check(capi.lib.lrm_debug_seed_search(di.handle, buf.ctypes.data, ln, S, 300, j.ctypes.data, rr.ctypes.data,
                                              k.ctypes.data, l.ctypes.data, cap, C.byref(n_out)), "debug_seed_search")
    n = int(n_out.value)
    keep = j[:n] >= 0
    j, rr, k, l = j[:n][keep], rr[:n][keep], k[:n][keep], l[:n][keep]
    o = np.argsort(j)
    assert np.array_equal(j[o], np.arange(max(ln - S, 0))), "one result per seed position"
    return rr[o].astype(np.int64), k[o], l[o]


def _check_against_census(rr, k, l, codes, cen, sa, what):
    """rr == census count for every looked-up S-mer; a located unique seed carries the census position; otherwise the rows
    k .. l are as many as the count and hold the census positions."""
    want = cen.count_codes(codes)
    bad = np.nonzero(rr != want)[0]
    assert len(bad) == 0, (what, "count", len(bad), [(int(i), int(rr[i]), int(want[i])) for i in bad[:8]])
    hit = rr > 0
    located = hit & ((k & np.uint64(LOC)) != 0)
    first = cen.first_positions(codes)
    assert (rr[located] == 1).all(), what
    assert np.array_equal((k[located] & np.uint64(LOC - 1)).astype(np.int64), first[located]), (what, "carried position")
    rows = hit & ~located
    assert np.array_equal((l[rows] - k[rows] + np.uint64(1)).astype(np.int64), rr[rows]), (what, "interval length")
    one = rows & (rr == 1)
    assert np.array_equal(sa[k[one].astype(np.int64)].astype(np.int64), first[one]), (what, "row of a unique seed")
    seen = set()
    for i in np.nonzero(rows & (rr > 1))[0]:
        if int(k[i]) not in seen:
            seen.add(int(k[i]))
            assert sorted(int(x) for x in sa[int(k[i]):int(l[i]) + 1]) == cen.positions(int(codes[i])), (what, "rows", int(i))
    return int(located.sum())


def _census_of_the_device(di, hi, cen, S, width=8192):
    content, sa = hi.content(), hi.sa()
    n_located = 0
    for first in range(4):                      # every S-mer in every role j mod F of a shared line
        for p, w in K.text_windows(content, S, width, first):
            rr, k, l = _device_seeds(di, w, S)
            n_located += _check_against_census(rr, k, l, cen.code_at[p:p + len(rr)], cen, sa, ("text", first, p))
    assert p + len(rr) == len(cen.at), "the last window ends on the S-mer of the last base"
    return n_located


def _neighbours(content, cen, S, F, rng, n=1500):
    """Present S-mers with one substitution at base 0, F - 1, the middle of the core and S - 1 (the tag's extra bits, the
    first base of the core, the residue / line): the k-mers, and their packed codes."""
    out = []
    pos = np.concatenate([[0, len(cen.at) - 1, len(cen.at) - 2], rng.integers(0, len(cen.at), size=n)])
    for p in pos:
        km = bytes(content[p:p + S])
        for at in (0, F - 1, (F - 1 + S) // 2, S - 1):
            for c in b"ACGT":
                if c != km[at]:
                    out.append(km[:at] + bytes([c]) + km[at + 1:])
    return out


@pytest.mark.parametrize("kind", ["random", "low-complexity"])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_table_census(gpu, texts, geometry, kind):
    S, opts, want_tables = GEOMETRIES[geometry]
    hi, cen = texts(kind, S)
    assert cen.at[-1] == (0 if kind == "random" else 3 if S == 20 else cen.at[-1])
    if kind == "random":
        assert cen.at[0] == 1 and cen.first_positions(cen.code_at[:1])[0] == 0      # A^S, unique, at position 0
    di = index.DeviceIndex.upload(hi, gpu, **opts)
    try:
        t = di.tables()
        assert {f: t[f] for f in want_tables} == want_tables, t
        if "crowded" in geometry:
            assert t["seed_table_side_entries"] > 1000, t
        n_located = _census_of_the_device(di, hi, cen, S)
        if geometry.startswith("sd"):
            assert n_located > len(cen.at)          # most S-mers are unique: they carry their positions (4 roles each)
        # S-mers the text does not hold (and a few it does: whatever the census says)
        rng = np.random.default_rng(S)
        kms = _neighbours(hi.content(), cen, S, t["seed_table_share"] or 4, rng)
        codes = np.array([K.pack(x) for x in kms], dtype=np.uint64)
        assert (cen.count_codes(codes) == 0).mean() > 0.9
        for lo in range(0, len(kms), 4000):
            part = kms[lo:lo + 4000]
            rr, k, l = _device_seeds(di, K.read_of(part), S)
            step = np.arange(len(part)) * (S + 1)
            _check_against_census(rr[step], k[step], l[step], codes[lo:lo + 4000], cen, hi.sa(), ("neighbours", lo))
    finally:
        di.close()


def _rows(reads):
    arr = np.zeros((len(reads), max(len(r) for r in reads) + 1), dtype=np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return arr, np.array([len(r) for r in reads], dtype=np.uint32)


@pytest.mark.parametrize("tables", ["auto", "sd-counts2", "sd-share2-crowded-counts2", "14-5byte-side"])
def test_low_complexity_reads_vs_oracle(gpu, texts, tables):
    """Reads made of the planted k-mers (counts 1 .. 4 across the saturated count code, thres - 1 / thres / thres + 1 for
    thres = 50 and 300) and windows over the runs, the ends and the boundaries of the text, under both vote paths and
    every round policy."""
    hi, cen = texts("low-complexity", 20)
    w = K.low_complexity()
    reads, lens = K.lowc_reads(w, hi.content())
    oi = orc.OracleIndex.from_host_index(hi)
    opts = {"auto": {}, "sd-counts2": _sd(cbits=2), "sd-share2-crowded-counts2": _sd(share=2, bits=14, cbits=2),
            "14-5byte-side": GEOMETRIES["14-5byte-side"][1]}[tables]
    di = index.DeviceIndex.upload(hi, gpu, **opts)
    try:
        for thres in (50, 300):
            want, _ = oi.seed_batch(reads, lens, 20, thres)
            assert (want["val"] > 0).sum() >= len(lens) - 2
            for exact in (0, 1):
                for rounds in (0, 1, 2):
                    di.set_map_options(vote_exact_only=exact, seed_rounds=rounds)
                    got = mapper.seed_batch(di, reads, lens, 20, thres)
                    assert np.array_equal(got, want), (thres, exact, rounds, np.nonzero(got != want)[0][:8])
    finally:
        di.close()


CASES = [(n, 1) for n in K.VOTE_CASES] + [(n, 30) for n in K.SCALED_CASES]


@pytest.mark.parametrize("name,scale", CASES, ids=["%s-x%d" % c for c in CASES])
def test_constructed_vote(gpu, name, scale):
    """One constructed phase-0 vote (tests/constructed.py: vote_case) against the oracle and against the winner the
    construction prescribes, through the fast kernel, through the exact kernel alone, and with the workgroup tier of the
    exact kernel cut into passes of 100 hits over a 512-slot table (lrm_debug_set_vote_limits; items of more than 192
    hits -- the x30 cases and the long ones -- take that tier).

    FB_LIMIT = 1536 survivors, the largest item of the fast kernel's workgroup form, and 1537, the first it hands to the
    exact kernel: nothing in test_vote_* or the long-read configurations pins that boundary (their items have 64 .. 130
    or ~1200 survivors), so settle-survivors-1536 / -1537 do."""
    c = K.vote_case(name, scale)
    hi = _host([c["seq"]])
    oi = orc.OracleIndex.from_host_index(hi)
    read = c["read"]
    reads, lens = _rows([read, read, c["seq"][len(read) + 64:len(read) + 64 + 700]])
    want, phases = oi.seed_batch(reads, lens, 20, c["thres"])
    key, val = c["expect"]
    assert phases[0] == 1 and want["val"][0] == val and (key is None or want["key"][0] == key)
    if name.startswith("settle-survivors"):
        tr = oi.seed_read(read, 20, c["thres"], trace=True)
        assert sum(1 for j, rr, _, _ in tr["seeds"] if j % 21 == 0 and 0 < rr < c["thres"]) == int(name.split("-")[-1])
    di = index.DeviceIndex.upload(hi, gpu)
    try:
        for exact, limits in ((0, None), (1, None), (0, (100, 512)), (1, (100, 512))):
            di.set_map_options(vote_exact_only=exact)
            di.debug_set_vote_limits(*(limits or (0, 0)))
            got = mapper.seed_batch(di, reads, lens, 20, c["thres"])
            assert np.array_equal(got, want), (name, exact, limits, got[:2], want[:2])
    finally:
        di.close()
