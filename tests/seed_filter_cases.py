"""Constructed batches for the presence bitmap in front of seed_search_kernel's table-line fetch (index_tables.hip:
sd_filter_build; seed_kernels.hip: sd_issue_filtered).  A clear bit stands for a table line of zeros, so a seed whose bit
is clear is "absent" without a fetch: what can go wrong is a bit wrongly clear (a seed of the text is lost) and the loop
around the fetch (a wavefront none of whose lanes fetches, one quad that does among fifteen that do not, the ends of a read).

One text: 20 kbp of random bases with a 150-base string in three copies, indexed with its reverse complement (40 kbp).
Every batch states a property of its reads against the TEXT alone; tests/test_seed_filter_cases_cpu.py proves each by brute
force (constructed.census), tests/test_gpu_seed_filter.py runs them."""
import numpy as np

import constructed as K
from longreadmapper_amd import synth

S, P, THRES = 20, 21, 300
FWD = 20_000
REP, REP_AT = 150, (2_000, 9_000, 15_500)
TILE = 1_000                                    # batch "tile": window step; a window is TILE + S bases
STRETCH = 24                                    # batch "stretch": clean bases of a read (STRETCH - S + 1 = 5 seed positions)
# first position of the clean stretch: 0 .. 3 within a quad (inside wavefront 1 of the first iteration), across a 64-lane
# boundary, across the 256-position iteration boundary and across the 2048-position workgroup boundary
STRETCH_AT = (68, 69, 70, 71, 62, 254, 2046)
STRETCH_LEN = 2_300
HOLE_LEN, HOLE_AT = 420, (150, 255)             # batch "stretch": clean reads with ONE substituted base
LENGTHS = (19, 20, 21, 63 + 20, 64 + 20, 2047 + 20, 2048 + 20, 2049 + 20, 4097 + 20)
BATCHES = ("tile", "random", "stretch", "lengths", "ont")

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def forward():
    """The forward sequence (bytes)."""
    rng = np.random.default_rng(1901)
    a = np.frombuffer(K._filler(rng, FWD), dtype=np.uint8).copy()
    rep = np.frombuffer(K._filler(rng, REP), dtype=np.uint8)
    for at in REP_AT:
        a[at:at + REP] = rep
    return bytes(a)


def _other(a, rng):
    """Every base of the array replaced by another one."""
    return _ACGT[(K._CODE[a] + rng.integers(1, 4, size=len(a))) % 4]


def stretch_read(seq, at, rng):
    """A window of the text in which every third base is substituted, and the two bases around [at, at + STRETCH) too,
    but for the STRETCH bases from `at`: the only S-mers of the read that the text can hold start at at .. at + STRETCH - S."""
    a = np.frombuffer(seq[3_000:3_000 + STRETCH_LEN], dtype=np.uint8).copy()
    hit = np.zeros(len(a), dtype=bool)
    hit[::3] = True
    hit[at - 1] = hit[at + STRETCH] = True
    hit[at:at + STRETCH] = False
    a[hit] = _other(a[hit], rng)
    return bytes(a)


def hole_read(seq, at, rng):
    """A clean window with one substituted base at `at`: the S positions at - S + 1 .. at lose their seed, five quads of a
    wavefront whose other quads keep theirs."""
    a = np.frombuffer(seq[11_000:11_000 + HOLE_LEN], dtype=np.uint8).copy()
    a[at:at + 1] = _other(a[at:at + 1], rng)
    return bytes(a)


def batch(name, seq):
    """The reads (list of bytes) of one batch over the forward sequence `seq`."""
    rng = np.random.default_rng(1902 + BATCHES.index(name))
    if name == "tile":
        # every S-mer of the text, both strands: the indexed text is the sequence followed by its reverse complement, and
        # windows of TILE + S bases (TILE seed positions each: a read's last S-mer is no seed) tile it without a gap, the
        # junction of the strands included.  The S-mer on the text's last base is the one the reference never reports.
        text = seq + K.revcomp(seq)
        return [text[a:a + TILE + S] for a in range(0, len(text) - S, TILE)]
    if name == "random":          # independent random sequence: no seed of any read is in the text
        return [K._filler(rng, n) for n in (3_000, 3_000, 2_048 + S, 4_096 + S, 257 + S, 64 + S, 700, 5_000)]
    if name == "stretch":
        return [stretch_read(seq, at, rng) for at in STRETCH_AT] + [hole_read(seq, at, rng) for at in HOLE_AT]
    if name == "lengths":         # odd and even iteration counts of the two-way unrolled loop, its tails, reads without a seed
        return [seq[4_000 + 37 * i:4_000 + 37 * i + n] for i, n in enumerate(LENGTHS)]
    assert name == "ont"          # 64 reads of 3 kbp with the ONT error profile, both strands
    r = synth.reads([np.frombuffer(seq, dtype=np.uint8)], 64, 3_000, profile=synth.ONT, seed=1903, nthreads=1)
    assert set(r["strand"].tolist()) == {0, 1}
    return [bytes(r["reads"][i, :int(r["lens"][i])]) for i in range(64)]


def rows(reads):
    arr = np.zeros((len(reads), max(len(r) for r in reads) + 1), dtype=np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return arr, np.array([len(r) for r in reads], dtype=np.uint32)


def seed_counts(read, cen):
    """Occurrences in the text of the S-mer at every seed position j < len - S of the read (the reference leaves the last
    S-mer of a read out: alnmain.c:353)."""
    nj = max(len(read) - S, 0)
    if nj == 0:
        return np.zeros(0, dtype=np.int64)
    return cen.count_codes(K._codes(np.frombuffer(read, dtype=np.uint8), S)[:nj])
