"""Constructed inputs for the two stages that build a compact second batch on the device (csrc/compact_rows.h: split reads,
secondary alignments), shared by tests/test_compact_cases_cpu.py and tests/test_gpu_compact_rows.py.

    order_pattern()        which reads of a batch of 65 536 + 256 + 37 carry a row: more than one workgroup of the count /
                           mark kernels, more than one tile of the scan kernel, every lane and wavefront edge
    split_order_case()     clip counts and reads (100 .. 400 bases) that give that pattern in the split stage
    secondary_records()    lrm_mapq records that give that pattern in the secondary stage
    gather_lengths         row lengths on, just before and just behind the 4096-byte chunk edges of the gather kernels
    split_gather_case()    reads and clip counts whose segments have those lengths, at the tightest row stride
    long_chimeras()        genuine reads between junk heads and tails of more than 4096 bases
    secondary_gather_case()  reads of those lengths inside an exact two-copy repeat, both strands at every length

Every builder asserts that its output has the edges it claims."""
import numpy as np

from longreadmapper_amd import synth
from longreadmapper_amd.records import CLIP_DT, MAPQ_DT, MAPQ_OVERFLOW

SP_BLOCK, SP_CHUNK, WAVE = 256, 4096, 64            # csrc/compact_rows.h
N_ORDER = 65_536 + 256 + 37                         # 258 workgroups, the last one partial; not a multiple of 64
M = 50                                              # the smallest legal split_min_len
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)

ROW_AT = (0, 63, 64, 127, 128, 255, 256, 257, 511, 512, 65_535, 65_536, 65_537, N_ORDER - 1)
TWO_AT = (255, 65_535, N_ORDER - 1)                 # split: two-segment reads in a workgroup's / a tile's last lane
WG_FULL, WG_EMPTY, WG_LAST_LANE, WG_WAVE3_LANE0 = 5, 7, 9, 11


def order_pattern(n=N_ORDER):
    """-> bool (n,): the reads that carry a row in the second batch."""
    assert n == N_ORDER, "the edges below are placed for this n"
    rng = np.random.default_rng(20_261)
    p = rng.random(n) < 1 / 6
    p[list(ROW_AT)] = True
    wg = lambda g: slice(g * SP_BLOCK, (g + 1) * SP_BLOCK)
    p[wg(WG_FULL)] = True
    p[wg(WG_EMPTY)] = False
    p[wg(WG_LAST_LANE)] = False
    p[WG_LAST_LANE * SP_BLOCK + SP_BLOCK - 1] = True
    p[wg(WG_WAVE3_LANE0)] = False
    p[WG_WAVE3_LANE0 * SP_BLOCK + 3 * WAVE] = True
    check_order_pattern(p)
    return p


def check_order_pattern(p):
    n = len(p)
    n_blk = (n + SP_BLOCK - 1) // SP_BLOCK
    assert n == N_ORDER and n_blk == 258 and n % SP_BLOCK == 37 and n % WAVE != 0
    assert all(p[i] for i in ROW_AT)
    per = np.add.reduceat(p.astype(np.int64), np.arange(0, n, SP_BLOCK))
    assert len(per) == n_blk
    assert per[WG_FULL] == SP_BLOCK and per[WG_EMPTY] == 0
    assert per[WG_LAST_LANE] == 1 and p[WG_LAST_LANE * SP_BLOCK + 255]
    assert per[WG_WAVE3_LANE0] == 1 and p[WG_WAVE3_LANE0 * SP_BLOCK + 192]
    assert (per[[254, 255, 256, 257]] > 0).all()                   # both scan tiles, both sides of the tile edge
    assert per[:256].sum() > 0 and per[256:].sum() > 0
    assert int(p.sum()) % SP_BLOCK != 0
    assert 0.14 < p.mean() < 0.20                                   # about 1 in 6
    return per


# ---------------------------------------------------------------------------------------------------------
# split: clips from the pattern
# ---------------------------------------------------------------------------------------------------------
def _kinds(ln):
    """The seven (cl, cr) kinds of a read of ln bases that has a segment; the number of segments of each."""
    return [(M, 0), (0, M), (M, M), (M - 1, M), (M, M - 1), (ln, 0), (ln + 5, 0)], (1, 1, 2, 1, 1, 1, 1)


def small_reference():
    return synth.reference(200_000, seed=97)


def clip_records(cl, cr):
    c = np.zeros(len(cl), dtype=CLIP_DT)
    c["left"], c["right"] = cl, cr
    return c


def split_order_case():
    """-> dict(ref, reads (n, 401), lens, cl, cr, kind (-1: no row), pattern)"""
    p = order_pattern()
    n = len(p)
    rng = np.random.default_rng(20_262)
    lens = rng.integers(100, 401, n).astype(np.uint32)
    lens[[0, 1, 2, 3]] = (100, 400, 101, 399)
    kind = np.where(p, rng.integers(0, 7, n), -1)
    kind[list(TWO_AT)] = 2
    kind[[0, 63, 64, 127, 128, 256, 257]] = (0, 1, 2, 3, 4, 5, 6)
    cl, cr = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for k in range(7):
        at = np.flatnonzero(kind == k)
        assert len(at) > 0
        for i in at:
            cl[i], cr[i] = _kinds(int(lens[i]))[0][k]
    none = np.flatnonzero(~p)
    below = rng.integers(0, M, (len(none), 2)).astype(np.uint32)
    below[::3] = (M - 1, M - 1)
    below[1::7] = (0, 0)
    cl[none], cr[none] = below[:, 0], below[:, 1]
    assert (cl[none] < M).all() and (cr[none] < M).all() and ((cl[none] == M - 1) & (cr[none] == M - 1)).any()
    has = (np.minimum(cl, lens) >= M) | (np.minimum(cr, lens) >= M)
    assert np.array_equal(has, p)
    assert (lens.min(), lens.max()) == (100, 400)
    ref = small_reference()
    reads = synth.reads([ref], n, 400, synth.ONT, seed=98)["reads"]
    reads *= (np.arange(401)[None, :] < lens[:, None]).astype(np.uint8)          # NUL behind every read's end
    return dict(ref=ref, reads=reads, lens=lens, cl=cl, cr=cr, kind=kind, pattern=p)


# ---------------------------------------------------------------------------------------------------------
# secondary: records from the pattern
# ---------------------------------------------------------------------------------------------------------
def secondary_records(p):
    """lrm_mapq records: a candidate (n1 = 20, n2 = 12) where p, otherwise one of the four kinds that are none."""
    rng = np.random.default_rng(20_263)
    rec = np.zeros(len(p), dtype=MAPQ_DT)
    kind = np.where(p, -1, rng.integers(0, 4, len(p)))
    rec["n1"][p], rec["n2"][p] = 20, 12
    for k, (n1, n2, flags) in enumerate(((20, 7, 0), (19, 9, 0), (20, 12, MAPQ_OVERFLOW), (0, 0, 0))):
        at = kind == k
        assert at.any()
        rec["n1"][at], rec["n2"][at], rec["flags"][at] = n1, n2, flags
    rec["radius"][rec["n1"] > 0] = 512
    return rec


# ---------------------------------------------------------------------------------------------------------
# gather: rows longer than one chunk
# ---------------------------------------------------------------------------------------------------------
gather_lengths = (4080, 4095, 4096, 4097, 4111, 4112, 8191, 8192, 8193, 8207, 12_287, 12_288, 12_289)
MAX_LEN = 12_289
assert {x % 16 for x in gather_lengths} == {0, 1, 15}
assert all(any(abs(x - e) <= 1 for x in gather_lengths) and e in gather_lengths for e in (4096, 8192, 12_288))


def round16(x):
    return (np.asarray(x) + 15) // 16 * 16


def split_gather_case():
    """-> dict(ref, reads (n, 12 290), lens, cl, cr): every length of gather_lengths as a left and as a right segment, one read
    that is one segment of max_len bases, every source phase mod 16 among the segments longer than one chunk."""
    stride = MAX_LEN + 1
    rows = []                                                       # (len, cl, cr)
    for k, g in enumerate(gather_lengths):
        rows.append((min(MAX_LEN, g + 3 * k), g, 0))                # left segment, the read goes on behind it
        rows.append((min(MAX_LEN, g + 100 + k), 0, g))              # right segment
    rows.append((MAX_LEN, MAX_LEN, 0))                              # cl = len = max_len: the tightest stride
    rows.append((MAX_LEN, MAX_LEN + 5, 0))
    rows.append((MAX_LEN, 4097, 8192))                              # two segments that fill the read
    rows.append((8400, 4111, 4112))
    for ph in range(16):                                            # right segments of 8193 bases at every source phase
        i = len(rows)
        start = 16 + (ph - i * stride) % 16
        rows.append((start + 8193, 0, 8193))
    lens = np.array([r[0] for r in rows], dtype=np.uint32)
    cl = np.array([r[1] for r in rows], dtype=np.uint32)
    cr = np.array([r[2] for r in rows], dtype=np.uint32)
    n = len(lens)
    assert lens.max() == MAX_LEN and (np.minimum(cr, lens) + np.minimum(cl, lens) <= lens).all()
    left, right = np.minimum(cl, lens), np.minimum(cr, lens)
    assert set(gather_lengths) <= set(left.tolist()) and set(gather_lengths) <= set(right.tolist())
    assert ((left == lens) & (lens == MAX_LEN)).any() and int(round16(MAX_LEN + 1)) == 12_304
    phases = set()
    for i in range(n):
        if left[i] > SP_CHUNK:
            phases.add((i * stride) % 16)
        if right[i] > SP_CHUNK:
            phases.add((i * stride + int(lens[i]) - int(right[i])) % 16)
    assert phases == set(range(16)), sorted(phases)
    ref = small_reference()
    reads = synth.reads([ref], n, MAX_LEN, synth.ONT, seed=99)["reads"]
    reads *= (np.arange(stride)[None, :] < lens[:, None]).astype(np.uint8)
    return dict(ref=ref, reads=reads, lens=lens, cl=cl, cr=cr)


def long_chimeras(ref, n=16, seed=5):
    """Genuine reads of 2500 .. 3200 bases between junk of 4200 .. 4500 bases (both ends, head only, tail only), at most 12 289
    bases each -> reads (n, 12 290), lens"""
    rng = np.random.default_rng(seed)
    real = synth.reads([ref], n, 3200, synth.ONT, seed=seed + 1)
    stride = MAX_LEN + 1
    reads, lens = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    for i in range(n):
        head = BASES[rng.integers(0, 4, int(rng.integers(4200, 4501)))] if i % 4 != 2 else BASES[:0]
        tail = BASES[rng.integers(0, 4, int(rng.integers(4200, 4501)))] if i % 4 != 3 else BASES[:0]
        piece = real["reads"][i, :int(rng.integers(2500, 3201))]
        whole = np.concatenate([head, piece, tail])
        assert len(whole) <= MAX_LEN
        reads[i, :len(whole)], lens[i] = whole, len(whole)
    return reads, lens


A0, B0, LN = 40_000, 180_000, 60_000                # the exact two-copy repeat of secondary_gather_case


def secondary_gather_case(per_strand=2):
    """-> dict(base, reads (n, 12 290), lens, strand): 300 kbp with an exact 60 kbp two-copy repeat; reads from inside a copy cut
    to gather_lengths, per_strand forward and per_strand reverse reads at every length."""
    base = synth.reference(300_000, seed=91).copy()
    base[B0:B0 + LN] = base[A0:A0 + LN]
    want = 2 * per_strand * len(gather_lengths)
    r = synth.reads([base[A0:A0 + LN]], 2 * want, MAX_LEN, synth.ONT, seed=93)
    take = {0: list(np.flatnonzero(r["strand"] == 0)), 1: list(np.flatnonzero(r["strand"] == 1))}
    assert min(len(take[0]), len(take[1])) >= want // 2
    src, lens, strand = [], [], []
    for g in gather_lengths:
        for s in (0, 1):
            for _ in range(per_strand):
                src.append(take[s].pop(0))
                lens.append(g)
                strand.append(s)
    lens = np.array(lens, dtype=np.uint32)
    reads = r["reads"][src].copy()
    reads *= (np.arange(reads.shape[1])[None, :] < lens[:, None]).astype(np.uint8)
    strand = np.array(strand, dtype=np.uint8)
    assert len(lens) >= 4 * len(gather_lengths)
    for g in gather_lengths:
        assert {int(s) for s in strand[lens == g]} == {0, 1}
    return dict(base=base, reads=reads, lens=lens, strand=strand)
