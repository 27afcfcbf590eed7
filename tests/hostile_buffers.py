"""Hostile buffers: one batch of reads in layouts whose bytes OUTSIDE the reads are live, and output tensors embedded in guard
fill.  The answer of every stage is a function of (reads[i, :lens[i]], lens) alone and a stage writes inside its outputs'
extents only; tests/test_hostile_buffers_cpu.py checks the premises on the references, tests/test_gpu_hostile_buffers.py
demands both of the device entries.

    batch()                         the text (two sequences, a 250-copy repeat family, an exact two-copy repeat), ~60 reads
                                    of the dword / 64-base / 1-KiB / RC_SEG edge lengths, and their continuations in the text
    build(b, layout, shift)         -> Buffer: the allocation of a layout, its base moved `shift` bytes in, D decoy rows
    references(b, reads2d)          the CPU references of every stage over rows in any layout
    guarded(mapper.DeviceMapper)    a DeviceMapper whose every output tensor lies in 0xA5 fill, op rows wider than needed
"""
import contextlib
import zlib

import numpy as np

import anchored_ref
import clip_ref
import mapq_ref
import orc
import rival_ref
import split_ref
import workloads
from gact_cases import rnd
from longreadmapper_amd import index, synth
from longreadmapper_amd.records import store_need, units16

M = 4097                                      # max_len of the batch
D = 8                                         # decoy rows behind row n of every input array, spare rows behind row n of every output
G = 3                                         # guard rows in front of and behind every output tensor
FILL = 0xA5
GACT = (320, 120, 128)
LENGTHS = (21, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
ONT = (0.04, 0.03, 0.03)
HARD = (0.09, 0.05, 0.05)                     # noisy enough for several seed phases
TWO_A, TWO_B, TWO_LEN = 10_000, 50_000, 8_000           # sequence 1: [TWO_A, +TWO_LEN) copied to [TWO_B, +TWO_LEN)
LAYOUTS = {                                   # name -> (stride, fill rule)
    "plain": (M + 1, "zero"),
    "text-pad-1": (M + 1, "text"),
    "text-pad-2": (M + 2, "text"),
    "acgt-pad": (M + 2, "acgt"),
    "lower-pad": ((M + 16) & ~15, "lower"),
    "ff-pad": (M + 1, "ff"),
    "abutting": (M, "text"),
}
_cache = {}


def _noisy(rng, src, at, length, sub, ins, dele):
    """Bases of src from `at` on, mutated, until `length` bases are out -> (read, source bases consumed)."""
    out, k = bytearray(), at
    while len(out) < length:
        c = src[k]
        k += 1
        x = rng.random()
        if x < dele:
            continue
        if x < dele + sub:
            c = b"ACGT"[(b"ACGT".index(c) + 1 + int(rng.integers(3))) % 4]
        out.append(c)
        if len(out) < length and rng.random() < ins:
            out.append(b"ACGT"[int(rng.integers(4))])
    return bytes(out), k - at


def _text():
    fam, elem = workloads.repeat_reference(250, 800, 500, seed=16)
    two = synth.reference(80_000, seed=17).copy()
    two[TWO_B:TWO_B + TWO_LEN] = two[TWO_A:TWO_A + TWO_LEN]
    return [fam, two], elem


def batch():
    """-> dict(seqs, hi, elem, reads [bytes], lens, tails [bytes: what follows the read's source in the text, read-oriented,
    M + 32 bases], spec [(kind, seq, strand)], n)"""
    if "batch" in _cache:
        return _cache["batch"]
    seqs, elem = _text()
    hi = index.HostIndex.build(seqs, names=["fam", "two"], hlen=8)
    rng = np.random.default_rng(2024)
    oriented = {(s, st): bytes(seqs[s]) if st == 0 else bytes(anchored_ref.revcomp(seqs[s])) for s in (0, 1) for st in (0, 1)}
    reads, tails, spec = [], [], []

    def add(kind, seq, strand, pos, length, noise=None, junk=0, at_end=False, exact_tail=0, n_at=None):
        """`length` read bases of sequence `seq` from forward position `pos` on (reverse strand: of the window of that many
        bases and a margin that starts there); junk: that many random bases replace the read's end; exact_tail: the last
        bases in front of them are copied, not mutated; n_at: an 'N' replaces that base."""
        src = oriented[(seq, strand)]
        room = length + length // 6 + 64 if noise else length
        a = len(src) - room if at_end else pos if strand == 0 else len(src) - pos - room
        body = length - junk - exact_tail
        if noise:
            rd, used = _noisy(rng, src, a, body, *noise)
        else:
            rd, used = src[a:a + body], body
        rd += src[a + used:a + used + exact_tail]
        used += exact_tail
        if n_at is not None:
            rd = rd[:n_at] + b"N" + rd[n_at + 1:]
        rd += rnd(junk, "junk", len(reads))
        follow = src[a + used + junk:a + used + junk + M + 32]
        follow += rnd(M + 32 - len(follow), "past the sequence", len(reads))
        reads.append(rd)
        tails.append(follow)
        spec.append((kind, seq, strand))

    free = [(19_000, 44_000), (59_000, 74_000)]                         # sequence 1 outside the two copies
    def place(length):
        lo, hi_ = free[int(rng.integers(2))]
        return int(rng.integers(lo, hi_ - length - length // 6 - 64))

    for length in LENGTHS:
        for strand in (0, 1):
            noise = None if length < 1000 else (HARD if length in (1023, 2048) else ONT)
            add("edge", 1, strand, place(length), length, noise)
    for strand in (0, 1, 0):                                            # full length, noisy
        add("full", 1, strand, place(M), M, ONT)
    for k, (length, junk) in enumerate(((3000, 700), (2100, 300), (4097, 900), (1500, 260))):
        add("junk", 1, k % 2, place(length), length, ONT, junk=junk)
    for k, (length, off) in enumerate(((2500, 300), (3000, 2000), (1800, 5000), (4096, 1000), (1200, 6500))):
        add("two-copy", 1, k % 2, (TWO_A if k % 2 == 0 else TWO_B) + off, length, ONT)
    for k, length in enumerate((500, 640, 2600)):                       # inside / across elements of the 250-copy family
        add("family", 0, k % 2, 40_000 + 1300 * k + 520, length, None if length < 1000 else ONT)
    # a non-ACGT base (the read is flagged: byte kernels and the bytewise anchor scan serve it) and, behind noise, an exact
    # end that is the read's longest match: under text padding the match goes on behind the read
    for k, length in enumerate((2049, 1500, 1027)):
        add("flagged", 1, k % 2, place(length), length, HARD, exact_tail=90, n_at=100 + 7 * k)
    add("seq-end", 1, 0, 0, 1300, None, at_end=True)                    # ends on the last base of sequence 1
    add("seq-end", 1, 1, 0, 333, None, at_end=True)                     # reverse strand: the sequence's first bases
    add("seq-end", 0, 0, 0, 129, None, at_end=True)

    # order: shuffled; two full-length reads in consecutive rows, one in the last row
    n = len(reads)
    full = [i for i, r in enumerate(reads) if len(r) == M]
    assert len(full) >= 4
    rest = [i for i in range(n) if i not in full[:3]]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    order = rest[:20] + full[:2] + rest[20:] + full[2:3]
    b = dict(seqs=seqs, hi=hi, elem=elem, n=n, reads=[reads[i] for i in order], tails=[tails[i] for i in order],
             spec=[spec[i] for i in order], lens=np.array([len(reads[i]) for i in order], dtype=np.uint32))
    _cache["batch"] = b
    return b


class Buffer:
    """alloc: every byte of the allocation (uint8); rows: the (n + D, stride) view behind the moved base; lens: n + D"""

    def __init__(self, alloc, shift, stride, lens):
        self.alloc, self.shift, self.stride, self.lens = alloc, shift, stride, lens
        self.rows = alloc[shift:shift + len(lens) * stride].reshape(len(lens), stride)


def _pad(rule, tail, count, key):
    if rule == "zero":
        return np.zeros(count, dtype=np.uint8)
    if rule == "ff":
        return np.full(count, 0xFF, dtype=np.uint8)
    if rule == "text":
        return np.frombuffer(tail[:count], dtype=np.uint8)
    rng = np.random.default_rng([zlib.crc32(repr(key).encode()), count])
    return np.frombuffer(b"ACGT" if rule == "acgt" else b"acgt", dtype=np.uint8)[rng.integers(0, 4, count)]


def build(b, layout, shift=0):
    """The batch in a layout: rows at the layout's stride behind a base moved `shift` bytes into the allocation, D decoy rows
    (copies of rows n-D .. n-1, padding included: the last one is a full-length read) behind row n.  The allocation ends on
    the last row's last byte."""
    stride, rule = LAYOUTS[layout]
    n = b["n"]
    src = list(range(n)) + list(range(n - D, n))
    lens = np.array([b["lens"][i] for i in src], dtype=np.uint32)
    alloc = np.empty(shift + len(src) * stride, dtype=np.uint8)
    alloc[:shift] = _pad("zero" if rule == "zero" else "acgt", b"", shift, ("front", layout))
    buf = Buffer(alloc, shift, stride, lens)
    for row, i in enumerate(src):
        k = int(lens[row])
        buf.rows[row, :k] = np.frombuffer(b["reads"][i], dtype=np.uint8)
        buf.rows[row, k:] = _pad(rule, b["tails"][i], stride - k, (layout, i))
    return buf


def shift_of(layout):
    """the 1 .. 15 bytes the moved base of a layout is moved by: a different residue per layout"""
    return 1 + (3 + 4 * list(LAYOUTS).index(layout)) % 15


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def mta_of(hi):
    return [(o, l) for _, o, l in hi.mta()]


def extension_ref(b, oi, rows, lens, best, mode):
    """The extension of a mode over rows (n, stride) with best[] -> dict(n_ops, score, meta_r, loc, off, seq_id, strand, ops
    [bytes], anchor / clip_left / clip_right where the mode has them); rows are oriented in place like the oracle does."""
    hi = b["hi"]
    classic = oi.extend_batch(rows, lens, best, GACT)
    n = len(lens)
    out = dict(meta_r=classic["meta_r"].copy(), seq_id=classic["meta"]["seq_id"].copy(), strand=classic["meta"]["strand"].copy(),
               n_ops=classic["n_ops"].copy(), score=classic["score"].copy(), loc=classic["meta"]["loc"].astype(np.int64),
               off=classic["meta"]["off"].astype(np.int64), ops=[bytes(classic["ops"][i, :max(int(classic["n_ops"][i]), 0)]) for i in range(n)])
    if mode == "classic":
        return out
    fn = anchored_ref.extend_batch if mode == "anchored" else clip_ref.extend_clipped_batch
    ext = fn(hi.content(), mta_of(hi), rows, lens, classic["meta"], classic["meta_r"], GACT)
    out["anchor"] = np.zeros((n, 6), dtype=np.int64)
    out["clip_left"], out["clip_right"] = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i, e in enumerate(ext):
        if e is None:
            out["n_ops"][i], out["score"][i], out["ops"][i] = 0, -1, b""
            continue
        out["n_ops"][i], out["score"][i], out["ops"][i], out["loc"][i], out["off"][i] = e["n_ops"], e["score"], e["ops"], e["loc"], e["off"]
        out["anchor"][i] = [e[k] for k in ("text_pos", "read_pos", "len", "delta", "left_ops", "flags")]
        out["clip_left"][i], out["clip_right"][i] = e.get("clip_left", 0), e.get("clip_right", 0)
    return out


def fenced(rows, lens):
    """a copy of rows with every non-ACGT read base mapped like the device's seed stage maps it"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = rows.copy()
    for i in range(len(lens)):
        r = out[i, :lens[i]]
        other = ~np.isin(r, acgt)
        r[other] = acgt[((r[other] >> 1) ^ (r[other] >> 2)) & 3]
    return out


def references(b, rows, lens, modes=("classic", "anchored", "clipped"), second=True):
    """Every reference over the first len(lens) rows of `rows` (any stride, any bytes outside the reads); rows is left as the
    oracle's extension leaves it.  -> dict(best, phases, mapq, rival, <mode>: extension_ref, split, secondary)"""
    hi = b["hi"]
    oi = orc.OracleIndex.from_host_index(hi)
    n = len(lens)
    before = rows.copy()
    # the seed side of the oracle is defined for ACGT only: a non-ACGT read base goes through the fence of DESIGN section 3,
    # ((c >> 1) ^ (c >> 2)) & 3 ('N' -> 'A'), here as on the device; the extension side takes the reads as they are
    seeded = fenced(rows, lens)
    best, phases = oi.seed_batch(seeded, lens)
    mq, _ = mapq_ref.batch(oi, seeded, lens)
    rival = rival_ref.batch(oi, seeded, lens)
    assert np.array_equal(rows, before)
    ref = dict(best=best, phases=phases, mapq=mq, rival=rival)
    for mode in modes:
        work = before.copy()
        ref[mode] = extension_ref(b, oi, work, lens, best, mode)
        ref["oriented"] = work
    rows[...] = ref["oriented"]
    if not second:
        return ref
    # split: the segments of the clipped mode, mapped as reads of their own
    cl = ref["clipped"]
    table = split_ref.plan(lens, cl["clip_left"], cl["clip_right"])
    seg_lens = np.array([t[2] for t in table], dtype=np.uint32)
    seg_rows = np.zeros((len(table), M + 1), dtype=np.uint8)
    for s, (read, start, ln, _) in enumerate(table):
        seg_rows[s, :ln] = rows[read, start:start + ln]
    seg_best, _ = oi.seed_batch(fenced(seg_rows, seg_lens), seg_lens)
    ref["split"] = dict(table=table, lens=seg_lens, best=seg_best, ext=extension_ref(b, oi, seg_rows, seg_lens, seg_best, "clipped"),
                        rows=seg_rows)
    # secondary: the candidates as sequenced, extended from their rival entries in the clipped mode
    cand = rival_ref.plan(mq)
    assert np.array_equal(cand, np.flatnonzero(rival[:, 1] > 0))
    sec_lens = lens[cand].astype(np.uint32)
    sec_rows = np.zeros((len(cand), M + 1), dtype=np.uint8)
    for s, i in enumerate(cand):
        sec_rows[s, :lens[i]] = before[i, :lens[i]]
    sec_best = np.zeros(len(cand), dtype=orc.ENTRY_DT)
    sec_best["key"], sec_best["val"], sec_best["bucket"] = rival[cand, 0], rival[cand, 1], rival[cand, 2]
    ext = extension_ref(b, oi, sec_rows, sec_lens, sec_best, "clipped")
    prim = ref["clipped"]
    same_place = (prim["meta_r"][cand] != 0) & (ext["meta_r"] != 0) & (ext["seq_id"] == prim["seq_id"][cand]) & \
        (ext["strand"] == prim["strand"][cand]) & (np.abs(ext["off"] - prim["off"][cand]) < lens[cand].astype(np.int64) // 2)
    reported = (ext["meta_r"] != 0) & (ext["score"] != -1) & ~same_place & ((ext["anchor"][:, 5] & anchored_ref.ANCHORED) != 0)
    ref["secondary"] = dict(cand=cand, lens=sec_lens, best=sec_best, ext=ext, rows=sec_rows,
                            flags=(reported * rival_ref.SEC_ALIGNED + same_place * rival_ref.SEC_DUPLICATE).astype(np.uint32))
    return ref


def same_references(a, c):
    """-> the names of what differs between two references() results (the oriented rows, padding included, are not compared)"""
    bad = [k for k in ("best", "phases", "mapq", "rival") if k in a and a[k].tobytes() != c[k].tobytes()]

    def ext_differs(x, y):
        return [k for k in x if (x[k] != y[k] if k == "ops" else not np.array_equal(x[k], y[k]))]
    for mode in ("classic", "anchored", "clipped"):
        if mode in a:
            bad += [(mode, k) for k in ext_differs(a[mode], c[mode])]
    for stage in ("split", "secondary"):
        if stage in a:
            x, y = a[stage], c[stage]
            bad += [(stage, k) for k in x if k != "ext" and (x[k] != y[k] if k == "table" else not np.array_equal(x[k], y[k]))]
            bad += [(stage, k) for k in ext_differs(x["ext"], y["ext"])]
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# guarded outputs
# ---------------------------------------------------------------------------------------------------------------------
def op_extent(mode, n_ops, abandoned, length, exact=True):
    """The first op-row byte a mode's extension leaves alone.  exact: what every store path does today -- the tail stores
    of the byte kernels, bs_expand16 (`left` bytes), the anchored stitch (`total` bytes) all end on byte n_ops -- and what the
    tests assert, on purpose tighter than the contract; not exact: the contract of include/lrm_accel.h, "Written extents", n_ops
    rounded up to 4 (classic) or 16 (anchored, clipped), which a kernel that comes to store whole groups may use -- the
    tests then move to it.  Either way a read without an alignment has n_ops == 0 and nothing is written, except the classic
    mode's abandoned alignment (a locus, score -1): the columns it can have had, 2 * length."""
    if n_ops <= 0:
        return 2 * length if mode == "classic" and abandoned else 0
    if exact:
        return n_ops
    return (n_ops + 3) // 4 * 4 if mode == "classic" else units16(n_ops)


def guarded(base):
    """base (mapper.DeviceMapper) -> a subclass whose every output tensor lies in FILL: G guard rows either side, and op rows
    of units16(store_need) + 48 bytes.  check_guards(used) asserts the fill."""

    class Guarded(base):
        _ss = 0

        @property
        def store_stride(self):
            return self._ss

        @store_stride.setter
        def store_stride(self, v):                       # (DeviceMapper sets what the mode needs: the rows become wider)
            self._ss = units16(v) + 48

        def _alloc(self, shape, dtype):
            shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
            row = int(np.prod(shape[1:], dtype=np.int64)) * dtype.itemsize
            raw = self.torch.full(((shape[0] + 2 * G) * row,), FILL, dtype=self.torch.uint8, device=self.dev)
            t = raw.view(dtype).view((shape[0] + 2 * G,) + shape[1:])[G:G + shape[0]]
            self.__dict__.setdefault("_guards", []).append((raw, row, shape[0], t))
            return t

        def raw_of(self, t):
            """every byte of the allocation around output tensor t as a (G + rows + G, row bytes) numpy array"""
            for raw, row, rows, mine in self._guards:
                if mine.data_ptr() == t.data_ptr():
                    return raw.cpu().numpy().reshape(rows + 2 * G, row)
            raise KeyError("not an output tensor of this mapper")

        def check_guards(self, t, used, what):
            """rows >= used of tensor t and its guard rows are FILL -> the rows [0, used) as bytes"""
            a = self.raw_of(t)
            assert (a[:G] == FILL).all(), (what, "guard rows in front")
            assert (a[G + used:] == FILL).all(), (what, "rows >= %d or the guard rows behind" % used,
                                                  np.flatnonzero((a[G + used:] != FILL).any(axis=1))[:4].tolist())
            return a[G:G + used]

        def refill(self):
            """every output tensor and its guard rows back to FILL: between two batches on one mapper"""
            for raw, _, _, _ in self._guards:
                raw.fill_(FILL)

        @contextlib.contextmanager
        def batch_max_len(self, max_len):
            """the calls inside pass max_len (<= the workspace's) as the batch's: a smaller batch on a larger workspace"""
            assert max_len <= self.max_len
            mine, self.max_len = self.max_len, max_len
            try:
                yield self
            finally:
                self.max_len = mine

    Guarded.__name__ = "Guarded" + base.__name__
    return Guarded
