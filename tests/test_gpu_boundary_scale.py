"""The host boundary (lrm_host.hip) at the size of a real batch: 38 000 ragged ONT reads, 0.38 Gbp, a result image of
~0.6 GB.  At that size a row of the image straddles two pieces of the download ring, the ring laps, the pageable upload
goes through some twenty staging chunks, the two dense buffers of a slot are used again and the automatic plan is the one
that runs -- none of which the 64-read scenarios of test_gpu_boundary.py reach.

The host boundary only moves data, so its reference is cheap and independent:
  A  the device-resident path (DeviceMapper.seed / .extend, downloaded with plain torch copies: nothing of lrm_host.hip
     runs) for EVERY read: op rows, n_ops, score, meta, meta_r, best, the reads after the in-place reverse complement;
  B  the layouts restated on the host: dense = rows[i, :n_ops[i]] at a 16-byte aligned, ascending offset; text =
     lrm_parse_cigar (host C, pinned against sam_ref.rle in test_io_host.py) of the same rows, "*" without an alignment;
     keep_reads = the caller's buffer comes back byte for byte;
  C  the CPU oracle on a sample (every 1 200th read, and the reads of the dense pageable run that straddle two ring
     pieces), which ties reference A to the oracle where the pieces meet.
Every case compares all reads."""
import ctypes as C

import numpy as np
import pytest

import orc
import sam_ref
import workloads
from longreadmapper_amd import index, mapper, synth
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu

# host_pipeline.h: RING_CHUNK (bytes of one pinned piece of the download ring) and N_RING (pieces of the ring).  A download
# of more than N_RING pieces re-uses the first chunk: the ring has lapped.
RING_CHUNK, N_RING = 16 << 20, 16
N_READS, L_MIN, L_MAX = 38_000, 2_000, 18_000
STRIDE, STORE_STRIDE = L_MAX + 1, 2 * L_MAX            # reads start at every byte phase; op rows are a multiple of 16
N_PAST_END = 16
assert STORE_STRIDE % 16 == 0


def _make_reads(ref):
    """~99 % reads of 2 000..18 000 bases (row starts at every phase of a ring piece), the `ragged` scenario's lengths
    (0, 1, 19, 20, 21, 63..65 ...) fifteen times over, 1 % random sequences, and a few reads that run past the end of
    the sequence (seq_lookup fails: meta_r = 0, no ops, "*" in the middle of the image)."""
    rng = np.random.default_rng(5)
    r = synth.reads([ref], N_READS, L_MAX, synth.ONT, seed=29)
    reads = r["reads"]
    lens = rng.integers(L_MIN, L_MAX + 1, size=N_READS).astype(np.uint32)
    ragged = np.asarray(workloads.scenario("ragged")["lens"], dtype=np.uint32)
    special = 1 + rng.choice(N_READS - 1, size=15 * len(ragged) + 360 + N_PAST_END, replace=False)
    short_at, rand_at, end_at = np.split(special, [15 * len(ragged), 15 * len(ragged) + 360])
    lens[0] = L_MAX
    lens[short_at] = np.tile(ragged, 15)
    reads[rand_at, :L_MAX] = synth.reference(len(rand_at) * L_MAX, seed=99).reshape(len(rand_at), L_MAX)
    for i in end_at:
        reads[i, :3000] = ref[-3000:]
        reads[i, 3000:L_MAX] = synth.reference(L_MAX - 3000, seed=1000 + int(i))
        lens[i] = 5000
    for i in range(N_READS):
        reads[i, lens[i]:] = 0
    return reads, lens, end_at


class _Buffers:
    """The caller's batch buffers, allocated once and used again by every case: one pageable set, pinned sets on demand."""

    def __init__(self):
        self.pageable = (np.empty((N_READS, STRIDE), dtype=np.uint8), np.empty((N_READS, STORE_STRIDE), dtype=np.uint8))
        self.pinned = []

    def get(self, pinned, k=0):
        if not pinned:
            return self.pageable
        while len(self.pinned) <= k:
            self.pinned.append((mapper.pinned_empty((N_READS, STRIDE)), mapper.pinned_empty((N_READS, STORE_STRIDE))))
        return self.pinned[k]

    def free(self):
        for r, st in self.pinned:
            mapper.pinned_free(r)
            mapper.pinned_free(st)
        self.pinned = []


@pytest.fixture(scope="module")
def world(gpu):
    import torch
    ref = synth.reference(4_641_652, seed=1, repeat_frac=0.05, rep_len=300, rep_copies=1000, rep_div=0.05)
    hi = index.HostIndex.build([ref], hlen=12)
    di = index.DeviceIndex.upload(hi, gpu)
    reads, lens, end_at = _make_reads(ref)
    # reference A: the device-resident path, plain torch copies down
    dm = mapper.DeviceMapper(di, N_READS, L_MAX, device=gpu)
    assert dm.store_stride == STORE_STRIDE
    d_reads = torch.from_numpy(reads).cuda()
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    dm.seed(d_reads, d_lens)
    dm.extend(d_reads, d_lens)
    torch.cuda.synchronize()
    want = dm.results(N_READS)
    want["reads"] = d_reads.cpu().numpy()
    dm.close()
    del dm, d_reads, d_lens
    torch.cuda.empty_cache()
    rows = want["ops"]
    for i in range(N_READS):                            # bytes behind n_ops are nobody's: zero, like a fresh store_mem
        rows[i, max(int(want["n_ops"][i]), 0):] = 0
    none = (want["n_ops"] <= 0) | (want["meta_r"] == 0) | (want["score"] == -1)
    assert (want["n_ops"] <= STORE_STRIDE).all()
    assert (want["n_ops"] == 0).sum() >= 15 and (want["meta_r"][end_at] == 0).all() and none.sum() < N_READS // 50
    rev = (want["meta_r"] != 0) & (want["meta"]["strand"] == 1)
    assert N_READS // 3 < rev.sum() < 2 * N_READS // 3 and not np.array_equal(want["reads"], reads)
    w = dict(hi=hi, di=di, reads=reads, lens=lens, want=want, none=none, bufs=_Buffers(), texts=None, oi=None, oracle={})
    yield w
    w["bufs"].free()
    di.close()


# ---- reference B: the layouts -------------------------------------------------------------------------------------------------

def _texts(world):
    """Run-length CIGAR text of every read from the reference rows, by the host's lrm_parse_cigar."""
    if world["texts"] is None:
        want, none = world["want"], world["none"]
        buf = C.create_string_buffer(2 * STORE_STRIDE + 16)
        out = []
        for i in range(N_READS):
            if none[i]:
                out.append(b"*")
                continue
            n = lib.lrm_parse_cigar(want["ops"][i].ctypes.data, int(want["n_ops"][i]), buf, len(buf))
            assert n > 0
            out.append(buf.raw[:n])
        for i in range(0, N_READS, 1200):              # ... and the Python restatement itself on a sample
            k = int(want["n_ops"][i])
            assert out[i].decode() == ("*" if none[i] else sam_ref.rle(bytes(want["ops"][i, :k]))), i
        world["texts"] = out
    return world["texts"]


def _units(res):
    """First read of every unit of a dense / text result: a unit's image starts at its first row of store_mem."""
    off = res["ops_off"]
    return np.flatnonzero(off == np.arange(len(off), dtype=np.int64) * STORE_STRIDE)


def _where(off, i, starts):
    u = int(np.searchsorted(starts, i, side="right")) - 1
    rel = int(off) - int(starts[u]) * STORE_STRIDE
    return "read %d, unit %d (reads from %d), image offset %d = piece %d + %d" % (i, u, starts[u], rel, rel // RING_CHUNK, rel % RING_CHUNK)


def _first_row_diff(a, b):
    bad = np.flatnonzero((a != b).any(axis=1))
    i = int(bad[0])
    return "%d rows differ, first: row %d at byte %d" % (len(bad), i, int(np.flatnonzero(a[i] != b[i])[0]))


def _check_small(res, want, perm, what):
    for f in ("best", "score", "n_ops", "meta_r"):
        assert np.array_equal(res[f], want[f][perm]), (what, f)
    for f in ("loc", "off", "seq_id", "strand"):
        assert np.array_equal(res["meta"][f], want["meta"][f][perm]), (what, "meta." + f)


def _check_reads(buf, expect, perm, what):
    if perm is None:
        assert np.array_equal(buf, expect), (what, "reads", _first_row_diff(buf, expect))
    else:
        for i, p in enumerate(perm):
            assert np.array_equal(buf[i], expect[p]), (what, "reads", i)


def _check_rows(store, want, what):
    """Row layout: the store went in zeroed, so one comparison covers every used op byte and every byte behind it."""
    assert np.array_equal(store, want["ops"]), (what, "op rows", _first_row_diff(store, want["ops"]))


def _check_dense(res, store, world, perm, what, text):
    want = world["want"]
    n = len(res["n_ops"])
    idx = np.arange(n) if perm is None else perm
    off, flat = res["ops_off"], store.reshape(-1)
    starts = _units(res)
    assert len(starts) and starts[0] == 0
    texts = _texts(world) if text else None
    size = np.array([len(texts[p]) + 1 for p in idx]) if text else np.maximum(res["n_ops"], 0).astype(np.int64)
    used = size > 0
    # 16-byte aligned, ascending, inside the rows of the read's unit, no two reads overlapping
    ends = np.append(starts[1:], n)
    unit_of = np.searchsorted(starts, np.arange(n), side="right") - 1
    assert (off[used] % 16 == 0).all(), what
    assert (off[used] >= starts[unit_of[used]] * STORE_STRIDE).all() and (off[used] + size[used] <= ends[unit_of[used]] * STORE_STRIDE).all(), what
    assert (off[used][1:] >= off[used][:-1] + size[used][:-1]).all(), what
    for i in range(n):
        o, k = int(off[i]), int(size[i])
        expect = texts[idx[i]] + b"\0" if text else want["ops"][idx[i], :k].tobytes()
        if flat[o:o + k].tobytes() != expect:
            d = int(np.flatnonzero(np.frombuffer(expect, dtype=np.uint8) != flat[o:o + k])[0])
            raise AssertionError("%s: %s bytes differ from byte %d of %d; %s" % (what, "text" if text else "op", d, k, _where(o + d, i, starts)))
    return starts


def _image(res, lens, keep_reads, lo=0, hi=None, text_sizes=None):
    """Bytes of the dense image of reads [lo, hi) as collect() lays it out: the 16-aligned used part of every op row (or
    text), then the 16-aligned reads that were reverse-complemented -- from the RETURNED n_ops, meta and the lens."""
    hi = len(lens) if hi is None else hi
    k = np.clip(res["n_ops"][lo:hi], 0, STORE_STRIDE).astype(np.int64) if text_sizes is None else text_sizes[lo:hi]
    ops = int(((k + 15) & ~15).sum())
    rev = (res["meta_r"][lo:hi] != 0) & (res["meta"]["strand"][lo:hi] == 1)
    rd = 0 if keep_reads else int(((lens[lo:hi][rev].astype(np.int64) + 15) & ~15).sum())
    return ops, rd


def _pieces(nbytes):
    return (nbytes + RING_CHUNK - 1) // RING_CHUNK


def _report(what, **kw):
    print("boundary-scale %-40s %s" % (what, "  ".join("%s=%s" % kv for kv in kw.items())))


# ---- reference C: the oracle on a sample ------------------------------------------------------------------------------------

def _oracle_check(world, idx, what):
    """Reference A equals the CPU oracle on reads idx."""
    if world["oi"] is None:
        world["oi"] = orc.OracleIndex.from_host_index(world["hi"])
    idx = np.array(sorted(set(int(i) for i in idx) - set(world["oracle"])), dtype=np.int64)
    if not len(idx):
        return
    oi, want = world["oi"], world["want"]
    lens = world["lens"][idx]
    reads = np.ascontiguousarray(world["reads"][idx])
    best, _ = oi.seed_batch(reads, lens, nthreads=8)
    ext = oi.extend_batch(reads, lens, best, nthreads=8)
    assert np.array_equal(best, want["best"][idx]), what
    for f in ("score", "n_ops", "meta_r"):
        assert np.array_equal(ext[f], want[f][idx]), (what, f)
    for f in ("loc", "off", "seq_id", "strand"):
        assert np.array_equal(ext["meta"][f], want["meta"][f][idx]), (what, f)
    assert np.array_equal(reads, want["reads"][idx]), what
    for n, i in enumerate(idx):
        k = max(int(ext["n_ops"][n]), 0)
        assert bytes(ext["ops"][n, :k]) == bytes(want["ops"][i, :k]), (what, i)
        world["oracle"][int(i)] = True


def test_device_resident_reference_equals_the_oracle_on_a_sample(world):
    _oracle_check(world, range(0, N_READS, 1200), "every 1200th read")
    assert len(world["oracle"]) == len(range(0, N_READS, 1200))


# ---- the cases --------------------------------------------------------------------------------------------------------------

def _submit(world, handle, opts, pinned, k=0, perm=None):
    reads, store = world["bufs"].get(pinned, k)
    if perm is None:
        reads[:] = world["reads"]
    else:
        np.take(world["reads"], perm, axis=0, out=reads)
    store.fill(0)
    lens = world["lens"] if perm is None else world["lens"][perm]
    if opts is None:
        return None, reads, store, lens
    return mapper.map_batch_submit(handle, reads, lens, store=store, options=opts), reads, store, lens


def _run(world, handle, opts, pinned, what):
    """One batch through the host-buffer call in the layout opts ask for, compared in full; -> (result, unit starts)."""
    pend, reads, store, lens = _submit(world, handle, opts, pinned)
    res = mapper.map_batch(handle, reads, lens, store=store) if pend is None else pend.wait()     # None: lrm_map_batch itself
    opts = opts or {}
    want = world["want"]
    _check_small(res, want, slice(None), what)
    _check_reads(reads, world["reads"] if opts.get("keep_reads") else want["reads"], None, what)
    if opts.get("cigar_text") or opts.get("dense_results"):
        return res, _check_dense(res, store, world, None, what, bool(opts.get("cigar_text")))
    _check_rows(store, want, what)
    return res, None


@pytest.mark.parametrize("pinned", [False, True])
def test_rows_automatic_plan(world, pinned):
    """The default layout under the plan the library makes by itself (four seed sub-batches, two units): rows placed
    across ring pieces; pageable buffers go up through some twenty staging chunks of 32 MiB."""
    what = "rows, %s, automatic" % ("pinned" if pinned else "pageable")
    res, _ = _run(world, world["di"], {} if pinned else None, pinned, what)
    ops, rd = _image(res, world["lens"], False)
    assert world["reads"].nbytes > 19 * (32 << 20)
    _report(what, image_MB=(ops + rd) >> 20, pieces_over_all_units=_pieces(ops + rd))


def test_rows_one_unit_laps_the_ring_twice(world):
    what = "rows, pageable, sub_batches=1"
    res, _ = _run(world, world["di"], {"sub_batches": 1}, False, what)
    ops, rd = _image(res, world["lens"], False)
    assert _pieces(ops + rd) > 2 * N_RING + 1, "one unit of %d bytes does not lap the ring twice" % (ops + rd)
    _report(what, image_MB=(ops + rd) >> 20, pieces=_pieces(ops + rd), laps=(_pieces(ops + rd) - 1) // N_RING)


def _unit_report(what, res, starts, lens, keep_reads, text_sizes=None):
    ends = list(starts[1:]) + [len(lens)]
    sizes = [_image(res, lens, keep_reads, int(a), int(b), text_sizes) for a, b in zip(starts, ends)]
    _report(what, units=len(starts), ops_MB=[o >> 20 for o, _ in sizes], ring_pieces_of_reads=[_pieces(r) for _, r in sizes],
            pieces_of_ops=[_pieces(o) for o, _ in sizes])
    return sizes


def test_dense_pinned_automatic_plan(world):
    """Reverse-complemented reads through the ring, the op bytes of a unit by one DMA behind them into the pinned store."""
    what = "dense, pinned, automatic"
    res, starts = _run(world, world["di"], {"dense_results": 1}, True, what)
    sizes = _unit_report(what, res, starts, world["lens"], False)
    assert len(starts) == 2 and all(r > 4 * RING_CHUNK for _, r in sizes)


def test_dense_pageable_one_unit_through_the_flat_ring(world):
    """A pageable store: the op bytes of the one unit come down through the ring as they are (`flat`), more pieces than
    the ring has chunks.  The reads that straddle two pieces are checked against the oracle too."""
    what = "dense, pageable, sub_batches=1"
    res, starts = _run(world, world["di"], {"dense_results": 1, "sub_batches": 1}, False, what)
    assert len(starts) == 1
    (ops, rd), = _unit_report(what, res, starts, world["lens"], False)
    assert ops > (N_RING + 1) * RING_CHUNK, "op bytes of %d bytes do not lap the ring" % ops
    off, k = res["ops_off"], np.maximum(res["n_ops"], 0)
    straddle = np.flatnonzero((k > 0) & (off // RING_CHUNK != (off + k - 1) // RING_CHUNK))
    assert len(straddle) >= N_RING
    _oracle_check(world, straddle, "reads across two ring pieces")


def test_dense_keep_reads_pinned(world):
    """Nothing is placed by the host: op bytes by DMA, the reads stay as they were submitted."""
    what = "dense + keep_reads, pinned, automatic"
    res, starts = _run(world, world["di"], {"dense_results": 1, "keep_reads": 1}, True, what)
    _unit_report(what, res, starts, world["lens"], True)


@pytest.mark.parametrize("pinned", [True, False])
def test_text_automatic_plan(world, pinned):
    """Both passes of cigar_text_kernel on every read; the text lengths size the image."""
    what = "text, %s, automatic" % ("pinned" if pinned else "pageable")
    res, starts = _run(world, world["di"], {"cigar_text": 1}, pinned, what)
    _unit_report(what, res, starts, world["lens"], False, np.array([len(t) + 1 for t in _texts(world)]))


def test_text_keep_reads_six_units(world):
    """Six units on one slot: dense[g & 1] is written again while the transfer out of it two units ago is awaited."""
    what = "text + keep_reads, pinned, six units"
    res, starts = _run(world, world["di"], {"cigar_text": 1, "keep_reads": 1, "sub_batches": 6, "group_subs": 1}, True, what)
    assert len(starts) == 6
    _unit_report(what, res, starts, world["lens"], True, np.array([len(t) + 1 for t in _texts(world)]))


def test_three_dense_batches_in_flight(world):
    """X, Y (the same reads in another order, so every offset differs) and X again, submitted back to back with three
    pinned buffer sets and waited for in order: each equals the reference permuted the same way."""
    want = world["want"]
    perm = np.random.default_rng(9).permutation(N_READS)
    perms = [None, perm, None]
    pend = []
    try:
        sets = [_submit(world, world["di"], None, True, k, p) for k, p in enumerate(perms)]      # the buffers first ...
        for _, reads, store, lens in sets:                                                        # ... then back to back
            pend.append((mapper.map_batch_submit(world["di"], reads, lens, store=store, options={"dense_results": 1}), reads, store, lens))
        for k, (p, (pb, reads, store, lens)) in enumerate(zip(perms, pend)):
            what = "dense, pinned, in flight, batch %d" % k
            res = pb.wait()
            _check_small(res, want, slice(None) if p is None else p, what)
            _check_reads(reads, want["reads"], p, what)
            starts = _check_dense(res, store, world, p, what, False)
            _unit_report(what, res, starts, lens, False)
            assert k == 0 or len(starts) == 1, "batch %d was planned as if nothing else were in flight" % k
    finally:
        for pb, *_ in pend:
            if pb.ticket is not None:
                pb.wait()


def test_rows_on_a_group_handle(world, gpu):
    """Two replicas (the one device listed twice): the batch is cut by bases on ragged lengths, each share goes through
    its own context, rows land in the one caller buffer."""
    dg = index.DeviceIndex.upload_multi(world["hi"], [gpu, gpu])
    try:
        assert dg.replicas == 2
        what = "rows, pageable, group of two"
        res, _ = _run(world, dg, {}, False, what)
        ops, rd = _image(res, world["lens"], False)
        cum = np.cumsum(world["lens"].astype(np.int64))
        cut = int(np.searchsorted(cum, cum[-1] // 2))
        assert abs(cut - N_READS // 2) > 8, "the cut by bases should not be the cut by reads"
        _report(what, image_MB=(ops + rd) >> 20, pieces_over_all_units=_pieces(ops + rd), cut_near_read=cut)
    finally:
        dg.close()
