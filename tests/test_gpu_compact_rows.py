"""The split and the secondary stage past one workgroup, one scan tile and one gather chunk (csrc/compact_rows.h,
split_kernels.hip, secondary_kernels.hip), on the constructed inputs of tests/compact_cases.py:

  order   65 829 reads, 258 workgroups of the count / mark kernels, two tiles of the scan kernel: the carried sum, the
          workgroup prefix and the `before` term of every wavefront hold something other than 0; a wrong one moves every
          later record of the table
  gather  rows of 4080 .. 12 289 bytes, up to four chunks, at the tightest legal row stride (the next multiple of 16 above
          the longest row) and at a stride of exactly two chunks; every source phase mod 16; both strands of the mirrored
          gather of the secondary stage

Tables against tests/split_ref.py / tests/rival_ref.py, rows against slices of the reads, per-row outputs against the
existing calls over a batch made of the rows (split: map_batch; secondary: the unchanged extension call, and the 240-read
stage run tests/test_gpu_secondary.py pins against it), device entry points against host entry points."""
import time

import numpy as np
import pytest

import compact_cases as cc
import orc
import rival_ref
import split_ref
from longreadmapper_amd import capi, index, mapper
from test_gpu_mapq import SMALL
from test_gpu_secondary import _same_as_the_extension_call, _same_meta, _stage, planted  # noqa: F401  (planted: a fixture)
from test_gpu_split import _check_segments, _device_split, _rows_of, _table

pytestmark = pytest.mark.gpu
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
FILL = 0x77


@pytest.fixture(scope="module")
def small(gpu):
    ref = cc.small_reference()
    hi = index.HostIndex.build([ref], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    yield ref, hi, di
    di.close()


def _expected_rows(reads, read, start, length, width, turned, fill):
    """Rows of `width` bytes: [0, len) the slice reads[read, start : start + len] (reverse-complemented where turned),
    zeros up to the next multiple of 16, `fill` behind that."""
    read, start, length = (np.asarray(x, dtype=np.int64)[:, None] for x in (read, start, length))
    cols = np.arange(width, dtype=np.int64)[None, :]
    t = np.asarray(turned, dtype=bool)[:, None]
    src_col = np.clip(start + np.where(t, length - 1 - cols, cols), 0, reads.shape[1] - 1)
    src = reads[read, src_col]
    src = np.where(t, COMP[src], src)
    return np.where(cols < length, src, np.where(cols < cc.round16(length), 0, fill)).astype(np.uint8)


def _split_only(di, gpu, reads, lens, cl, cr, max_len, seg_cap, fill=None, **kw):
    """lrm_split_batch_dev over the caller's clip records, no primary pass -> (split results, the whole row buffer, the
    reads as the stage left them)"""
    import torch
    n = len(lens)
    dm = mapper.DeviceMapper(di, n, max_len, device=gpu, clip=True, split=True, split_min_len=cc.M, seg_cap=seg_cap, **kw)
    try:
        d_reads, d_lens = torch.from_numpy(reads).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
        dm.clip.copy_(torch.from_numpy(cc.clip_records(cl, cr).view(np.int32).reshape(n, 2)).cuda())
        if fill is not None:
            dm.seg["rows"].fill_(fill)
        k = dm.split(d_reads, d_lens)
        torch.cuda.synchronize()
        sp = dm.split_results()
        assert len(sp["seg"]) == k
        return sp, dm.seg["rows"].cpu().numpy(), d_reads.cpu().numpy(), dm.seg_row_stride
    finally:
        dm.close()


def _turned(res):
    return (res["meta_r"] != 0) & (res["meta"]["strand"] == 1)


def _check_split(di, sp, all_rows, reads, lens, cl, cr, fill):
    """The table against split_ref.plan, the rows against the slices, every per-segment output against map_batch over the rows."""
    table = split_ref.plan(lens, cl, cr, cc.M)
    k = len(table)
    assert _table(sp["seg"]) == table
    t = np.array(table, dtype=np.int64)
    assert np.array_equal(sp["lens"], t[:, 2])
    want_rows = _expected_rows(reads, t[:, 0], t[:, 1], t[:, 2], all_rows.shape[1], _turned(sp), fill)
    bad = np.flatnonzero((all_rows[:k] != want_rows).any(axis=1))
    assert bad.size == 0, (bad[:8].tolist(), [table[s] for s in bad[:8]])
    assert (all_rows[k:] == fill).all()
    rows, seg_lens = _rows_of(reads, lens, table)
    after = rows.copy()
    want = mapper.map_batch(di, after, seg_lens, clip=True)
    _check_segments(sp, want, after, table)
    return table


def test_split_order_at_scale(small, gpu):
    """258 workgroups, two scan tiles, two-segment reads in the last lane of a workgroup, of a tile and of the batch."""
    ref, hi, di = small
    di.set_map_options()
    c = cc.split_order_case()
    reads, lens, cl, cr = c["reads"], c["lens"], c["cl"], c["cr"]
    n_want = len(split_ref.plan(lens, cl, cr, cc.M))
    sp, all_rows, reads_after, stride = _split_only(di, gpu, reads, lens, cl, cr, 400, n_want + 8, fill=0, seg_rows=512)
    assert stride == 416 and np.array_equal(reads_after, reads)
    table = _check_split(di, sp, all_rows, reads, lens, cl, cr, 0)
    aligned = int(((sp["seg"]["flags"] & split_ref.SEG_ALIGNED) != 0).sum())
    print("split order: %d reads, %d segments, %d aligned, %d turned round" % (len(lens), len(table), aligned, int(_turned(sp).sum())))
    assert len(table) == n_want == 12_603


def test_split_long_segments_at_the_tight_stride(small, gpu):
    """Segments of up to four chunks, the longest one byte short of filling its row of 12 304; nothing is written outside
    a segment's own 16-byte units."""
    ref, hi, di = small
    di.set_map_options()
    g = cc.split_gather_case()
    reads, lens, cl, cr = g["reads"], g["lens"], g["cl"], g["cr"]
    n_want = len(split_ref.plan(lens, cl, cr, cc.M))
    sp, all_rows, reads_after, stride = _split_only(di, gpu, reads, lens, cl, cr, cc.MAX_LEN, n_want + 3, fill=FILL)
    assert stride == 12_304 and np.array_equal(reads_after, reads) and all_rows.shape == (n_want + 3, stride)
    table = _check_split(di, sp, all_rows, reads, lens, cl, cr, FILL)
    seg_len = np.array([t[2] for t in table])
    print("split gather: %d segments, %d longer than a chunk, longest %d, %d turned round" %
          (len(table), (seg_len > cc.SP_CHUNK).sum(), seg_len.max(), int(_turned(sp).sum())))
    assert seg_len.max() == cc.MAX_LEN and (seg_len > cc.SP_CHUNK).sum() >= 16 + 2 * 10


def test_split_long_segments_host_entry_point_equals_device(small, gpu):
    """Genuine reads between junk heads and tails of more than 4096 bases: primary pass and split stage on device buffers
    against lrm_split_batch over one map_batch(clip=True) call, whose rows a host loop gathers."""
    ref, hi, di = small
    di.set_map_options()
    reads, lens = cc.long_chimeras(ref)
    dev, oriented = _device_split(di, gpu, reads, lens)
    table = _table(dev["split"]["seg"], mask=~np.uint32(0))
    seg_len = np.array([t[2] for t in table])
    print("long chimeras: %d reads, %d segments, %d longer than a chunk (%s)" %
          (len(lens), len(table), (seg_len > cc.SP_CHUNK).sum(), sorted(seg_len.tolist())))
    assert (seg_len > cc.SP_CHUNK).sum() >= 1
    assert _table(dev["split"]["seg"]) == split_ref.plan(lens, dev["clip"]["left"], dev["clip"]["right"])
    buf = reads.copy()
    res = mapper.map_batch(di, buf, lens, clip=True)
    assert np.array_equal(buf, oriented)
    sp = mapper.split_batch(di, buf, lens, res)
    k = len(table)
    assert _table(sp["seg"], mask=~np.uint32(0)) == table
    assert np.array_equal(sp["rows"][:k], dev["split"]["rows"]) and np.array_equal(sp["lens"], dev["split"]["lens"])
    for key in ("best", "n_ops", "score", "meta_r", "clip"):
        assert sp[key].tobytes() == dev["split"][key].tobytes(), key
    for key in ("text_pos", "read_pos", "len", "delta", "left_ops", "flags"):
        assert np.array_equal(sp["anchor"][key], dev["split"]["anchor"][key]), key
    assert _same_meta(sp["meta"], dev["split"]["meta"])
    for s in range(k):
        assert mapper.ops_of(sp, s) == mapper.ops_of(dev["split"], s), s
    # the rows before their own extension are slices of the oriented reads
    t = np.array(table, dtype=np.int64)
    want_rows = _expected_rows(oriented, t[:, 0], t[:, 1], t[:, 2], sp["rows"].shape[1], _turned(sp), 0)
    assert np.array_equal(sp["rows"][:k], want_rows)


# ---------------------------------------------------------------------------------------------------------
# secondary
# ---------------------------------------------------------------------------------------------------------
def test_secondary_order_at_scale(planted, gpu):
    """The 240 planted reads tiled into 65 829 by the order pattern: every record of the big table against the oracle's
    entries, every per-candidate output against the same read's in the 240-read stage run."""
    r, di, want = planted["r"], planted["di"], planted["want"]
    pool_reads, pool_lens = r["reads"], r["lens"].astype(np.uint32)
    pool_prim, _, _, _, pool, _, _ = _stage(di, gpu, pool_reads, pool_lens, "clipped")
    is_cand = want[:, 1] > 0
    cand, none = np.flatnonzero(is_cand), np.flatnonzero(~is_cand)
    assert np.array_equal(pool["table"]["read"], cand) and len(cand) >= 40
    at_pool = np.full(len(pool_lens), -1, dtype=np.int64)
    at_pool[cand] = np.arange(len(cand))

    p = cc.order_pattern()
    n = len(p)
    rng = np.random.default_rng(20_264)
    tile = np.where(p, rng.choice(cand, n), rng.choice(none, n))
    assert len(set(tile[p].tolist())) == len(cand) and len(set(tile[~p].tolist())) == len(none)
    reads, lens = pool_reads[tile], pool_lens[tile]
    k_want = int(p.sum())
    t0 = time.perf_counter()
    before, after, reads_before, reads_after, out, b0, b1 = _stage(di, gpu, reads, lens, "clipped", sec_cap=k_want + 8)
    print("secondary order: %d reads, %d candidates, stage run %.2f s" % (n, len(out["table"]), time.perf_counter() - t0))
    assert np.array_equal(reads_before, reads_after)
    assert b1 - b0 == 24 * n + 8 * ((n + 255) // 256) + 8                 # the stage's scratch at this n

    # the table
    tb = out["table"]
    assert len(tb) == k_want and np.array_equal(tb["read"], np.flatnonzero(p)) and not tb["_pad"].any()
    src = tile[p]                                                           # the pool read of candidate s
    c = at_pool[src]                                                        # ... and its place in the pool's table
    assert (c >= 0).all()
    assert np.array_equal(tb["hits"], want[src, 1]) and np.array_equal(out["lens"], pool_lens[src])
    for f, col in (("key", 0), ("val", 1), ("bucket", 2)):
        assert np.array_equal(out["rival"][f], want[src, col]), f
    # every per-candidate output, byte for byte
    assert np.array_equal(out["rows"], pool["rows"][c])
    for key in ("n_ops", "score", "meta_r"):
        assert np.array_equal(out[key], pool[key][c]), key
    assert _same_meta(out["meta"], pool["meta"][c])
    used = np.arange(out["ops"].shape[1])[None, :] < out["n_ops"][:, None]
    assert not ((out["ops"] != pool["ops"][c]) & used).any()
    for key in ("anchor", "clip"):
        assert out[key].tobytes() == pool[key][c].tobytes(), key
    assert np.array_equal(tb["flags"], pool["table"]["flags"][c])
    assert ((tb["flags"] & capi.SEC_ALIGNED) != 0).sum() >= 0.7 * k_want

    # the primary results: the pool's at the tiled index, before the stage and after it
    for res in (before, after):
        for key in ("best", "mapq", "anchor", "clip"):
            assert res[key].tobytes() == pool_prim[key][tile].tobytes(), key
        for key in ("n_ops", "score", "meta_r"):
            assert np.array_equal(res[key], pool_prim[key][tile]), key
        assert _same_meta(res["meta"], pool_prim["meta"][tile])
    for q in range(len(pool_lens)):
        m = max(int(pool_prim["n_ops"][q]), 0)
        assert (after["ops"][tile == q, :m] == pool_prim["ops"][q, :m]).all(), q


@pytest.fixture(scope="module")
def long_sec(gpu):
    c = cc.secondary_gather_case()
    hi = index.HostIndex.build([c["base"]], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    oi = orc.OracleIndex.from_host_index(hi)
    want = rival_ref.batch(oi, c["reads"], c["lens"])
    yield dict(c, di=di, want=want)
    di.close()


def _long_batch(long_sec, width):
    sel = np.flatnonzero(long_sec["lens"] <= width)
    reads = np.ascontiguousarray(long_sec["reads"][sel, :width + 1])
    return reads, long_sec["lens"][sel].astype(np.uint32), long_sec["want"][sel]


@pytest.mark.parametrize("width", [12_289, 8191], ids=["stride-12304", "stride-two-chunks"])
@pytest.mark.parametrize("mode", ["classic", "clipped"])
def test_secondary_long_candidates(long_sec, gpu, mode, width):
    """Candidates of up to four chunks on both strands: at 12 304 the last chunk has one live lane, at 8192 the guard on the
    row stride never stops a lane and the mirrored source of a reverse-strand read starts in the last chunk."""
    di = long_sec["di"]
    reads, lens, want = _long_batch(long_sec, width)
    n = len(lens)
    prim, _, oriented, _, out, _, _ = _stage(di, gpu, reads, lens, mode)
    row_stride = out["rows"].shape[1]
    assert row_stride == int(cc.round16(width + 1)) == (12_304 if width == 12_289 else 2 * cc.SP_CHUNK)
    assert (want[:, 1] > 0).all() and np.array_equal(out["table"]["read"], np.arange(n)) and not out["table"]["_pad"].any()
    assert np.array_equal(out["table"]["hits"], want[:, 1]) and np.array_equal(out["lens"], lens)
    for f, col in (("key", 0), ("val", 1), ("bucket", 2)):
        assert np.array_equal(out["rival"][f], want[:, col]), f
    mirrored = _turned(prim)
    per_len = {int(g): (int(mirrored[lens == g].sum()), int((~mirrored[lens == g]).sum())) for g in sorted(set(lens.tolist()))}
    print("secondary gather %s, row stride %d: (mirrored, not mirrored) candidates per length %s" % (mode, row_stride, per_len))
    assert set(per_len) == {g for g in cc.gather_lengths if g <= width} and all(a >= 1 and b >= 1 for a, b in per_len.values())
    assert not np.array_equal(oriented[mirrored], reads[mirrored])
    # rows: the read as sequenced (turned round by the candidate's own extension where that resolved to the reverse strand),
    # zeros from its end to the end of the row
    want_rows = _expected_rows(reads, np.arange(n), np.zeros(n), lens, row_stride, _turned(out), 0)
    bad = np.flatnonzero((out["rows"] != want_rows).any(axis=1))
    assert bad.size == 0, (bad.tolist(), lens[bad].tolist(), mirrored[bad].tolist())
    _same_as_the_extension_call(di, gpu, mode, reads, lens, np.arange(n), want, out)
    assert ((out["table"]["flags"] & capi.SEC_ALIGNED) != 0).sum() >= 0.7 * n


@pytest.mark.parametrize("width", [12_289, 8191], ids=["stride-12304", "stride-two-chunks"])
def test_secondary_long_candidates_host_buffers(long_sec, gpu, width):
    """mapper.secondary_batch over map_batch(mapq=True) of the long reads against the device stage, reads turned round
    in place and kept as sequenced."""
    di = long_sec["di"]
    reads, lens, want = _long_batch(long_sec, width)
    prim, _, oriented, _, out, _, _ = _stage(di, gpu, reads, lens, "clipped")
    k = len(out["table"])
    assert k == len(lens)
    for opts in ({}, {"keep_reads": 1}):
        rm = reads.copy()
        res = mapper.map_batch(di, rm, lens, options=dict(opts), clip=True, mapq=True)
        assert np.array_equal(rm, reads if opts else oriented)
        sec = mapper.secondary_batch(di, rm, lens, res, options=dict(opts), clip=True)
        assert len(sec["table"]) == k and sec["rows"].shape[1] == out["rows"].shape[1]
        for name in ("table", "rival", "anchor", "clip"):
            assert sec[name].tobytes() == out[name].tobytes(), (opts, name)
        for name in ("lens", "n_ops", "score", "meta_r"):
            assert np.array_equal(sec[name], out[name]), (opts, name)
        assert _same_meta(sec["meta"], out["meta"])
        assert np.array_equal(sec["rows"][:k], out["rows"]), opts
        for s in range(k):
            assert mapper.ops_of(sec, s) == bytes(out["ops"][s, :int(out["n_ops"][s])]), (opts, s)
