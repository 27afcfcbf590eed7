"""Batch entry points of the hot path, host-buffer and device-buffer flavours.

`seed_batch` / `extend_batch` are PART 1 / PART 2 of single_end() (alnmain.c:333-451) for a
whole batch; names, argument meaning and data conventions follow the reference (best[],
cig[], limit[], meta_r[], m[])."""
import ctypes as C

import numpy as np

from . import capi
from .capi import check, lib

ENTRY_DT = np.dtype([("key", "<u8"), ("val", "<u8"), ("bucket", "<u8")])
META_DT = np.dtype([("loc", "<u8"), ("off", "<u8"), ("seq_id", "<i4"), ("strand", "u1"), ("_pad", "V3")])
assert ENTRY_DT.itemsize == 24 and META_DT.itemsize == 24

DEFAULT_SEED_LEN = 20      # alnmain.c:577-580
DEFAULT_THRES = 300
DEFAULT_GACT = (320, 120, 128)
N_KERNELS = 9              # LRM_N_KERNELS in include/lrm_accel.h
ANCHOR_DT = np.dtype([("text_pos", "<u8"), ("read_pos", "<u4"), ("len", "<u4"), ("delta", "<i4"), ("left_ops", "<u4"),
                      ("flags", "<u4"), ("_pad", "V4")])      # lrm_anchor
assert ANCHOR_DT.itemsize == 32
CLIP_DT = np.dtype([("left", "<u4"), ("right", "<u4")])          # lrm_clip
SEGMENT_DT = np.dtype([("read", "<u4"), ("start", "<u4"), ("len", "<u4"), ("flags", "<u4")])      # lrm_segment
SEG_RIGHT, SEG_ALIGNED = capi.SEG_RIGHT, capi.SEG_ALIGNED
MAPQ_DT = np.dtype([("n1", "<u4"), ("n2", "<u4"), ("radius", "<u4"), ("mapq", "u1"), ("phase", "u1"), ("flags", "u1"),
                    ("_pad", "u1")])                              # lrm_mapq (docs/GACT_SPEC.md, "Mapping quality")
assert MAPQ_DT.itemsize == 16
MAPQ_OVERFLOW = capi.MAPQ_OVERFLOW
SUMMARY_DT = np.dtype([("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("ins_runs", "<u4"), ("del_runs", "<u4"),
                       ("clip_left", "<u4"), ("clip_right", "<u4")])      # lrm_aln_summary (docs/GACT_SPEC.md, "Alignment summary and PAF")
assert SUMMARY_DT.itemsize == 32


def aln_summary_host(ops):
    """lrm_aln_summary_host: the alignment summary record of one alignment's op bytes -> dict of the lrm_aln_summary fields."""
    data = bytes(ops)
    a = capi.AlnSummary()
    lib.lrm_aln_summary_host(data, len(data), C.byref(a))
    return {f: int(getattr(a, f)) for f, _ in a._fields_}


def anchored_store_stride(max_len):
    """Op bytes per read the anchored mode needs: both jobs' targets are an eighth longer than their queries."""
    return 2 * max_len + max_len // 8 + 2


def _anchor_options(options, anchored, anchor_min_len, clip=False, clip_penalty=0, clip_end_bonus=0):
    """clip (docs/GACT_SPEC.md, "End clipping": each job of an anchored read keeps its best-scoring prefix, '=' +1, any
    other column -clip_penalty (0 = 2), when that gains more than clip_end_bonus (0 = 6); the rest becomes 'S') implies
    anchored."""
    if not anchored and not clip:
        return options
    extra = {"anchored": 1, "anchor_min_len": anchor_min_len}
    if clip:
        extra.update(clip=1, clip_penalty=clip_penalty, clip_end_bonus=clip_end_bonus)
    return {**(options or {}), **extra}


def debug_anchor(index, read, loc, min_len=0):
    """lrm_debug_anchor: the anchor of one forward-oriented read at one voted locus -> dict of the lrm_anchor fields."""
    read = np.ascontiguousarray(read, dtype=np.uint8)
    a = capi.Anchor()
    check(lib.lrm_debug_anchor(index.handle, read.ctypes.data, len(read), loc, min_len, C.byref(a)), "lrm_debug_anchor")
    return {f: int(getattr(a, f)) for f, _ in a._fields_}


def debug_gact_jobs(reads, lens, text, toffs, tlens, gact=DEFAULT_GACT, gact_impl=0, bs_waves=0, counting=False, meta_r=None,
                    store_stride=None, fill=0, device=0):
    """lrm_debug_gact_jobs (tests only): read row k against text[toffs[k] : toffs[k] + tlens[k]] as one job table through the
    extension's plan and launch.  -> dict(ops=(n, store_stride) uint8, rows preset to `fill`; n_ops, score (preset to the
    same byte); counters: gact_tiles and capi.BS_COUNTERS of the launch)."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    text = np.ascontiguousarray(np.frombuffer(bytes(text), dtype=np.uint8))
    toffs = np.ascontiguousarray(toffs, dtype=np.uint64)
    tlens = np.ascontiguousarray(tlens, dtype=np.uint32)
    n, stride = reads.shape
    assert len(lens) == len(toffs) == len(tlens) == n
    if store_stride is None:
        store_stride = (int((lens.astype(np.int64) + tlens).max()) + 3) & ~3
    ops = np.full((n, store_stride), fill, dtype=np.uint8)
    n_ops = np.full(n, fill * 0x01010101, dtype=np.uint32).view(np.int32)
    score = n_ops.copy()
    counters = np.zeros(1 + len(capi.BS_COUNTERS), dtype=np.uint64)
    if meta_r is not None:
        meta_r = np.ascontiguousarray(meta_r, dtype=np.int32)
        assert len(meta_r) == n
    t = capi.GactTable(n, reads.ctypes.data, stride, lens.ctypes.data, text.ctypes.data, len(text), toffs.ctypes.data,
                       tlens.ctypes.data, None if meta_r is None else meta_r.ctypes.data, ops.ctypes.data, store_stride,
                       n_ops.ctypes.data, score.ctypes.data, counters.ctypes.data)
    check(lib.lrm_debug_gact_jobs(C.byref(t), capi.GactParams(*gact), gact_impl, bs_waves, int(bool(counting)), device),
          "lrm_debug_gact_jobs")
    return dict(ops=ops, n_ops=n_ops, score=score,
                counters=dict(zip(("gact_tiles",) + capi.BS_COUNTERS, (int(x) for x in counters))))


def seed_batch(index, reads, lens, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES):
    """Host buffers in, best[] out (numpy structured array key/val/bucket)."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n, stride = reads.shape
    best = np.zeros(n, dtype=ENTRY_DT)
    p = capi.Params(n, seed_len, thres)
    check(lib.lrm_seed_batch(index.handle, reads.ctypes.data, stride, lens.ctypes.data, n, p, best.ctypes.data),
          "lrm_seed_batch")
    return best


def extend_batch(index, reads, lens, best, gact=DEFAULT_GACT, anchored=False, anchor_min_len=0, clip=False, clip_penalty=0,
                 clip_end_bonus=0):
    """Host buffers; `reads` is modified in place (reverse-strand reads are rev-comped).
    anchored: the anchored extension mode (lrm_map_options.anchored) for this call, on top of the handle's options.
    clip: its end clipping (lrm_map_options.clip; implies anchored): the read ends that do not align come out as 'S'
    columns; clip_penalty / clip_end_bonus: P and B of the rule, 0 = the defaults 2 and 6.

    Returns dict(ops=(n, store_stride) uint8, n_ops, score, meta, meta_r)."""
    extra = _anchor_options(None, anchored, anchor_min_len, clip, clip_penalty, clip_end_bonus)
    if extra:
        with index.map_options_plus(**extra):
            return _extend_batch(index, reads, lens, best, gact, True)
    return _extend_batch(index, reads, lens, best, gact, False)


def _extend_batch(index, reads, lens, best, gact, anchored):
    assert reads.dtype == np.uint8 and reads.flags.c_contiguous and reads.flags.writeable
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    best = np.ascontiguousarray(best, dtype=ENTRY_DT)
    n, stride = reads.shape
    max_len = int(lens.max()) if n else 0
    store_stride = anchored_store_stride(max_len) if anchored else max(2 * max_len, 1)     # alnmain.c:316-320
    store = np.zeros((n, store_stride), dtype=np.uint8)
    cig = (capi.Cigar * max(n, 1))()
    score = np.zeros(n, dtype=np.int32)
    meta = np.zeros(n, dtype=META_DT)
    meta_r = np.zeros(n, dtype=np.int32)
    gp = capi.GactParams(*gact)
    check(lib.lrm_extend_batch(index.handle, reads.ctypes.data, stride, lens.ctypes.data, n, best.ctypes.data, gp,
                               C.cast(cig, C.c_void_p), store.ctypes.data, store_stride, score.ctypes.data,
                               meta.ctypes.data, meta_r.ctypes.data), "lrm_extend_batch")
    n_ops = np.ctypeslib.as_array(C.cast(cig, C.POINTER(C.c_int32)), shape=(max(n, 1), 4))[:n, 2].copy()
    return dict(ops=store, n_ops=n_ops, score=score, meta=meta, meta_r=meta_r)


def pinned_empty(shape, dtype=np.uint8):
    """numpy array in pinned host memory (lrm_host_alloc): the DMA engines read / write it directly.
    Free with pinned_free(arr)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = lib.lrm_host_alloc(max(n, 1))
    if not p:
        raise capi.LrmError("lrm_host_alloc: " + lib.lrm_last_error().decode(errors="replace"))
    buf = (C.c_char * max(n, 1)).from_address(p)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    return arr


def pinned_free(arr):
    lib.lrm_host_free(arr.ctypes.data)


class PendingBatch:
    """A batch submitted with map_batch_submit: wait() blocks until its results are in the caller's arrays."""

    def __init__(self, ticket, keep, n, dense, text=False, extras=None):
        self.ticket, self._keep, self.n, self.dense, self.text = ticket, keep, n, dense, text
        self._extras = extras or {}          # "mapq" / "summary": the record arrays the batch fills on top

    def wait(self):
        t, self.ticket = self.ticket, None
        assert t is not None, "already waited for"
        check(lib.lrm_map_batch_wait(t), "lrm_map_batch_wait")
        best, store, cig, score, meta, meta_r = self._keep[:6]
        n = self.n
        cv = np.ctypeslib.as_array(C.cast(cig, C.POINTER(C.c_int32)), shape=(max(n, 1), 4))[:n]
        out = dict(best=best, ops=store, n_ops=cv[:, 2].copy(), score=score, meta=meta, meta_r=meta_r)
        out.update(self._extras)
        if self.dense:          # cig[i].cigar = store_mem + off[i]
            ptr = np.ctypeslib.as_array(C.cast(cig, C.POINTER(C.c_uint64)), shape=(max(n, 1), 2))[:n, 0]
            out["ops_off"] = (ptr - np.uint64(store.ctypes.data)).astype(np.int64)
        out["is_text"] = self.text   # cig[i].cigar -> NUL-terminated run-length CIGAR text: text_of(res, i)
        return out


def text_of(res, i):
    """Run-length CIGAR text of read i from a map_batch result in the cigar_text layout."""
    assert res.get("is_text")
    flat = res["ops"].reshape(-1)
    o = int(res["ops_off"][i])
    chunk = 64
    while True:
        b = bytes(flat[o:o + chunk])
        z = b.find(b"\0")
        if z >= 0:
            return b[:z]
        chunk *= 4


def ops_of(res, i):
    """Op bytes of read i from a map_batch result in either layout."""
    k = int(res["n_ops"][i])
    if "ops_off" in res:
        o = int(res["ops_off"][i])
        return bytes(res["ops"].reshape(-1)[o:o + k])
    return bytes(res["ops"][i, :k])


def map_batch_submit(index, reads, lens, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES, gact=DEFAULT_GACT, store=None,
                     options=None, anchored=False, anchor_min_len=0, clip=False, clip_penalty=0, clip_end_bonus=0, mapq=False,
                     summary=False):
    """lrm_map_batch_submit_ex (mapq=True: the result gains "mapq", the MAPQ_DT records of the batch; summary=True: it gains
    "summary", the SUMMARY_DT records; neither: lrm_map_batch_submit): queues the batch and returns a PendingBatch.  `reads` is modified in place like
    extend_batch once the batch runs; `store` may be a caller-provided (n, >= 2*max_len) uint8 array (e.g. pinned;
    anchored: >= anchored_store_stride(max_len)); `options`: dict of lrm_map_options fields (None: the handle's
    defaults); anchored=True adds the anchored extension mode to them, clip=True that mode with its end clipping
    (see extend_batch)."""
    assert reads.dtype == np.uint8 and reads.flags.c_contiguous and reads.flags.writeable
    options = _anchor_options(options, anchored, anchor_min_len, clip, clip_penalty, clip_end_bonus)
    anchored = bool(options and options.get("anchored"))
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n, stride = reads.shape
    max_len = int(lens.max()) if n else 0
    if store is None:
        need = anchored_store_stride(max_len) if anchored else 2 * max_len
        store = np.zeros((n, max((need + 15) // 16 * 16, 16)), dtype=np.uint8)
    store_stride = store.shape[1]
    best = np.zeros(n, dtype=ENTRY_DT)
    cig = (capi.Cigar * max(n, 1))()
    score = np.zeros(n, dtype=np.int32)
    meta = np.zeros(n, dtype=META_DT)
    meta_r = np.zeros(n, dtype=np.int32)
    opt = capi.map_options(**options) if options is not None else None
    ticket = C.c_void_p()
    extras = {}
    if mapq:
        extras["mapq"] = np.zeros(n, dtype=MAPQ_DT)
    if summary:
        extras["summary"] = np.zeros(n, dtype=SUMMARY_DT)
    ex = capi.BatchExtras(C.sizeof(capi.BatchExtras), 0, extras["mapq"].ctypes.data if mapq else None,
                          extras["summary"].ctypes.data if summary else None)
    check(lib.lrm_map_batch_submit_ex(index.handle, reads.ctypes.data, stride, lens.ctypes.data, n,
                                      capi.Params(n, seed_len, thres), capi.GactParams(*gact), best.ctypes.data,
                                      C.cast(cig, C.c_void_p), store.ctypes.data, store_stride, score.ctypes.data,
                                      meta.ctypes.data, meta_r.ctypes.data, C.byref(opt) if opt is not None else None,
                                      C.byref(ex) if extras else None, C.byref(ticket)), "lrm_map_batch_submit_ex")
    text = bool(opt.cigar_text) if opt is not None else False
    dense = (bool(opt.dense_results) or text) if opt is not None else False
    keep = (best, store, cig, score, meta, meta_r, reads, lens)
    return PendingBatch(ticket, keep, n, dense, text, extras)


def map_batch(index, reads, lens, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES, gact=DEFAULT_GACT, store=None,
              options=None, anchored=False, anchor_min_len=0, clip=False, clip_penalty=0, clip_end_bonus=0, mapq=False, summary=False):
    """PART 1 + PART 2 in one device pass; `reads` is modified in place like extend_batch.
    Without `options` this is lrm_map_batch (the handle's default options), with them (or with anchored=True or
    clip=True, which are among them) submit + wait.  mapq=True: the mapping-quality records (MAPQ_DT) come back as
    res["mapq"] next to the other results, which do not change; summary=True: the alignment summary records (SUMMARY_DT) as
    res["summary"], likewise (submit + wait through lrm_map_batch_submit_ex)."""
    options = _anchor_options(options, anchored, anchor_min_len, clip, clip_penalty, clip_end_bonus)
    if options is not None or mapq or summary:
        return map_batch_submit(index, reads, lens, seed_len, thres, gact, store, options, mapq=mapq, summary=summary).wait()
    assert reads.dtype == np.uint8 and reads.flags.c_contiguous and reads.flags.writeable
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n, stride = reads.shape
    max_len = int(lens.max()) if n else 0
    if store is None:
        store = np.zeros((n, max(2 * max_len, 1)), dtype=np.uint8)
    store_stride = store.shape[1]
    best = np.zeros(n, dtype=ENTRY_DT)
    cig = (capi.Cigar * max(n, 1))()
    score = np.zeros(n, dtype=np.int32)
    meta = np.zeros(n, dtype=META_DT)
    meta_r = np.zeros(n, dtype=np.int32)
    check(lib.lrm_map_batch(index.handle, reads.ctypes.data, stride, lens.ctypes.data, n,
                            capi.Params(n, seed_len, thres), capi.GactParams(*gact), best.ctypes.data,
                            C.cast(cig, C.c_void_p), store.ctypes.data, store_stride, score.ctypes.data,
                            meta.ctypes.data, meta_r.ctypes.data), "lrm_map_batch")
    n_ops = np.ctypeslib.as_array(C.cast(cig, C.POINTER(C.c_int32)), shape=(max(n, 1), 4))[:n, 2].copy()
    return dict(best=best, ops=store, n_ops=n_ops, score=score, meta=meta, meta_r=meta_r)


def split_plan(lens, clip, split_min_len=0, cap=None):
    """lrm_split_plan: the segment table (SEGMENT_DT) of a batch from its read lengths and lrm_clip records; pure host.
    cap=None: room for every segment; otherwise -> (rc, n_seg, table) without raising on rc == -3."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    clip = np.ascontiguousarray(clip, dtype=CLIP_DT)
    n = len(lens)
    room = 2 * n if cap is None else cap
    seg = np.zeros(max(room, 1), dtype=SEGMENT_DT)
    k = C.c_uint64()
    rc = lib.lrm_split_plan(lens.ctypes.data, clip.ctypes.data, n, split_min_len, seg.ctypes.data if room else None, room,
                            C.byref(k))
    if cap is None:
        check(rc, "lrm_split_plan")
        return seg[:k.value].copy()
    return rc, int(k.value), seg[:min(k.value, room)].copy()


def clip_of_cigar(ops_or_text, is_text=False):
    """lrm_clip_of_cigar of one alignment: op bytes, or (is_text) its run-length text -> (left, right)."""
    data = bytes(ops_or_text)
    buf = C.create_string_buffer(data, len(data) + 1)
    n_ops = len(data) if not is_text else (0 if data == b"*" else 1)
    cg = capi.Cigar(C.cast(buf, capi.u8p), n_ops, 0)
    left, right = C.c_uint32(), C.c_uint32()
    check(lib.lrm_clip_of_cigar(C.byref(cg), int(is_text), C.byref(left), C.byref(right)), "lrm_clip_of_cigar")
    return int(left.value), int(right.value)


class SplitBuffers:
    """Host arrays of an lrm_split_out for up to cap segments of up to max_seg bases."""

    def __init__(self, cap, max_seg):
        self.cap = cap
        self.row_stride = (max_seg + 16) // 16 * 16
        self.store_stride = (anchored_store_stride(max_seg) + 15) // 16 * 16
        k = max(cap, 1)
        self.seg = np.zeros(k, dtype=SEGMENT_DT)
        self.rows = np.zeros((k, self.row_stride), dtype=np.uint8)
        self.lens = np.zeros(k, dtype=np.uint32)
        self.best = np.zeros(k, dtype=ENTRY_DT)
        self.cig = (capi.Cigar * k)()
        self.store = np.zeros((k, self.store_stride), dtype=np.uint8)
        self.score = np.zeros(k, dtype=np.int32)
        self.meta = np.zeros(k, dtype=META_DT)
        self.meta_r = np.zeros(k, dtype=np.int32)
        self.anchor = np.zeros(k, dtype=ANCHOR_DT)
        self.clip = np.zeros(k, dtype=CLIP_DT)
        self.out = capi.SplitOut(cap, 0, self.seg.ctypes.data, self.rows.ctypes.data, self.row_stride, self.lens.ctypes.data,
                                 self.best.ctypes.data, C.cast(self.cig, C.c_void_p), self.store.ctypes.data, self.store_stride,
                                 self.score.ctypes.data, self.meta.ctypes.data, self.meta_r.ctypes.data, self.anchor.ctypes.data,
                                 self.clip.ctypes.data)

    def result(self, dense, text):
        k = int(self.out.n_seg)
        cv = np.ctypeslib.as_array(C.cast(self.cig, C.POINTER(C.c_int32)), shape=(max(self.cap, 1), 4))[:k]
        res = dict(seg=self.seg[:k], rows=self.rows[:k], lens=self.lens[:k], best=self.best[:k], ops=self.store, n_ops=cv[:, 2].copy(),
                   score=self.score[:k], meta=self.meta[:k], meta_r=self.meta_r[:k], anchor=self.anchor[:k], clip=self.clip[:k],
                   is_text=text, buffers=self)
        if dense:
            ptr = np.ctypeslib.as_array(C.cast(self.cig, C.POINTER(C.c_uint64)), shape=(max(self.cap, 1), 2))[:k, 0]
            res["ops_off"] = (ptr - np.uint64(self.store.ctypes.data)).astype(np.int64)
        return res


def _cigars_of(res, n):
    """lrm_cigar array that points into a map_batch result, as the C caller would still hold it."""
    cig = (capi.Cigar * max(n, 1))()
    base = res["ops"].ctypes.data
    stride = res["ops"].shape[1] if res["ops"].ndim == 2 else 0
    for i in range(n):
        off = int(res["ops_off"][i]) if "ops_off" in res else i * stride
        cig[i].cigar = C.cast(C.c_void_p(base + off), capi.u8p)
        cig[i].n_cigar_op = int(res["n_ops"][i])
        cig[i].score = int(res["score"][i])
    return cig


def split_batch(index, reads, lens, res, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES, gact=DEFAULT_GACT, options=None,
                anchor_min_len=0, clip_penalty=0, clip_end_bonus=0, split_min_len=0, cap=None, buffers=None):
    """lrm_split_batch: the second pass over `res`, what map_batch(index, reads, lens, clip=True, ...) returned for `reads`
    (as that call left them), with the same options.  -> dict(seg=SEGMENT_DT table, rows, lens, best, ops, n_ops, score, meta,
    meta_r, anchor, clip [, ops_off]); ops_of / text_of read a segment's alignment like a read's.  cap: room for that many
    segments (None: for every possible one); more raise LrmError, the count is in .n_seg of the exception."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n, stride = reads.shape
    options = _anchor_options(options, True, anchor_min_len, True, clip_penalty, clip_end_bonus)
    options = {**options, "split": 1, "split_min_len": split_min_len}
    opt = capi.map_options(**options)
    text = bool(opt.cigar_text)
    dense = bool(opt.dense_results) or text
    if buffers is None:
        buffers = SplitBuffers(2 * n if cap is None else cap, int(lens.max()) if n else 0)
    cig = _cigars_of(res, n)
    meta = np.ascontiguousarray(res["meta"], dtype=META_DT)
    meta_r = np.ascontiguousarray(res["meta_r"], dtype=np.int32)
    rc = lib.lrm_split_batch(index.handle, reads.ctypes.data, stride, lens.ctypes.data, n, C.cast(cig, C.c_void_p), meta.ctypes.data,
                             meta_r.ctypes.data, capi.Params(n, seed_len, thres), capi.GactParams(*gact), C.byref(opt),
                             C.byref(buffers.out))
    if rc < 0:
        e = capi.LrmError("lrm_split_batch: " + lib.lrm_last_error().decode(errors="replace"))
        e.rc, e.n_seg = rc, int(buffers.out.n_seg)
        raise e
    return buffers.result(dense, text)


def result_flags(score, meta_r, meta, mapq=None):
    """lrm_result_flags; mapq: the MAPQ_DT records of the batch (lrm_result_flags_mapq: a mapped read's MAPQ is its record's)."""
    n = len(score)
    flag = np.zeros(n, dtype=np.int32)
    out = np.zeros(n, dtype=np.int32)
    valid = np.zeros(n, dtype=np.int32)
    score = np.ascontiguousarray(score, dtype=np.int32)
    meta_r = np.ascontiguousarray(meta_r, dtype=np.int32)
    meta = np.ascontiguousarray(meta, dtype=META_DT)
    if mapq is not None:
        mq = np.ascontiguousarray(mapq, dtype=MAPQ_DT)
        assert len(mq) == n
        lib.lrm_result_flags_mapq(score.ctypes.data, meta_r.ctypes.data, meta.ctypes.data, mq.ctypes.data, n, flag.ctypes.data,
                                  out.ctypes.data, valid.ctypes.data)
    else:
        lib.lrm_result_flags(score.ctypes.data, meta_r.ctypes.data, meta.ctypes.data, n, flag.ctypes.data,
                             out.ctypes.data, valid.ctypes.data)
    return flag, out, valid


class DeviceMapper:
    """Device-resident batches: torch tensors own the HBM buffers, kernels run on torch's
    current stream (so torch.cuda.Event brackets them)."""

    def __init__(self, index, n_max, max_len, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES, gact=DEFAULT_GACT,
                 device=0, anchored=False, anchor_min_len=0, clip=False, clip_penalty=0, clip_end_bonus=0, split=False,
                 split_min_len=0, seg_cap=None, seg_rows=None, mapq=False, summary=False):
        """summary: extend() runs the alignment summary stage behind the extension, whichever mode (lrm_aln_summary_dev);
        summary_records(n) and results(n)["summary"] are the SUMMARY_DT records of the last extend call.
        mapq: seed() runs the mapping-quality stage behind the seed stage (lrm_seed_batch_mapq_dev); mapq_records(n) and
        results(n)["mapq"] are the MAPQ_DT records of the last seed call.
        split (needs clip): split() after extend() maps the soft-clipped ends of at least split_min_len bases (0 = 200) as
        reads of their own (lrm_split_batch_dev), results() returns them as res["split"].  seg_cap: room for that many
        segments (None: 2 * n_max, every possible one); seg_rows: rows of the segment workspace (None: min(seg_cap, n_max);
        0: no workspace of its own -- the primary's is used a second time); more segments than rows run in chunks."""
        import torch
        self.torch = torch
        self.index = index
        self.n_max, self.max_len = n_max, max_len
        self.seed_len, self.thres, self.gact = seed_len, thres, gact
        self.dev = torch.device("cuda", device)
        ws = C.c_void_p()
        check(lib.lrm_workspace_create(C.byref(ws), index.handle, n_max, max_len, seed_len, thres),
              "lrm_workspace_create")
        self.ws = ws
        anchored = bool(anchored or clip)
        self.anchored, self.anchor_min_len = anchored, anchor_min_len
        self.clip_on, self.clip_penalty, self.clip_end_bonus = bool(clip), clip_penalty, clip_end_bonus
        # anchored: lrm_extend_batch_anchored_dev, results() also returns the lrm_anchor records; clip (implies anchored):
        # lrm_extend_batch_clipped_dev, results() also returns the lrm_clip records (soft-clipped bases per read)
        self.store_stride = (anchored_store_stride(max_len) + 15) // 16 * 16 if anchored else 2 * max_len
        self.best = torch.zeros((n_max, 3), dtype=torch.int64, device=self.dev)       # lrm_entry
        self.store = torch.zeros((n_max, self.store_stride), dtype=torch.uint8, device=self.dev)
        self.n_ops = torch.zeros(n_max, dtype=torch.int32, device=self.dev)
        self.score = torch.zeros(n_max, dtype=torch.int32, device=self.dev)
        self.meta = torch.zeros((n_max, 24), dtype=torch.uint8, device=self.dev)      # lrm_seq_meta
        self.meta_r = torch.zeros(n_max, dtype=torch.int32, device=self.dev)
        self.anchor = torch.zeros((n_max, 32), dtype=torch.uint8, device=self.dev) if anchored else None     # lrm_anchor
        self.clip = torch.zeros((n_max, 2), dtype=torch.int32, device=self.dev) if clip else None           # lrm_clip
        self.mapq = torch.zeros((n_max, 16), dtype=torch.uint8, device=self.dev) if mapq else None           # lrm_mapq
        self.summary = torch.zeros((n_max, 32), dtype=torch.uint8, device=self.dev) if summary else None    # lrm_aln_summary
        self.split_on, self.split_min_len, self.ws_seg, self.n_seg = bool(split), split_min_len, None, 0
        if split:
            if not clip:
                raise capi.LrmError("DeviceMapper: split needs clip")
            cap = self.seg_cap = 2 * n_max if seg_cap is None else seg_cap
            rows = min(cap, n_max) if seg_rows is None else seg_rows
            if rows:
                wseg = C.c_void_p()
                check(lib.lrm_workspace_create(C.byref(wseg), index.handle, rows, max_len, seed_len, thres), "lrm_workspace_create")
                self.ws_seg = wseg
            k = max(cap, 1)
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
            self.seg_row_stride = (max_len + 16) // 16 * 16
            self.seg = dict(seg=z((k, 4), torch.int32), rows=z((k, self.seg_row_stride), torch.uint8), lens=z(k, torch.int32),
                            best=z((k, 3), torch.int64), store=z((k, self.store_stride), torch.uint8), n_ops=z(k, torch.int32),
                            score=z(k, torch.int32), meta=z((k, 24), torch.uint8), meta_r=z(k, torch.int32),
                            anchor=z((k, 32), torch.uint8), clip=z((k, 2), torch.int32))
            g = self.seg
            self.split_dev = capi.SplitDev(cap, g["seg"].data_ptr(), g["rows"].data_ptr(), self.seg_row_stride, g["lens"].data_ptr(),
                                           g["best"].data_ptr(), g["store"].data_ptr(), self.store_stride, g["n_ops"].data_ptr(),
                                           g["score"].data_ptr(), g["meta"].data_ptr(), g["meta_r"].data_ptr(),
                                           g["anchor"].data_ptr(), g["clip"].data_ptr())

    def workspace_bytes(self):
        return int(lib.lrm_workspace_bytes(self.ws))

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def seed(self, d_reads, d_lens, n=None):
        n = d_reads.shape[0] if n is None else n
        p = capi.Params(n, self.seed_len, self.thres)
        if self.mapq is not None:
            check(lib.lrm_seed_batch_mapq_dev(self.index.handle, self.ws, d_reads.data_ptr(), d_reads.stride(0),
                                              d_lens.data_ptr(), n, self.max_len, p, self.best.data_ptr(),
                                              self.mapq.data_ptr(), self._stream()), "lrm_seed_batch_mapq_dev")
            return
        check(lib.lrm_seed_batch_dev(self.index.handle, self.ws, d_reads.data_ptr(), d_reads.stride(0),
                                     d_lens.data_ptr(), n, self.max_len, p, self.best.data_ptr(), self._stream()),
              "lrm_seed_batch_dev")

    def mapq_records(self, n):
        """The lrm_mapq records (MAPQ_DT) of the last seed() -- DeviceMapper(..., mapq=True)."""
        assert self.mapq is not None
        return self.mapq[:n].cpu().numpy().reshape(-1).view(MAPQ_DT)

    def summary_records(self, n):
        """The lrm_aln_summary records (SUMMARY_DT) of the last extend() -- DeviceMapper(..., summary=True)."""
        assert self.summary is not None
        return self.summary[:n].cpu().numpy().reshape(-1).view(SUMMARY_DT)

    def extend(self, d_reads, d_lens, n=None):
        n = d_reads.shape[0] if n is None else n
        self._extend(d_reads, d_lens, n)
        if self.summary is not None:
            check(lib.lrm_aln_summary_dev(self.index.handle, self.store.data_ptr(), self.store_stride, self.n_ops.data_ptr(),
                                          self.score.data_ptr(), self.meta_r.data_ptr(), n, self.summary.data_ptr(),
                                          self._stream()), "lrm_aln_summary_dev")

    def _extend(self, d_reads, d_lens, n):
        gp = capi.GactParams(*self.gact)
        if self.clip_on:
            check(lib.lrm_extend_batch_clipped_dev(self.index.handle, self.ws, d_reads.data_ptr(), d_reads.stride(0),
                                                   d_lens.data_ptr(), n, self.max_len, self.best.data_ptr(), gp,
                                                   self.store.data_ptr(), self.store_stride, self.n_ops.data_ptr(),
                                                   self.score.data_ptr(), self.meta.data_ptr(), self.meta_r.data_ptr(),
                                                   self.anchor.data_ptr(), self.anchor_min_len, self.clip_penalty,
                                                   self.clip_end_bonus, self.clip.data_ptr(), self._stream()),
                  "lrm_extend_batch_clipped_dev")
            return
        if self.anchored:
            check(lib.lrm_extend_batch_anchored_dev(self.index.handle, self.ws, d_reads.data_ptr(), d_reads.stride(0),
                                                    d_lens.data_ptr(), n, self.max_len, self.best.data_ptr(), gp,
                                                    self.store.data_ptr(), self.store_stride, self.n_ops.data_ptr(),
                                                    self.score.data_ptr(), self.meta.data_ptr(), self.meta_r.data_ptr(),
                                                    self.anchor.data_ptr(), self.anchor_min_len, self._stream()),
                  "lrm_extend_batch_anchored_dev")
            return
        check(lib.lrm_extend_batch_dev(self.index.handle, self.ws, d_reads.data_ptr(), d_reads.stride(0),
                                       d_lens.data_ptr(), n, self.max_len, self.best.data_ptr(), gp,
                                       self.store.data_ptr(), self.store_stride, self.n_ops.data_ptr(),
                                       self.score.data_ptr(), self.meta.data_ptr(), self.meta_r.data_ptr(),
                                       self._stream()), "lrm_extend_batch_dev")

    def split(self, d_reads, d_lens, n=None):
        """lrm_split_batch_dev after extend() on the same stream -> number of segments (the call waits for that count).
        More than seg_cap raise LrmError with .rc == -3 and .n_seg."""
        assert self.split_on
        n = d_reads.shape[0] if n is None else n
        k = C.c_uint64()
        rc = lib.lrm_split_batch_dev(self.index.handle, self.ws_seg or self.ws, d_reads.data_ptr(), d_reads.stride(0), d_lens.data_ptr(),
                                     n, self.clip.data_ptr(), capi.Params(n, self.seed_len, self.thres), capi.GactParams(*self.gact),
                                     self.anchor_min_len, self.clip_penalty, self.clip_end_bonus, self.split_min_len,
                                     C.byref(self.split_dev), C.byref(k), self._stream())
        self.n_seg = int(k.value) if rc >= 0 else 0
        if rc < 0:
            e = capi.LrmError("lrm_split_batch_dev: " + lib.lrm_last_error().decode(errors="replace"))
            e.rc, e.n_seg = rc, int(k.value)
            raise e
        return self.n_seg

    def seg_timing(self):
        """timing() of the segment workspace (the split stage's own kernels are in the revcomp_kernel slot)."""
        ms = np.zeros(N_KERNELS, dtype=np.float64)
        launches = np.zeros(N_KERNELS, dtype=np.uint64)
        check(lib.lrm_workspace_timing(self.ws_seg or self.ws, ms.ctypes.data, launches.ctypes.data, self._stream()),
              "lrm_workspace_timing")
        return {lib.lrm_kernel_name(i).decode(): (float(ms[i]), int(launches[i])) for i in range(N_KERNELS)}

    def split_results(self):
        """The outputs of the last split() as numpy arrays (same keys as split_batch, `ops` in rows)."""
        k, g = self.n_seg, self.seg
        h = {name: t[:k].cpu().numpy() for name, t in g.items()}
        best = np.zeros(k, dtype=ENTRY_DT)
        b = h["best"].view(np.uint64).reshape(k, 3)
        best["key"], best["val"], best["bucket"] = b[:, 0], b[:, 1], b[:, 2]
        return dict(seg=h["seg"].reshape(-1).view(SEGMENT_DT), rows=h["rows"], lens=h["lens"].view(np.uint32), best=best,
                    ops=h["store"], n_ops=h["n_ops"], score=h["score"], meta=h["meta"].reshape(-1).view(META_DT),
                    meta_r=h["meta_r"], anchor=h["anchor"].reshape(-1).view(ANCHOR_DT), clip=h["clip"].reshape(-1).view(CLIP_DT),
                    is_text=False)

    def stats(self):
        st = capi.Stats()
        check(lib.lrm_workspace_stats(self.ws, C.byref(st), self._stream()), "lrm_workspace_stats")
        return dict(vote_tier2_items=int(st.vote_tier2_items), vote_tier3_items=int(st.vote_tier3_items),
                    reads_decided_phase0=int(st.reads_decided_phase0), gact_tiles=int(st.gact_tiles),
                    seeds_evaluated=int(st.seeds_evaluated), seed_table_lookups=int(st.seed_table_lookups),
                    seed_rank_requests=int(st.seed_rank_requests), vote_redo_items=int(st.vote_redo_items),
                    **{name: int(getattr(st, name)) for name in capi.BS_COUNTERS})

    def debug_vote_results(self, n):
        """lrm_debug_vote_results: (n, seed_len + 1, 6) uint64 -- key1, val1, bucket1, key2, val2, bucket2 of every (read, phase)
        of the last seed() call as the vote kernels left them; only the phases that call evaluated are meaningful."""
        out = np.zeros((n, self.seed_len + 1, 6), dtype=np.uint64)
        check(lib.lrm_debug_vote_results(self.ws, n, out.ctypes.data, self._stream()), "lrm_debug_vote_results")
        return out

    def set_counting(self, enable=True):
        """The next seed and extend calls run the counting builds of the seed kernel (stats(): requests of the device
        layout) and of the bit-sliced extension kernel (stats(): bs_* path counts)."""
        check(lib.lrm_workspace_set_counting(self.ws, int(enable)), "lrm_workspace_set_counting")

    def set_timing(self, enable=True):
        check(lib.lrm_workspace_set_timing(self.ws, int(enable)), "lrm_workspace_set_timing")

    def timing(self):
        """-> {kernel name: (total ms, launches)} accumulated since set_timing / the last call."""
        ms = np.zeros(N_KERNELS, dtype=np.float64)
        launches = np.zeros(N_KERNELS, dtype=np.uint64)
        check(lib.lrm_workspace_timing(self.ws, ms.ctypes.data, launches.ctypes.data, self._stream()),
              "lrm_workspace_timing")
        return {lib.lrm_kernel_name(i).decode(): (float(ms[i]), int(launches[i])) for i in range(N_KERNELS)}

    def results(self, n):
        """Copy the outputs of the last seed+extend to numpy (host)."""
        best = self.best[:n].cpu().numpy().view(np.uint64).reshape(n, 3)
        out = np.zeros(n, dtype=ENTRY_DT)
        out["key"], out["val"], out["bucket"] = best[:, 0], best[:, 1], best[:, 2]
        meta = self.meta[:n].cpu().numpy().reshape(-1).view(META_DT)
        res = dict(best=out, ops=self.store[:n].cpu().numpy(), n_ops=self.n_ops[:n].cpu().numpy(),
                   score=self.score[:n].cpu().numpy(), meta=meta, meta_r=self.meta_r[:n].cpu().numpy())
        if self.anchored:
            res["anchor"] = self.anchor[:n].cpu().numpy().reshape(-1).view(ANCHOR_DT)
        if self.clip_on:
            res["clip"] = self.clip[:n].cpu().numpy().reshape(-1).view(CLIP_DT)
        if self.split_on:
            res["split"] = self.split_results()
        if self.mapq is not None:
            res["mapq"] = self.mapq_records(n)
        if self.summary is not None:
            res["summary"] = self.summary_records(n)
        return res

    def close(self):
        if getattr(self, "ws_seg", None):
            lib.lrm_workspace_free(self.ws_seg)
            self.ws_seg = None
        if self.ws:
            lib.lrm_workspace_free(self.ws)
            self.ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
