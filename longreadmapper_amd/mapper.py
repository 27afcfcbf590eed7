"""Batch entry points of the hot path on host buffers (device buffers: DeviceMapper, device.py).

`seed_batch` / `extend_batch` are PART 1 / PART 2 of single_end() (alnmain.c:333-451) for a
whole batch; names, argument meaning and data conventions follow the reference (best[],
cig[], limit[], meta_r[], m[])."""
import ctypes as C
import weakref

import numpy as np

from . import capi
from .capi import check, lib
from .device import DeviceMapper  # noqa: F401  (every public name of the binding stays importable from here)
from .records import (ANCHOR_DT, CIGAR_DT, CLIP_DT, DEFAULT_GACT, DEFAULT_SEED_LEN, DEFAULT_THRES, ENTRY_DT, MAPQ_DT,  # noqa: F401
                      MAPQ_OVERFLOW, META_DT, N_KERNELS, DIFF_NO_ROOM, SEC_ALIGNED, SEC_DUPLICATE, SECONDARY_DT, SEG_ALIGNED, SEG_RIGHT, SEGMENT_DT, SUMMARY_DT, anchored_store_stride,
                      store_need, units16)
from .textio import cigar_table


def _fields(record):
    return {f: int(getattr(record, f)) for f, _ in record._fields_}


def aln_summary_host(ops):
    """lrm_aln_summary_host: the alignment summary record of one alignment's op bytes -> dict of the lrm_aln_summary fields."""
    data = bytes(ops)
    a = capi.AlnSummary()
    lib.lrm_aln_summary_host(data, len(data), C.byref(a))
    return _fields(a)


def aln_diff_host(ops, target):
    """lrm_aln_diff_host: the difference events (uint32 words) of one alignment's op bytes against `target`, the text from the
    first aligned target base on (what is left of it: positions behind its end give base 0)."""
    data, text = bytes(ops), bytes(target)
    count = int(lib.lrm_aln_diff_host(data, len(data), text, len(text), None))
    ev = np.zeros(max(count, 1), dtype=np.uint32)
    got = int(lib.lrm_aln_diff_host(data, len(data), text, len(text), ev.ctypes.data))
    assert got == count
    return ev[:count]


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
    return _fields(a)


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


def _batch(reads, lens):
    """-> (lens as uint32, n, max_len, the (reads, stride, lens, n) arguments every batch call takes after the handle)."""
    assert reads.dtype == np.uint8 and reads.flags.c_contiguous and reads.flags.writeable
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n, stride = reads.shape
    return lens, n, int(lens.max()) if n else 0, (reads.ctypes.data, stride, lens.ctypes.data, n)


class ResultBuffers:
    """The host arrays a batch call fills for up to n reads: best, cig (CIGAR_DT), store, score, meta, meta_r and, asked
    for, the mapq / summary records.  store: the caller's own (n, stride) uint8 array instead of a new one."""

    def __init__(self, n, store_stride=None, store=None, mapq=False, summary=False, md=False, md_cap=None, md_events=None):
        self.best = np.zeros(n, dtype=ENTRY_DT)
        self.cig = np.zeros(max(n, 1), dtype=CIGAR_DT)
        self.store = np.zeros((n, store_stride), dtype=np.uint8) if store is None else store
        self.score = np.zeros(n, dtype=np.int32)
        self.meta = np.zeros(n, dtype=META_DT)
        self.meta_r = np.zeros(n, dtype=np.int32)
        self.extras = {}          # "mapq" / "summary": the record arrays the batch fills on top
        if mapq:
            self.extras["mapq"] = np.zeros(n, dtype=MAPQ_DT)
        if summary:
            self.extras["summary"] = np.zeros(n, dtype=SUMMARY_DT)
        self.diff = None
        if md:          # the difference events: room for md_cap of them (None: the bound, a read has no more events than columns)
            cap = n * self.store.shape[1] if md_cap is None else md_cap
            self.md_off, self.md_cnt = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
            if md_events is not None:           # the caller's own uint32 array (e.g. pinned: the events are then DMA'd straight into it)
                assert md_events.dtype == np.uint32 and md_events.flags.c_contiguous and len(md_events) >= cap
            self.md_events = np.empty(max(cap, 1), dtype=np.uint32) if md_events is None else md_events
            self.md_needed = np.zeros(1, dtype=np.uint64)
            self.diff = capi.BatchDiff(C.sizeof(capi.BatchDiff), 0, self.md_off.ctypes.data, self.md_cnt.ctypes.data,
                                       self.md_events.ctypes.data if cap else None, cap, self.md_needed.ctypes.data)
        # (cig_out, store_mem, store_stride, score_out, meta_out, meta_r): how every batch call's argument list ends
        self.out_args = (self.cig.ctypes.data, self.store.ctypes.data, self.store.shape[1], self.score.ctypes.data,
                         self.meta.ctypes.data, self.meta_r.ctypes.data)

    def result(self, k=None, dense=False, text=None, **more):
        """dict of the first k rows (None: all n) [and of those of the arrays in `more`].  dense: with ops_off, since
        cig[i].cigar = store_mem + off[i]; text (not None): with is_text -- True: cig[i].cigar -> NUL-terminated run-length
        CIGAR text, text_of(res, i)."""
        k = len(self.best) if k is None else k
        res = dict(best=self.best[:k], ops=self.store, n_ops=self.cig["n_cigar_op"][:k].copy(), score=self.score[:k],
                   meta=self.meta[:k], meta_r=self.meta_r[:k], **{f: a[:k] for f, a in {**more, **self.extras}.items()})
        if self.diff is not None:
            res.update(md_off=self.md_off[:k], md_cnt=self.md_cnt[:k], md_events=self.md_events, md_needed=int(self.md_needed[0]))
        if dense:
            res["ops_off"] = (self.cig["cigar"][:k] - np.uint64(self.store.ctypes.data)).astype(np.int64)
        if text is not None:
            res["is_text"] = text
        return res


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
    lens, n, max_len, batch = _batch(reads, lens)
    best = np.ascontiguousarray(best, dtype=ENTRY_DT)
    buf = ResultBuffers(n, max(store_need(max_len, anchored), 1))
    check(lib.lrm_extend_batch(index.handle, *batch, best.ctypes.data, capi.GactParams(*gact), *buf.out_args), "lrm_extend_batch")
    res = buf.result()
    del res["best"]          # (the caller's, not a result)
    return res


def pinned_empty(shape, dtype=np.uint8):
    """numpy array in pinned host memory (lrm_host_alloc): the DMA engines read / write it directly.
    Free with pinned_free(arr)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = lib.lrm_host_alloc(max(n, 1))
    if not p:
        raise capi.failure("lrm_host_alloc")
    buf = (C.c_char * max(n, 1)).from_address(p)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    return arr


def pinned_free(arr):
    lib.lrm_host_free(arr.ctypes.data)


def _abandon(ticket, *arrays):
    lib.lrm_map_batch_wait(ticket)       # the code is nobody's any more; `arrays` go once this returns


class PendingBatch:
    """A batch submitted with map_batch_submit: wait() blocks until its results are in the caller's arrays.

    Until then the issuer and collector threads of the handle write into the arrays of the batch, and this object holds
    the only references to some of them.  One that is dropped (or left as a `with` block) without wait() therefore
    waits for its ticket first and lets go of the arrays after: numpy never frees a DMA target, no ticket leaks.  The
    order against the index's own finalizer does not matter: lrm_index_free lets the batches in flight run to
    completion and their tickets stay valid (host_pipeline.hip, lrm_host_ctx_free)."""

    def __init__(self, ticket, buffers, keep, dense, text):
        self.ticket, self._buffers, self.dense, self.text = ticket, buffers, dense, text
        self._keep = keep                # reads, lens: wait() detaches the finalizer, which drops ITS references, before it waits
        self._finalizer = weakref.finalize(self, _abandon, ticket, buffers, *keep)

    def wait(self):
        t, self.ticket = self.ticket, None
        assert t is not None, "already waited for"
        self._finalizer.detach()
        check(lib.lrm_map_batch_wait(t), "lrm_map_batch_wait")
        return self._buffers.result(dense=self.dense, text=self.text)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._finalizer.alive:        # not waited for: as when dropped
            self._finalizer()
            self.ticket = None


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
                     summary=False, md=False, md_cap=None, md_events=None, pileup=None, pileup_min_mapq=0):
    """pileup: a pileup.Pileup, or a list with one per replica of the handle (lrm_map_batch_submit_ex3; docs/GACT_SPEC.md, "Pileup on
    the host-buffer path and across replicas"): every extension group of the batch is added to its replica's accumulator; with
    mapq=True only the reads whose record says mapq >= pileup_min_mapq.  All counts are in when wait() returns; every other
    output is the same bytes.
    md_events: a caller-provided uint32 array for the events (needs md_cap; e.g. pinned_empty).  md=True (lrm_map_batch_submit_ex2): the result gains the difference events of the batch -- md_off, md_cnt (per read),
    md_events (uint32 words; read i's are md_events[md_off[i]:md_off[i] + md_cnt[i]], md_off[i] == DIFF_NO_ROOM: no room) and
    md_needed, the batch's total; md_cap: room for that many events (None: the bound n * store_stride).
    lrm_map_batch_submit_ex (mapq=True: the result gains "mapq", the MAPQ_DT records of the batch; summary=True: it gains
    "summary", the SUMMARY_DT records; neither: lrm_map_batch_submit): queues the batch and returns a PendingBatch.  `reads` is modified in place like
    extend_batch once the batch runs; `store` may be a caller-provided (n, >= 2*max_len) uint8 array (e.g. pinned;
    anchored: >= anchored_store_stride(max_len)); `options`: dict of lrm_map_options fields (None: the handle's
    defaults); anchored=True adds the anchored extension mode to them, clip=True that mode with its end clipping
    (see extend_batch)."""
    lens, n, max_len, batch = _batch(reads, lens)
    options = _anchor_options(options, anchored, anchor_min_len, clip, clip_penalty, clip_end_bonus)
    anchored = bool(options and options.get("anchored"))
    buf = ResultBuffers(n, max(units16(store_need(max_len, anchored)), 16), store, mapq, summary, md, md_cap, md_events)
    opt = capi.map_options(**options) if options is not None else None
    ticket = C.c_void_p()
    ex = capi.BatchExtras(C.sizeof(capi.BatchExtras), 0, buf.extras["mapq"].ctypes.data if mapq else None,
                          buf.extras["summary"].ctypes.data if summary else None)
    if pileup is not None:
        piles = list(pileup) if isinstance(pileup, (list, tuple)) else [pileup]
        arr = (C.c_void_p * max(len(piles), 1))(*[None if a is None else a.handle for a in piles])
        bp = capi.BatchPileup(C.sizeof(capi.BatchPileup), pileup_min_mapq, arr, len(piles), 0)
        check(lib.lrm_map_batch_submit_ex3(index.handle, *batch, capi.Params(n, seed_len, thres), capi.GactParams(*gact),
                                           buf.best.ctypes.data, *buf.out_args, C.byref(opt) if opt is not None else None,
                                           C.byref(ex) if buf.extras else None, C.byref(buf.diff) if md else None, C.byref(bp),
                                           C.byref(ticket)), "lrm_map_batch_submit_ex3")
        text = bool(opt.cigar_text) if opt is not None else False
        dense = (bool(opt.dense_results) or text) if opt is not None else False
        return PendingBatch(ticket, buf, (reads, lens, *piles), dense, text)          # (the accumulators outlive the ticket)
    if md:
        check(lib.lrm_map_batch_submit_ex2(index.handle, *batch, capi.Params(n, seed_len, thres), capi.GactParams(*gact),
                                           buf.best.ctypes.data, *buf.out_args, C.byref(opt) if opt is not None else None,
                                           C.byref(ex) if buf.extras else None, C.byref(buf.diff), C.byref(ticket)),
              "lrm_map_batch_submit_ex2")
    else:
        check(lib.lrm_map_batch_submit_ex(index.handle, *batch, capi.Params(n, seed_len, thres), capi.GactParams(*gact),
                                          buf.best.ctypes.data, *buf.out_args, C.byref(opt) if opt is not None else None,
                                          C.byref(ex) if buf.extras else None, C.byref(ticket)), "lrm_map_batch_submit_ex")
    text = bool(opt.cigar_text) if opt is not None else False
    dense = (bool(opt.dense_results) or text) if opt is not None else False
    return PendingBatch(ticket, buf, (reads, lens), dense, text)


def map_batch(index, reads, lens, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES, gact=DEFAULT_GACT, store=None,
              options=None, anchored=False, anchor_min_len=0, clip=False, clip_penalty=0, clip_end_bonus=0, mapq=False, summary=False,
              md=False, md_cap=None, md_events=None, pileup=None, pileup_min_mapq=0):
    """pileup, pileup_min_mapq: see map_batch_submit (submit + wait).
    PART 1 + PART 2 in one device pass; `reads` is modified in place like extend_batch.
    Without `options` this is lrm_map_batch (the handle's default options), with them (or with anchored=True or
    clip=True, which are among them) submit + wait.  mapq=True: the mapping-quality records (MAPQ_DT) come back as
    res["mapq"] next to the other results, which do not change; summary=True: the alignment summary records (SUMMARY_DT) as
    res["summary"], likewise (submit + wait through lrm_map_batch_submit_ex); md=True: the difference events as md_off, md_cnt,
    md_events and md_needed (map_batch_submit)."""
    options = _anchor_options(options, anchored, anchor_min_len, clip, clip_penalty, clip_end_bonus)
    if options is not None or mapq or summary or md or pileup is not None:
        return map_batch_submit(index, reads, lens, seed_len, thres, gact, store, options, mapq=mapq, summary=summary, md=md,
                                md_cap=md_cap, md_events=md_events, pileup=pileup, pileup_min_mapq=pileup_min_mapq).wait()
    lens, n, max_len, batch = _batch(reads, lens)
    buf = ResultBuffers(n, max(store_need(max_len, False), 1), store)
    check(lib.lrm_map_batch(index.handle, *batch, capi.Params(n, seed_len, thres), capi.GactParams(*gact), buf.best.ctypes.data,
                            *buf.out_args), "lrm_map_batch")
    return buf.result()


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


class _PassBuffers(ResultBuffers):
    """Host arrays of a second pass's out struct (lrm_split_out, lrm_secondary_out) for up to cap rows of up to max_len bases.
    A subclass names the dtype of its table and its struct; both structs have their fields in the same order."""
    TABLE_DT = OUT = None

    def __init__(self, cap, max_len, anchored):
        self.cap = cap
        self.row_stride = (max_len + 16) // 16 * 16
        self.store_stride = max(units16(store_need(max_len, anchored)), 16)
        k = max(cap, 1)
        super().__init__(k, self.store_stride)
        self.table = np.zeros(k, dtype=self.TABLE_DT)
        self.rows = np.zeros((k, self.row_stride), dtype=np.uint8)
        self.lens = np.zeros(k, dtype=np.uint32)
        self.anchor = np.zeros(k, dtype=ANCHOR_DT)
        self.clip = np.zeros(k, dtype=CLIP_DT)
        cig, store, store_stride, score, meta, meta_r = self.out_args
        self.out = self.OUT(cap, 0, self.table.ctypes.data, self.rows.ctypes.data, self.row_stride, self.lens.ctypes.data,
                            self.best.ctypes.data, cig, store, store_stride, score, meta, meta_r, self.anchor.ctypes.data,
                            self.clip.ctypes.data)

    def _result(self, k, dense, text, table, entry="best"):
        res = super().result(k, dense, text, **{table: self.table}, rows=self.rows, lens=self.lens, anchor=self.anchor, clip=self.clip)
        if entry != "best":
            res[entry] = res.pop("best")
        res["buffers"] = self
        return res


class SplitBuffers(_PassBuffers):
    """Host arrays of an lrm_split_out for up to cap segments of up to max_seg bases."""
    TABLE_DT, OUT = SEGMENT_DT, capi.SplitOut

    def __init__(self, cap, max_seg):
        super().__init__(cap, max_seg, True)
        self.seg = self.table

    def result(self, k=None, dense=False, text=None):
        return self._result(int(self.out.n_seg) if k is None else k, dense, text, "seg")


class SecondaryBuffers(_PassBuffers):
    """Host arrays of an lrm_secondary_out for up to cap candidates of up to max_len bases."""
    TABLE_DT, OUT = SECONDARY_DT, capi.SecondaryOut

    def result(self, dense=False, text=None):
        return self._result(int(self.out.n_sec), dense, text, "table", "rival")


def _second_pass_args(reads, lens, res, options):
    """What split_batch and secondary_batch hand to the library alike: the caller's arrays in the library's types, the
    lrm_map_options (None: the handle's defaults) and the layout they give -> reads, lens, meta, meta_r, opt, text, dense"""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    opt = capi.map_options(**options) if options is not None else None
    text = bool(opt.cigar_text) if opt is not None else False
    dense = (bool(opt.dense_results) or text) if opt is not None else False
    meta = np.ascontiguousarray(res["meta"], dtype=META_DT)
    meta_r = np.ascontiguousarray(res["meta_r"], dtype=np.int32)
    return reads, lens, meta, meta_r, opt, text, dense


def _cigars_of(res, n):
    """lrm_cigar array that points into a map_batch result, as the C caller would still hold it."""
    ops = res["ops"]
    off = res["ops_off"][:n] if "ops_off" in res else np.arange(n, dtype=np.int64) * (ops.shape[1] if ops.ndim == 2 else 0)
    return cigar_table(np.asarray(off).astype(np.uint64) + np.uint64(ops.ctypes.data), res["n_ops"][:n], res["score"][:n])


def split_batch(index, reads, lens, res, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES, gact=DEFAULT_GACT, options=None,
                anchor_min_len=0, clip_penalty=0, clip_end_bonus=0, split_min_len=0, cap=None, buffers=None):
    """lrm_split_batch: the second pass over `res`, what map_batch(index, reads, lens, clip=True, ...) returned for `reads`
    (as that call left them), with the same options.  -> dict(seg=SEGMENT_DT table, rows, lens, best, ops, n_ops, score, meta,
    meta_r, anchor, clip [, ops_off]); ops_of / text_of read a segment's alignment like a read's.  cap: room for that many
    segments (None: for every possible one); more raise LrmError, the count is in .n_seg of the exception."""
    options = _anchor_options(options, True, anchor_min_len, True, clip_penalty, clip_end_bonus)
    options = {**options, "split": 1, "split_min_len": split_min_len}
    reads, lens, meta, meta_r, opt, text, dense = _second_pass_args(reads, lens, res, options)
    n, stride = reads.shape
    if buffers is None:
        buffers = SplitBuffers(2 * n if cap is None else cap, int(lens.max()) if n else 0)
    cig = _cigars_of(res, n)
    rc = lib.lrm_split_batch(index.handle, reads.ctypes.data, stride, lens.ctypes.data, n, cig.ctypes.data, meta.ctypes.data,
                             meta_r.ctypes.data, capi.Params(n, seed_len, thres), capi.GactParams(*gact), C.byref(opt),
                             C.byref(buffers.out))
    if rc < 0:
        raise capi.failure("lrm_split_batch", rc=rc, n_seg=int(buffers.out.n_seg))
    return buffers.result(dense=dense, text=text)


def secondary_batch(index, reads, lens, res, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES, gact=DEFAULT_GACT, options=None,
                    anchored=False, anchor_min_len=0, clip=False, clip_penalty=0, clip_end_bonus=0, min_hits=0, ratio_pct=0, cap=None):
    """lrm_secondary_batch: the second pass over `res`, what map_batch(index, reads, lens, mapq=True, ...) returned for `reads`
    (as that call left them; options: that call's -- keep_reads says whether reverse-strand reads were turned round, cigar_text
    / dense_results the layout of the candidates' alignments).  anchored / clip ...: the extension the candidates go through.
    -> dict(table=SECONDARY_DT, rows, lens, rival, ops, n_ops, score, meta, meta_r, anchor, clip [, ops_off]); ops_of / text_of
    read a candidate's alignment like a read's; res["buffers"].out is the lrm_secondary_out (textio.sam_format(secondary=...)).
    cap: room for that many candidates (None: every read); more raise LrmError with .rc == -3 and .n_sec."""
    reads, lens, meta, meta_r, opt, text, dense = _second_pass_args(reads, lens, res, options)
    n, stride = reads.shape
    anchored = bool(anchored or clip)
    so = capi.SecondaryOptions(C.sizeof(capi.SecondaryOptions), min_hits, ratio_pct, int(anchored), anchor_min_len, int(bool(clip)),
                               clip_penalty, clip_end_bonus)
    buffers = SecondaryBuffers(n if cap is None else cap, int(lens.max()) if n else 0, anchored)
    mq = np.ascontiguousarray(res["mapq"], dtype=MAPQ_DT)
    rc = lib.lrm_secondary_batch(index.handle, reads.ctypes.data, stride, lens.ctypes.data, n, mq.ctypes.data, meta.ctypes.data,
                                 meta_r.ctypes.data, capi.Params(n, seed_len, thres), capi.GactParams(*gact),
                                 C.byref(opt) if opt is not None else None, C.byref(so), C.byref(buffers.out))
    if rc < 0:
        raise capi.failure("lrm_secondary_batch", rc=rc, n_sec=int(buffers.out.n_sec))
    return buffers.result(dense=dense, text=text)


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
