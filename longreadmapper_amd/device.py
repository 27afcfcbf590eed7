"""Device-resident batches: DeviceMapper runs the stages on buffers that torch tensors own (host buffers: mapper.py)."""
import ctypes as C

import numpy as np

from . import capi
from .capi import check, lib
from .records import (ANCHOR_DT, CLIP_DT, DEFAULT_GACT, DEFAULT_SEED_LEN, DEFAULT_THRES, ENTRY_DT, MAPQ_DT, META_DT, N_KERNELS,
                      SECONDARY_DT, SEGMENT_DT, SUMMARY_DT, store_need, units16)


def _records(t, dt):
    """The rows of a device tensor as a numpy array of the records (dtype dt) they hold."""
    return t.cpu().numpy().reshape(-1).view(dt)


def _timing(ws, stream):
    """lrm_workspace_timing -> {kernel name: (total ms, launches)}."""
    ms = np.zeros(N_KERNELS, dtype=np.float64)
    launches = np.zeros(N_KERNELS, dtype=np.uint64)
    check(lib.lrm_workspace_timing(ws, ms.ctypes.data, launches.ctypes.data, stream), "lrm_workspace_timing")
    return {lib.lrm_kernel_name(i).decode(): (float(ms[i]), int(launches[i])) for i in range(N_KERNELS)}


class DeviceMapper:
    """Device-resident batches: torch tensors own the HBM buffers, kernels run on torch's
    current stream (so torch.cuda.Event brackets them)."""

    def __init__(self, index, n_max, max_len, seed_len=DEFAULT_SEED_LEN, thres=DEFAULT_THRES, gact=DEFAULT_GACT,
                 device=0, anchored=False, anchor_min_len=0, clip=False, clip_penalty=0, clip_end_bonus=0, split=False,
                 split_min_len=0, seg_cap=None, seg_rows=None, mapq=False, summary=False, md=False, secondary=False, sec_cap=None,
                 sec_min_hits=0, sec_ratio_pct=0, pileup=None, pileup_min_mapq=0, pileup_ins_cols=0):
        """pileup=(lo, hi): an accumulator over the text positions [lo, hi) (lrm_pileup_create; docs/GACT_SPEC.md, "Pileup";
        index.text_window gives a sequence's).  extend() adds every batch behind the summary and the event stages
        (lrm_pileup_add_dev) -- with mapq=True only the reads whose lrm_mapq record says mapq >= pileup_min_mapq -- and it
        stays in device memory across batches: pileup_columns() returns the PILEUP_COL_DT records, pileup_reset() clears it.
        pileup_ins_cols=K (1..8): the accumulator also counts the bases of the first K columns of every insertion
        (lrm_pileup_create_ins; docs/GACT_SPEC.md, "Pileup insertions and the polished consensus"): pileup_ins_columns(),
        pileup_polish() with the inserted bases, pileup_site_alleles().
        secondary (needs mapq): secondary() after seed() and extend() finds the rival locus of every candidate read and
        extends the read there, in this mapper's extension mode (lrm_secondary_batch_dev; docs/GACT_SPEC.md, "Secondary
        alignments"); secondary_results() returns the table and the per-candidate outputs.  sec_cap: room for that many
        candidates (None: n_max, every read); sec_min_hits, sec_ratio_pct: H and pct of the candidate test (0: 8, 50).  Nothing is
        allocated without it.  With split as well: secondary() comes before split() when the split stage runs on this
        mapper's own workspace (seg_rows=0); refused otherwise -- the split stage has seeded its segments there, and
        secondary() / rival() raise LrmError ("the workspace did not run the seed stage of this batch with the phase output")
        behind any seed stage on this workspace other than the last seed() of this batch.
        md (implies summary): extend() also makes the difference events of the batch (docs/GACT_SPEC.md, "Difference events
        and MD:Z": lrm_aln_diff_offsets_dev, then lrm_aln_diff_dev into a buffer of the batch's true total -- the one place
        extend() waits for the device: the total crosses to the host); diff_records(n) returns (offsets, events).
        summary: extend() runs the alignment summary stage behind the extension, whichever mode (lrm_aln_summary_dev);
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
        self.store_stride = units16(store_need(max_len, True)) if anchored else store_need(max_len, False)
        t = self._result_tensors(n_max)
        self.best, self.store, self.n_ops = t["best"], t["store"], t["n_ops"]
        self.score, self.meta, self.meta_r = t["score"], t["meta"], t["meta_r"]
        self.anchor = self._record_tensor(n_max, ANCHOR_DT) if anchored else None
        self.clip = self._record_tensor(n_max, CLIP_DT, torch.int32) if clip else None
        self.mapq = self._record_tensor(n_max, MAPQ_DT) if mapq else None
        self.summary = self._record_tensor(n_max, SUMMARY_DT) if summary or md else None
        self.diff_off = self._alloc(n_max + 1, torch.int64) if md else None
        self.diff_events = self._alloc(1, torch.int32) if md else None
        self.pileup, self.pileup_window, self.pileup_min_mapq = None, None, pileup_min_mapq
        self.pileup_ins_cols = int(pileup_ins_cols) if pileup is not None else 0
        if pileup is not None:
            pl = C.c_void_p()
            check(lib.lrm_pileup_create_ins(C.byref(pl), index.handle, int(pileup[0]), int(pileup[1]), self.pileup_ins_cols), "lrm_pileup_create_ins")
            self.pileup, self.pileup_window = pl, (int(pileup[0]), int(pileup[1]))
        self.sec, self.n_sec = None, 0
        if secondary:
            if not mapq:
                raise capi.LrmError("DeviceMapper: secondary needs mapq")
            cap = self.sec_cap = n_max if sec_cap is None else sec_cap
            k = max(cap, 1)
            self.sec_row_stride = (max_len + 16) // 16 * 16
            self.sec_store_stride = units16(self.store_stride)
            g = self.sec = dict(table=self._record_tensor(k, SECONDARY_DT, torch.int32),
                                rows=self._alloc((k, self.sec_row_stride), torch.uint8), lens=self._alloc(k, torch.int32),
                                rival=self._record_tensor(k, ENTRY_DT, torch.int64),
                                store=self._alloc((k, self.sec_store_stride), torch.uint8), n_ops=self._alloc(k, torch.int32),
                                score=self._alloc(k, torch.int32), meta=self._record_tensor(k, META_DT),
                                meta_r=self._alloc(k, torch.int32))
            if anchored:
                g["anchor"] = self._record_tensor(k, ANCHOR_DT)
            if clip:
                g["clip"] = self._record_tensor(k, CLIP_DT, torch.int32)
            ptr = {name: t.data_ptr() for name, t in g.items()}
            self.sec_dev = capi.SecondaryDev(cap, ptr["table"], ptr["rows"], self.sec_row_stride, ptr["lens"], ptr["rival"], ptr["store"],
                                             self.sec_store_stride, ptr["n_ops"], ptr["score"], ptr["meta"], ptr["meta_r"],
                                             ptr.get("anchor"), ptr.get("clip"))
            self.sec_opt = capi.SecondaryOptions(C.sizeof(capi.SecondaryOptions), sec_min_hits, sec_ratio_pct, int(anchored),
                                                 anchor_min_len, int(bool(clip)), clip_penalty, clip_end_bonus)
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
            self.seg_row_stride = (max_len + 16) // 16 * 16
            g = self.seg = dict(seg=self._record_tensor(k, SEGMENT_DT, torch.int32),
                                rows=self._alloc((k, self.seg_row_stride), torch.uint8), lens=self._alloc(k, torch.int32),
                                **self._result_tensors(k),
                                anchor=self._record_tensor(k, ANCHOR_DT), clip=self._record_tensor(k, CLIP_DT, torch.int32))
            self.split_dev = capi.SplitDev(cap, g["seg"].data_ptr(), g["rows"].data_ptr(), self.seg_row_stride, g["lens"].data_ptr(),
                                           g["best"].data_ptr(), g["store"].data_ptr(), self.store_stride, g["n_ops"].data_ptr(),
                                           g["score"].data_ptr(), g["meta"].data_ptr(), g["meta_r"].data_ptr(),
                                           g["anchor"].data_ptr(), g["clip"].data_ptr())

    def _alloc(self, shape, dtype):
        """Every buffer this mapper owns comes from here: zeros of the shape (tests override it to place guards around them)."""
        return self.torch.zeros(shape, dtype=dtype, device=self.dev)

    def _record_tensor(self, rows, dt, word=None):
        """Device buffer of `rows` records of dtype dt, as columns of `word` (default: bytes)."""
        word = word or self.torch.uint8
        return self._alloc((rows, dt.itemsize // word.itemsize), word)

    def _result_tensors(self, rows):
        """The result buffer set of `rows` reads: what an extension call writes, and best[] in front of it."""
        i32 = self.torch.int32
        return dict(best=self._record_tensor(rows, ENTRY_DT, self.torch.int64),
                    store=self._alloc((rows, self.store_stride), self.torch.uint8),
                    n_ops=self._alloc(rows, i32), score=self._alloc(rows, i32),
                    meta=self._record_tensor(rows, META_DT), meta_r=self._alloc(rows, i32))

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
        return _records(self.mapq[:n], MAPQ_DT)

    def summary_records(self, n):
        """The lrm_aln_summary records (SUMMARY_DT) of the last extend() -- DeviceMapper(..., summary=True)."""
        assert self.summary is not None
        return _records(self.summary[:n], SUMMARY_DT)

    def diff_records(self, n):
        """(offsets, events) of the last extend() -- DeviceMapper(..., md=True): n + 1 uint64 exclusive prefix sums of n_x + n_del,
        and the uint32 event words; read i's events are events[offsets[i]:offsets[i + 1]]."""
        assert self.diff_off is not None
        off = self.diff_off[:n + 1].cpu().numpy().view(np.uint64)
        return off, self.diff_events[:int(off[n])].cpu().numpy().view(np.uint32)

    def extend(self, d_reads, d_lens, n=None):
        n = d_reads.shape[0] if n is None else n
        self._extend(d_reads, d_lens, n)
        if self.summary is not None:
            check(lib.lrm_aln_summary_dev(self.index.handle, self.store.data_ptr(), self.store_stride, self.n_ops.data_ptr(),
                                          self.score.data_ptr(), self.meta_r.data_ptr(), n, self.summary.data_ptr(),
                                          self._stream()), "lrm_aln_summary_dev")
        if self.diff_off is not None:
            check(lib.lrm_aln_diff_offsets_dev(self.summary.data_ptr(), n, self.diff_off.data_ptr(), self._stream()),
                  "lrm_aln_diff_offsets_dev")
            total = int(self.diff_off[n].item())
            if total > self.diff_events.numel():
                self.diff_events = self._alloc(total, self.torch.int32)
            check(lib.lrm_aln_diff_dev(self.index.handle, self.store.data_ptr(), self.store_stride, self.n_ops.data_ptr(),
                                       self.score.data_ptr(), self.meta_r.data_ptr(), self.meta.data_ptr(), n, self.diff_off.data_ptr(),
                                       total, self.diff_events.data_ptr(), self._stream()), "lrm_aln_diff_dev")
        if self.pileup is not None:
            check(lib.lrm_pileup_add_dev(self.pileup, d_reads.data_ptr(), d_reads.stride(0), d_lens.data_ptr(), self.store.data_ptr(),
                                         self.store_stride, self.n_ops.data_ptr(), self.score.data_ptr(), self.meta_r.data_ptr(),
                                         self.meta.data_ptr(), n, self.mapq.data_ptr() if self.mapq is not None else None,
                                         self.pileup_min_mapq if self.mapq is not None else 0, self._stream()), "lrm_pileup_add_dev")

    def pileup_columns(self, first=None, count=None):
        """The PILEUP_COL_DT records of window positions first .. first + count - 1 (default: the whole window) of everything
        extend() has added since the accumulator was created or reset -- DeviceMapper(..., pileup=(lo, hi))."""
        assert self.pileup is not None
        first = 0 if first is None else first
        count = self.pileup_window[1] - self.pileup_window[0] - first if count is None else count
        out = self._record_tensor(max(count, 1), capi.PILEUP_COL_DT, self.torch.int32)
        check(lib.lrm_pileup_read_dev(self.pileup, first, count, out.data_ptr(), self._stream()), "lrm_pileup_read_dev")
        return _records(out[:count], capi.PILEUP_COL_DT)

    def pileup_sites(self, first=None, count=None, cap=None, min_depth=0, min_count=0, min_pct=0, consensus=False):
        """The call stage over the accumulator (lrm_pileup_sites_dev; docs/GACT_SPEC.md, "Pileup calls") on window positions
        first .. first + count - 1 (default: the whole window): -> (sites, total, cons).  sites: the PILEUP_SITE_DT records of
        the positions where the reads disagree with the text, ascending; total: their number; cons: with consensus=True one
        letter per position (uint8), else None.  A zero option means its default (8, 4, 25).  cap: the room of the first
        table (default: 4096 + count // 256 records); when the sites did not fit, the stage runs once more with cap = total
        -- the counters do not move, so the second call is the same question."""
        assert self.pileup is not None
        first = 0 if first is None else first
        count = self.pileup_window[1] - self.pileup_window[0] - first if count is None else count
        cap = min(count, 4096 + count // 256) if cap is None else cap
        opt = capi.PileupCallOptions(min_depth, min_count, min_pct, 0)
        d_total = self._alloc(1, self.torch.int64)
        d_cons = self._alloc(max(count, 1), self.torch.uint8) if consensus else None
        while True:
            d_sites = self._record_tensor(max(cap, 1), capi.PILEUP_SITE_DT, self.torch.int32)
            check(lib.lrm_pileup_sites_dev(self.pileup, C.byref(opt), first, count, d_sites.data_ptr() if cap else None, cap, d_total.data_ptr(),
                                           d_cons.data_ptr() if consensus else None, self._stream()), "lrm_pileup_sites_dev")
            total = int(d_total.cpu()[0])
            if total <= cap:
                break
            cap = total
        sites = _records(d_sites[:total], capi.PILEUP_SITE_DT)
        return sites, total, (d_cons[:count].cpu().numpy() if consensus else None)

    def _pileup_range(self, first, count):
        first = 0 if first is None else first
        return first, (self.pileup_window[1] - self.pileup_window[0] - first if count is None else count)

    def pileup_ins_columns(self, first=None, count=None):
        """The insertion words of window positions first .. first + count - 1 (default: the whole window) -> uint32 array of
        shape (count, K, 4): [position, insertion column, base class A C G T] (lrm_pileup_ins_read_dev) --
        DeviceMapper(..., pileup=(lo, hi), pileup_ins_cols=K)."""
        assert self.pileup is not None
        first, count = self._pileup_range(first, count)
        k = self.pileup_ins_cols
        out = self._alloc((max(count, 1), max(k, 1), 4), self.torch.int32)
        check(lib.lrm_pileup_ins_read_dev(self.pileup, first, count, out.data_ptr(), self._stream()), "lrm_pileup_ins_read_dev")
        return out[:count].cpu().numpy().view(np.uint32)

    def pileup_polish(self, first=None, count=None, cap=None, min_depth=0, min_count=0, min_pct=0):
        """The polished sequence of window positions first .. first + count - 1 (default: the whole window) as uint8 bytes
        (lrm_pileup_polish_dev): the consensus letters, deleted positions dropped, the inserted bases put in where the
        accumulator counts them (pileup_ins_cols) -- what textio.write_consensus takes for a window that is one sequence.
        cap: the room of the first buffer (default: count + count // 64 + 64); when the bytes did not fit, the stage runs
        once more with cap = the length -- the counters do not move, so the second call is the same question."""
        assert self.pileup is not None
        first, count = self._pileup_range(first, count)
        cap = count + count // 64 + 64 if cap is None else cap
        opt = capi.PileupCallOptions(min_depth, min_count, min_pct, 0)
        d_len = self._alloc(1, self.torch.int64)
        while True:
            d_seq = self._alloc(max(cap, 1), self.torch.uint8)
            check(lib.lrm_pileup_polish_dev(self.pileup, C.byref(opt), first, count, d_seq.data_ptr() if cap else None, cap, d_len.data_ptr(),
                                            self._stream()), "lrm_pileup_polish_dev")
            total = int(d_len.cpu()[0])
            if total <= cap:
                break
            cap = total
        return d_seq[:total].cpu().numpy()

    def pileup_site_alleles(self, sites, min_depth=0, min_count=0, min_pct=0):
        """The inserted allele of every record of a site table of this accumulator (pileup_sites()) -> PILEUP_INS_ALLELE_DT
        records (lrm_pileup_site_alleles_dev): n_col0, len, flags (INS_ENTERS, INS_FULL) and the len bases."""
        assert self.pileup is not None
        sites = np.ascontiguousarray(sites, dtype=capi.PILEUP_SITE_DT)
        n = len(sites)
        opt = capi.PileupCallOptions(min_depth, min_count, min_pct, 0)
        d_sites = self._record_tensor(max(n, 1), capi.PILEUP_SITE_DT, self.torch.int32)
        if n:
            d_sites[:n].copy_(self.torch.from_numpy(sites.view(np.int32).reshape(n, -1)))
        d_out = self._record_tensor(max(n, 1), capi.PILEUP_INS_ALLELE_DT, self.torch.int32)
        check(lib.lrm_pileup_site_alleles_dev(self.pileup, C.byref(opt), d_sites.data_ptr(), n, d_out.data_ptr(), self._stream()),
              "lrm_pileup_site_alleles_dev")
        return _records(d_out[:n], capi.PILEUP_INS_ALLELE_DT)

    def pileup_variants(self, first=None, count=None, cap=None, min_depth=0, min_count=0, min_pct=0, hom_pct=0):
        """The variant stage over the accumulator (lrm_pileup_variants_dev; docs/GACT_SPEC.md, "Pileup variants and VCF") on
        window positions first .. first + count - 1 (default: the whole window) -> (variants, total): PILEUP_VARIANT_DT
        records in ascending position, DEL before SNV before INS -- adjacent deleted positions merged into one record, the
        inserted allele inside the INS record (pileup_ins_cols), gt 2 where the alternative reaches hom_pct (0: 70) percent of
        the depth.  What textio.write_vcf takes.  cap as for pileup_sites(): a table that did not fit is asked for once more."""
        assert self.pileup is not None
        first, count = self._pileup_range(first, count)
        cap = min(3 * count, 4096 + count // 256) if cap is None else cap
        opt = capi.PileupVariantOptions(capi.PileupCallOptions(min_depth, min_count, min_pct, 0), hom_pct, (0, 0, 0))
        d_total = self._alloc(1, self.torch.int64)
        while True:
            d_vars = self._record_tensor(max(cap, 1), capi.PILEUP_VARIANT_DT, self.torch.int32)
            check(lib.lrm_pileup_variants_dev(self.pileup, C.byref(opt), first, count, d_vars.data_ptr() if cap else None, cap, d_total.data_ptr(),
                                              self._stream()), "lrm_pileup_variants_dev")
            total = int(d_total.cpu()[0])
            if total <= cap:
                break
            cap = total
        return _records(d_vars[:total], capi.PILEUP_VARIANT_DT), total

    def pileup_reset(self):
        assert self.pileup is not None
        check(lib.lrm_pileup_reset(self.pileup, self._stream()), "lrm_pileup_reset")

    def pileup_bytes(self):
        return int(lib.lrm_pileup_bytes(self.pileup)) if self.pileup is not None else 0

    def _extend(self, d_reads, d_lens, n):
        args = (self.index.handle, self.ws, d_reads.data_ptr(), d_reads.stride(0), d_lens.data_ptr(), n, self.max_len,
                self.best.data_ptr(), capi.GactParams(*self.gact), self.store.data_ptr(), self.store_stride, self.n_ops.data_ptr(),
                self.score.data_ptr(), self.meta.data_ptr(), self.meta_r.data_ptr())
        if self.clip_on:
            check(lib.lrm_extend_batch_clipped_dev(*args, self.anchor.data_ptr(), self.anchor_min_len, self.clip_penalty,
                                                   self.clip_end_bonus, self.clip.data_ptr(), self._stream()),
                  "lrm_extend_batch_clipped_dev")
        elif self.anchored:
            check(lib.lrm_extend_batch_anchored_dev(*args, self.anchor.data_ptr(), self.anchor_min_len, self._stream()),
                  "lrm_extend_batch_anchored_dev")
        else:
            check(lib.lrm_extend_batch_dev(*args, self._stream()), "lrm_extend_batch_dev")

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
            raise capi.failure("lrm_split_batch_dev", rc=rc, n_seg=int(k.value))
        return self.n_seg

    def rival(self, d_lens, n, min_hits=0, ratio_pct=0):
        """lrm_rival_dev right behind seed() (mapq=True) -> the (n, 3) int64 device tensor of the rival entries."""
        assert self.mapq is not None
        out = self._record_tensor(max(n, 1), ENTRY_DT, self.torch.int64)
        check(lib.lrm_rival_dev(self.index.handle, self.ws, d_lens.data_ptr(), n, capi.Params(n, self.seed_len, self.thres),
                                self.best.data_ptr(), self.mapq.data_ptr(), min_hits, ratio_pct, out.data_ptr(), self._stream()),
              "lrm_rival_dev")
        return out[:n]

    def secondary(self, d_reads, d_lens, n=None, as_sequenced=False):
        """lrm_secondary_batch_dev after seed() and extend() on the same stream -> number of candidates (the call waits for
        that count).  as_sequenced: extend() has not run on d_reads (no duplicate test).  More than sec_cap raise LrmError
        with .rc == -3 and .n_sec."""
        assert self.sec is not None
        n = d_reads.shape[0] if n is None else n
        k = C.c_uint64()
        meta, meta_r = (None, None) if as_sequenced else (self.meta.data_ptr(), self.meta_r.data_ptr())
        rc = lib.lrm_secondary_batch_dev(self.index.handle, self.ws, d_reads.data_ptr(), d_reads.stride(0), d_lens.data_ptr(), n,
                                         self.best.data_ptr(), self.mapq.data_ptr(), meta, meta_r,
                                         capi.Params(n, self.seed_len, self.thres), capi.GactParams(*self.gact), C.byref(self.sec_opt),
                                         C.byref(self.sec_dev), C.byref(k), self._stream())
        self.n_sec = int(k.value) if rc >= 0 else 0
        if rc < 0:
            raise capi.failure("lrm_secondary_batch_dev", rc=rc, n_sec=int(k.value))
        return self.n_sec

    def secondary_results(self):
        """The outputs of the last secondary() as numpy arrays: table (SECONDARY_DT), rows, lens, rival, ops, n_ops, score,
        meta, meta_r and, in the anchored modes, anchor / clip."""
        k = self.n_sec
        h = {"ops" if name == "store" else name: t[:k].cpu().numpy() for name, t in self.sec.items()}
        for name, dt in (("table", SECONDARY_DT), ("rival", ENTRY_DT), ("meta", META_DT), ("anchor", ANCHOR_DT), ("clip", CLIP_DT)):
            if name in h:
                h[name] = h[name].reshape(-1).view(dt)
        h["lens"] = h["lens"].view(np.uint32)
        return h

    def seg_timing(self):
        """timing() of the segment workspace (the split stage's own kernels are in the revcomp_kernel slot)."""
        return _timing(self.ws_seg or self.ws, self._stream())

    def split_results(self):
        """The outputs of the last split() as numpy arrays (same keys as split_batch, `ops` in rows)."""
        k, g = self.n_seg, self.seg
        h = {"ops" if name == "store" else name: t[:k].cpu().numpy() for name, t in g.items()}
        for name, dt in (("seg", SEGMENT_DT), ("best", ENTRY_DT), ("meta", META_DT), ("anchor", ANCHOR_DT), ("clip", CLIP_DT)):
            h[name] = h[name].reshape(-1).view(dt)
        h["lens"] = h["lens"].view(np.uint32)
        return dict(h, is_text=False)

    def stats(self):
        st = capi.Stats()
        check(lib.lrm_workspace_stats(self.ws, C.byref(st), self._stream()), "lrm_workspace_stats")
        return {name: int(getattr(st, name)) for name, _ in capi.Stats._fields_}

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
        return _timing(self.ws, self._stream())

    def results(self, n):
        """Copy the outputs of the last seed+extend to numpy (host).  With md=True the summary stage runs too (the events are
        sized by its records), so "summary" is among the keys whether summary=True was given or not; the events themselves
        come from diff_records(n)."""
        res = dict(best=_records(self.best[:n], ENTRY_DT), ops=self.store[:n].cpu().numpy(), n_ops=self.n_ops[:n].cpu().numpy(),
                   score=self.score[:n].cpu().numpy(), meta=_records(self.meta[:n], META_DT), meta_r=self.meta_r[:n].cpu().numpy())
        if self.anchored:
            res["anchor"] = _records(self.anchor[:n], ANCHOR_DT)
        if self.clip_on:
            res["clip"] = _records(self.clip[:n], CLIP_DT)
        if self.split_on:
            res["split"] = self.split_results()
        if self.mapq is not None:
            res["mapq"] = self.mapq_records(n)
        if self.summary is not None:
            res["summary"] = self.summary_records(n)
        return res

    def close(self):
        if getattr(self, "pileup", None):
            lib.lrm_pileup_free(self.pileup)
            self.pileup = None
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
