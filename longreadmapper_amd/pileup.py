"""A pileup accumulator of its own (lrm_pileup; docs/GACT_SPEC.md, "Pileup on the host-buffer path and across replicas"): what the
host-buffer batch calls add to (mapper.map_batch(..., pileup=)), one per replica of a group handle, merged afterwards.
DeviceMapper (device.py) keeps an accumulator of its own behind its pileup_* methods; the read-side methods here take the same
arguments."""
import ctypes as C

import numpy as np

from . import capi
from .capi import check, lib
from .records import PILEUP_COL_DT, PILEUP_INS_ALLELE_DT, PILEUP_SITE_DT, PILEUP_VARIANT_DT

GUARD_WORDS = 16           # behind the counter words of either allocation (lrm_debug_pileup_raw / _ins_raw)


class Pileup:
    """One lrm_pileup over the text positions [lo, hi) with ins_cols insertion columns.

    index_or_replica: a DeviceIndex of one device, or the raw handle lrm_index_replica returned.  replica=r: the accumulator
    of replica r of a group handle (lrm_pileup_create_replica; replica 0 of a group handle is the group handle itself, which
    lrm_pileup_create refuses).  device: the device of that replica; torch allocates the read-side buffers there and the
    calls run on torch's current stream of it."""

    def __init__(self, index_or_replica, lo, hi, ins_cols=0, replica=None, device=0):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.index = index_or_replica          # (kept alive: the accumulator reads the text of its handle)
        handle = getattr(index_or_replica, "handle", index_or_replica)
        self.lo, self.hi, self.ins_cols = int(lo), int(hi), int(ins_cols)
        h = C.c_void_p()
        if replica is None:
            check(lib.lrm_pileup_create_ins(C.byref(h), handle, self.lo, self.hi, self.ins_cols), "lrm_pileup_create_ins")
        else:
            check(lib.lrm_pileup_create_replica(C.byref(h), handle, int(replica), self.lo, self.hi, self.ins_cols), "lrm_pileup_create_replica")
        self.handle = h

    @property
    def width(self):
        return self.hi - self.lo

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _alloc(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device=self.dev)

    def _records(self, rows, dt):
        return self._alloc((max(rows, 1), dt.itemsize // 4), self.torch.int32)

    def _range(self, first, count):
        first = 0 if first is None else first
        return first, (self.width - first if count is None else count)

    @staticmethod
    def _host(t, rows, dt):
        return t[:rows].cpu().numpy().reshape(-1).view(dt)

    # ---- the read side: the arguments of DeviceMapper.pileup_* ----
    def columns(self, first=None, count=None):
        """The PILEUP_COL_DT records of window positions first .. first + count - 1 (default: the whole window)."""
        first, count = self._range(first, count)
        out = self._records(count, PILEUP_COL_DT)
        check(lib.lrm_pileup_read_dev(self.handle, first, count, out.data_ptr(), self._stream()), "lrm_pileup_read_dev")
        return self._host(out, count, PILEUP_COL_DT)

    def sites(self, first=None, count=None, cap=None, min_depth=0, min_count=0, min_pct=0, consensus=False):
        """lrm_pileup_sites_dev -> (sites, total, cons); a table that did not fit is asked for again with cap = total."""
        first, count = self._range(first, count)
        cap = min(count, 4096 + count // 256) if cap is None else cap
        opt = capi.PileupCallOptions(min_depth, min_count, min_pct, 0)
        d_total = self._alloc(1, self.torch.int64)
        d_cons = self._alloc(max(count, 1), self.torch.uint8) if consensus else None
        while True:
            d_sites = self._records(cap, PILEUP_SITE_DT)
            check(lib.lrm_pileup_sites_dev(self.handle, C.byref(opt), first, count, d_sites.data_ptr() if cap else None, cap, d_total.data_ptr(),
                                           d_cons.data_ptr() if consensus else None, self._stream()), "lrm_pileup_sites_dev")
            total = int(d_total.cpu()[0])
            if total <= cap:
                break
            cap = total
        return self._host(d_sites, total, PILEUP_SITE_DT), total, (d_cons[:count].cpu().numpy() if consensus else None)

    def ins_columns(self, first=None, count=None):
        """lrm_pileup_ins_read_dev -> uint32 array of shape (count, K, 4): [position, insertion column, base class A C G T]."""
        first, count = self._range(first, count)
        out = self._alloc((max(count, 1), max(self.ins_cols, 1), 4), self.torch.int32)
        check(lib.lrm_pileup_ins_read_dev(self.handle, first, count, out.data_ptr(), self._stream()), "lrm_pileup_ins_read_dev")
        return out[:count].cpu().numpy().view(np.uint32)

    def polish(self, first=None, count=None, cap=None, min_depth=0, min_count=0, min_pct=0):
        """lrm_pileup_polish_dev -> the polished bytes (uint8); a buffer that was too small is asked for again with cap = the length."""
        first, count = self._range(first, count)
        cap = count + count // 64 + 64 if cap is None else cap
        opt = capi.PileupCallOptions(min_depth, min_count, min_pct, 0)
        d_len = self._alloc(1, self.torch.int64)
        while True:
            d_seq = self._alloc(max(cap, 1), self.torch.uint8)
            check(lib.lrm_pileup_polish_dev(self.handle, C.byref(opt), first, count, d_seq.data_ptr() if cap else None, cap, d_len.data_ptr(),
                                            self._stream()), "lrm_pileup_polish_dev")
            total = int(d_len.cpu()[0])
            if total <= cap:
                break
            cap = total
        return d_seq[:total].cpu().numpy()

    def site_alleles(self, sites, min_depth=0, min_count=0, min_pct=0):
        """lrm_pileup_site_alleles_dev of a site table of this accumulator -> PILEUP_INS_ALLELE_DT records."""
        sites = np.ascontiguousarray(sites, dtype=PILEUP_SITE_DT)
        n = len(sites)
        opt = capi.PileupCallOptions(min_depth, min_count, min_pct, 0)
        d_sites = self._records(n, PILEUP_SITE_DT)
        if n:
            d_sites[:n].copy_(self.torch.from_numpy(sites.view(np.int32).reshape(n, -1)))
        d_out = self._records(n, PILEUP_INS_ALLELE_DT)
        check(lib.lrm_pileup_site_alleles_dev(self.handle, C.byref(opt), d_sites.data_ptr(), n, d_out.data_ptr(), self._stream()),
              "lrm_pileup_site_alleles_dev")
        return self._host(d_out, n, PILEUP_INS_ALLELE_DT)

    def variants(self, first=None, count=None, cap=None, min_depth=0, min_count=0, min_pct=0, hom_pct=0):
        """lrm_pileup_variants_dev -> (variants, total): PILEUP_VARIANT_DT records, deleted runs merged, the inserted allele inside;
        a table that did not fit is asked for again with cap = total."""
        first, count = self._range(first, count)
        cap = min(3 * count, 4096 + count // 256) if cap is None else cap
        opt = capi.PileupVariantOptions(capi.PileupCallOptions(min_depth, min_count, min_pct, 0), hom_pct, (0, 0, 0))
        d_total = self._alloc(1, self.torch.int64)
        while True:
            d_vars = self._records(cap, PILEUP_VARIANT_DT)
            check(lib.lrm_pileup_variants_dev(self.handle, C.byref(opt), first, count, d_vars.data_ptr() if cap else None, cap, d_total.data_ptr(),
                                              self._stream()), "lrm_pileup_variants_dev")
            total = int(d_total.cpu()[0])
            if total <= cap:
                break
            cap = total
        return self._host(d_vars, total, PILEUP_VARIANT_DT), total

    # ---- management ----
    def reset(self):
        check(lib.lrm_pileup_reset(self.handle, self._stream()), "lrm_pileup_reset")

    def bytes(self):
        return int(lib.lrm_pileup_bytes(self.handle))

    def merge(self, other, staged_chunk=None):
        """self += other (lrm_pileup_merge_dev), asynchronous on torch's current stream of this accumulator's device; the batches
        that add to `other` must have been waited for.  staged_chunk (tests): lrm_debug_pileup_merge_staged with chunks of
        that many words."""
        if staged_chunk is None:
            check(lib.lrm_pileup_merge_dev(self.handle, other.handle, self._stream()), "lrm_pileup_merge_dev")
        else:
            check(lib.lrm_debug_pileup_merge_staged(self.handle, other.handle, staged_chunk, self._stream()), "lrm_debug_pileup_merge_staged")

    def raw(self, guard=True):
        """lrm_debug_pileup_raw: the 8 W + 1 counter words [and the 16 guard words behind them] as uint32; waits for the stream."""
        out = np.zeros(8 * self.width + 1 + (GUARD_WORDS if guard else 0), dtype=np.uint32)
        check(lib.lrm_debug_pileup_raw(self.handle, out.ctypes.data, len(out), self._stream()), "lrm_debug_pileup_raw")
        return out

    def ins_raw(self, guard=True):
        """lrm_debug_pileup_ins_raw: the 4 K W insertion words [and the 16 guard words behind them] as uint32."""
        out = np.zeros(4 * self.ins_cols * self.width + (GUARD_WORDS if guard else 0), dtype=np.uint32)
        check(lib.lrm_debug_pileup_ins_raw(self.handle, out.ctypes.data, len(out), self._stream()), "lrm_debug_pileup_ins_raw")
        return out

    def close(self):
        if getattr(self, "handle", None):
            lib.lrm_pileup_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
