"""Probe (run on the GPU box): what the difference events cost (docs/GACT_SPEC.md, "Difference events and MD:Z").  The bench
workload (ONT reads on an E. coli-sized text with planted repeat families) is seeded and extended once through DeviceMapper,
so that its op rows sit in HBM; then aln_diff_kernel alone is timed over them with events on the stream: a warm-up and
REPEATS timed launches, and the same for aln_summary_kernel and the offsets scan.  Printed: ms per Gbp of reads (mean, min,
max) and the achieved bytes per second (one byte of ops and one byte of text read per column, four bytes written per event).
Next to it the revcomp slot of the extension's launch timing; bs_expand is booked together with gact_bs, so its figure comes
from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/md_probe.py), which lists all four.
    python tools/md_probe.py       PROBE_READS / PROBE_LEN / PROBE_REF scale it down, PROBE_REPEATS (default 10)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longreadmapper_amd import index, mapper, synth
from longreadmapper_amd.capi import check, lib

REPEATS = int(os.environ.get("PROBE_REPEATS", "10"))
n = int(os.environ.get("PROBE_READS", "100000"))
length = int(os.environ.get("PROBE_LEN", "10000"))
ref_len = int(os.environ.get("PROBE_REF", "4641652"))
ref = synth.reference(ref_len, seed=1, repeat_frac=0.05, rep_len=300, rep_copies=1000, rep_div=0.05)
hi = index.HostIndex.build([ref], hlen=12)
di = index.DeviceIndex.upload(hi, 0)
r = synth.reads([ref], n, length, synth.ONT, seed=11)
gbp = float(r["lens"].sum()) / 1e9
d_reads = torch.from_numpy(r["reads"]).cuda()
d_lens = torch.from_numpy(r["lens"].astype(np.int32)).cuda()
print("bench workload (ONT %d bp): %d reads, %.3f Gbp, %d timed repeats" % (length, n, gbp, REPEATS), flush=True)
dm = mapper.DeviceMapper(di, n, length, md=True)
dm.seed(d_reads, d_lens)
dm.set_timing(True)
dm.extend(d_reads, d_lens)                                   # (runs the stages once: the warm-up)
torch.cuda.synchronize()
t = dm.timing()
n_ops = dm.n_ops[:n].cpu().numpy()
cols = int(n_ops[n_ops > 0].sum())
off, ev = dm.diff_records(n)
total = int(off[n])
s = dm.summary_records(n)
tcols = int((s["n_eq"].astype(np.int64) + s["n_x"] + s["n_del"]).sum())
print("  op rows in HBM: %.3f G columns (%.3f per read base), %.3f G target bases, %.3f G events (%.3f per column); revcomp slot of "
      "this extension %.3f ms per Gbp" % (cols / 1e9, cols / 1e9 / gbp, tcols / 1e9, total / 1e9, total / max(cols, 1),
                                          t["revcomp_kernel"][0] / gbp), flush=True)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(what, moved, call):
    ms = []
    for rep in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print("  %s: %.3f ms per Gbp (min %.3f, max %.3f over the repeats); %.0f GB/s at the fastest" %
          (what, np.mean(ms) / gbp, min(ms) / gbp, max(ms) / gbp, moved / (min(ms) * 1e-3) / 1e9), flush=True)


timed("aln_diff_kernel", cols + tcols + 4 * total + 52 * n,   # ops and text in, events out, per read three words, the locus and two offsets
      lambda: check(lib.lrm_aln_diff_dev(di.handle, dm.store.data_ptr(), dm.store_stride, dm.n_ops.data_ptr(), dm.score.data_ptr(),
                                         dm.meta_r.data_ptr(), dm.meta.data_ptr(), n, dm.diff_off.data_ptr(), total,
                                         dm.diff_events.data_ptr(), stream), "lrm_aln_diff_dev"))
timed("aln_summary_kernel", cols + 44 * n,
      lambda: check(lib.lrm_aln_summary_dev(di.handle, dm.store.data_ptr(), dm.store_stride, dm.n_ops.data_ptr(), dm.score.data_ptr(),
                                            dm.meta_r.data_ptr(), n, dm.summary.data_ptr(), stream), "lrm_aln_summary_dev"))
timed("aln_diff_offsets_kernel", 40 * n,
      lambda: check(lib.lrm_aln_diff_offsets_dev(dm.summary.data_ptr(), n, dm.diff_off.data_ptr(), stream), "lrm_aln_diff_offsets_dev"))
off2, ev2 = dm.diff_records(n)
mapped = (dm.meta_r[:n].cpu().numpy() != 0) & (dm.score[:n].cpu().numpy() != -1)
print("  events: %d mapped reads; the repeats wrote the same %d words: %s; kinds X / D-open / D-more: %s" %
      (int(mapped.sum()), total, bool(np.array_equal(ev, ev2) and np.array_equal(off, off2)),
       np.bincount((ev >> 8) & 3, minlength=3).tolist()))
dm.close()
di.close()
