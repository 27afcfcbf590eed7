"""Probe (run on the GPU box): what the alignment summary stage costs (docs/GACT_SPEC.md, "Alignment summary and PAF").  The
bench workload (ONT reads on an E. coli-sized text with planted repeat families) is seeded and extended once through
DeviceMapper, so that its op rows sit in HBM; then aln_summary_kernel alone is timed over them with events on the stream: a
warm-up and REPEATS timed launches.  Printed: ms per Gbp of reads (mean, min, max) and the achieved bytes per second (one
byte read per column, 32 bytes written per read).  Next to it the revcomp slot of the extension's launch timing, the other
stream kernel the workspace books on its own; bs_expand is booked together with gact_bs, so its figure comes from a kernel
trace of this script (rocprofv3 --kernel-trace --stats -- python tools/summary_probe.py), which lists all three.
    python tools/summary_probe.py       PROBE_READS / PROBE_LEN / PROBE_REF scale it down, PROBE_REPEATS (default 10)"""
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
dm = mapper.DeviceMapper(di, n, length, summary=True)
dm.seed(d_reads, d_lens)
dm.set_timing(True)
dm.extend(d_reads, d_lens)                                   # (runs the stage once: the warm-up)
torch.cuda.synchronize()
t = dm.timing()
n_ops = dm.n_ops[:n].cpu().numpy()
cols = int(n_ops[n_ops > 0].sum())
print("  op rows in HBM: %.3f G columns (%.3f per read base); revcomp slot of this extension %.3f ms per Gbp" %
      (cols / 1e9, cols / 1e9 / gbp, t["revcomp_kernel"][0] / gbp), flush=True)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ms = []
for rep in range(REPEATS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.lrm_aln_summary_dev(di.handle, dm.store.data_ptr(), dm.store_stride, dm.n_ops.data_ptr(), dm.score.data_ptr(),
                                  dm.meta_r.data_ptr(), n, dm.summary.data_ptr(), stream), "lrm_aln_summary_dev")
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
moved = cols + 32 * n + 12 * n                               # op bytes in, records out, the three words per read the rule reads
print("  aln_summary_kernel: %.3f ms per Gbp (min %.3f, max %.3f over the repeats); %.0f GB/s at the fastest" %
      (np.mean(ms) / gbp, min(ms) / gbp, max(ms) / gbp, moved / (min(ms) * 1e-3) / 1e9))
s = dm.summary_records(n)
mapped = (dm.meta_r[:n].cpu().numpy() != 0) & (dm.score[:n].cpu().numpy() != -1)
nm = s["n_x"].astype(np.int64) + s["n_ins"] + s["n_del"]
print("  records: %d mapped reads; NM == score for %d of them; identity %.4f, gap opens per kbp %.2f" %
      (int(mapped.sum()), int((nm[mapped] == dm.score[:n].cpu().numpy()[mapped]).sum()),
       float(s["n_eq"][mapped].sum()) / max(float((s["n_eq"] + s["n_x"] + s["n_ins"] + s["n_del"])[mapped].sum()), 1.0),
       1e3 * float((s["ins_runs"] + s["del_runs"])[mapped].sum()) / max(float(r["lens"][mapped].sum()), 1.0)))
dm.close()
di.close()
