"""Probe (run on the GPU box): what the anchored extension mode costs.  The bench workload (ONT reads on an E. coli-sized
text) and a PacBio-CLR workload, HBM-resident through DeviceMapper with launch timing: classic vs anchored vs anchored with
end clipping (its kernel is recorded in the extension kernel's slot, next to the stitch), a warm-up and three timed
repeats each, ms per kernel slot (mean, and the spread of the per-repeat totals), and the median ED / len.
The last leg is the split stage (lrm_split_batch_dev): the bench workload with PROBE_CHIMERAS (default 0.05) of its reads
turned into chimeras (the second 40 % of the read replaced by the start of another read), per-slot times of the segment
workspace -- compact_count / scan / mark / gather, split_flag in the revcomp slot, seed and extension of the segment batch in
theirs -- and the wall time of the call, which holds the stage's one host wait.
    python tools/anchored_probe.py          PROBE_READS / PROBE_LEN / PROBE_REF scale it down"""
import time
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longreadmapper_amd import index, mapper, synth

REPEATS = 3
n = int(os.environ.get("PROBE_READS", "100000"))
ref_len = int(os.environ.get("PROBE_REF", "4641652"))
ref = synth.reference(ref_len, seed=1, repeat_frac=0.05, rep_len=300, rep_copies=1000, rep_div=0.05)
hi = index.HostIndex.build([ref], hlen=12)
di = index.DeviceIndex.upload(hi, 0)
for name, profile, length, count in (("bench workload (ONT 10 kbp)", synth.ONT, int(os.environ.get("PROBE_LEN", "10000")), n),
                                     ("PacBio CLR 15 kbp", synth.PACBIO_CLR, 15000, max(n // 5, 1))):
    r = synth.reads([ref], count, length, profile, seed=11)
    d_lens = torch.from_numpy(r["lens"].astype(np.int32)).cuda()
    print("%s: %d reads, %.2f Gbp" % (name, count, float(r["lens"].sum()) / 1e9), flush=True)
    for label, anchored, clip in (("classic", False, False), ("anchored", True, False), ("anch+clip", True, True)):
        dm = mapper.DeviceMapper(di, count, length, anchored=anchored, clip=clip)
        per_slot, totals = {}, []
        for rep in range(REPEATS + 1):                      # the first one warms up (and allocates the mode's scratch)
            d_reads = torch.from_numpy(r["reads"]).cuda()   # the extension reverse-complements in place: a fresh copy
            dm.seed(d_reads, d_lens)
            torch.cuda.synchronize()
            dm.set_timing(rep > 0)
            dm.extend(d_reads, d_lens)
            torch.cuda.synchronize()
            if rep > 0:
                t = dm.timing()
                totals.append(sum(ms for ms, _ in t.values()))
                for k, (ms, launches) in t.items():
                    if launches:
                        per_slot[k] = per_slot.get(k, 0.0) + ms / REPEATS
        res = dm.results(count)
        ok = res["score"] >= 0
        print("  %-9s extension %.2f ms (min %.2f, max %.2f)  median ED/len %.4f  workspace %.2f GiB" %
              (label, np.mean(totals), min(totals), max(totals),
               float(np.median(res["score"][ok] / r["lens"][ok])), dm.workspace_bytes() / 2.0**30))
        print("           " + "  ".join("%s %.2f" % (k.replace("_kernel", ""), v) for k, v in per_slot.items()), flush=True)
        dm.close()
        del dm
# split stage: a stated fraction of chimeras in the bench workload
frac = float(os.environ.get("PROBE_CHIMERAS", "0.05"))
length = int(os.environ.get("PROBE_LEN", "10000"))
r = synth.reads([ref], n, length, synth.ONT, seed=11)
rng = np.random.default_rng(5)
chim = np.flatnonzero(rng.random(n) < frac)
reads = r["reads"].copy()
for i in chim:
    j, ln = int(rng.integers(0, n)), int(r["lens"][i])
    cut = ln * 6 // 10
    take = min(ln - cut, int(r["lens"][j]))
    reads[i, cut:cut + take] = r["reads"][j, :take]
d_lens = torch.from_numpy(r["lens"].astype(np.int32)).cuda()
dm = mapper.DeviceMapper(di, n, length, clip=True, split=True, seg_cap=max(4 * len(chim), 1024))
per_slot, walls, segs = {}, [], 0
for rep in range(REPEATS + 1):
    d_reads = torch.from_numpy(reads).cuda()
    dm.seed(d_reads, d_lens)
    dm.extend(d_reads, d_lens)
    torch.cuda.synchronize()
    lib_ws = dm.ws_seg
    mapper.check(mapper.lib.lrm_workspace_set_timing(lib_ws, int(rep > 0)), "lrm_workspace_set_timing")
    t0 = time.perf_counter()
    segs = dm.split(d_reads, d_lens)
    torch.cuda.synchronize()
    if rep > 0:
        walls.append((time.perf_counter() - t0) * 1e3)
        for k, (ms, launches) in dm.seg_timing().items():
            if launches:
                per_slot[k] = per_slot.get(k, 0.0) + ms / REPEATS
sp = dm.results(n)["split"]
print("split stage: %d reads (%.2f Gbp), %d chimeras, %d segments, %d reported; call %.2f ms wall (min %.2f, max %.2f)" %
      (n, float(r["lens"].sum()) / 1e9, len(chim), segs, int(((sp["seg"]["flags"] & 2) != 0).sum()), np.mean(walls), min(walls), max(walls)))
print("           " + "  ".join("%s %.2f" % (k.replace("_kernel", ""), v) for k, v in per_slot.items()), flush=True)
dm.close()
di.close()
