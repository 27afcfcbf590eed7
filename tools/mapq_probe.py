"""Probe (run on the GPU box): what the mapping-quality stage costs (docs/GACT_SPEC.md, "Mapping quality").  The bench
workload (ONT reads on an E. coli-sized text with planted repeat families), HBM-resident through DeviceMapper with launch
timing: the seed stage without the stage and with it, a warm-up and REPEATS timed repeats each.  The stage's kernel is
booked into the decide slot, so its time is the difference of that slot; the total of the seed stage is printed next to it.
Printed per Gbp of reads: mean, min and max over the repeats.  Then the distribution of the records.
    python tools/mapq_probe.py          PROBE_READS / PROBE_LEN / PROBE_REF scale it down, PROBE_REPEATS (default 5)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longreadmapper_amd import index, mapper, synth

REPEATS = int(os.environ.get("PROBE_REPEATS", "5"))
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
decide, recs = {}, None
for label, on in (("off", False), ("on", True)):
    dm = mapper.DeviceMapper(di, n, length, mapq=on)
    slot, total = [], []
    for rep in range(REPEATS + 1):                          # the first one warms up (and allocates the phase bytes)
        dm.set_timing(rep > 0)
        dm.seed(d_reads, d_lens)
        torch.cuda.synchronize()
        if rep > 0:
            t = dm.timing()
            slot.append(t["decide_kernel"][0] / gbp)
            total.append(sum(ms for ms, _ in t.values()) / gbp)
    decide[label] = slot
    print("  mapq %-3s decide slot %.3f ms per Gbp (min %.3f, max %.3f)   seed stage %.2f ms per Gbp (min %.2f, max %.2f)   workspace %.2f GiB" %
          (label, np.mean(slot), min(slot), max(slot), np.mean(total), min(total), max(total), dm.workspace_bytes() / 2.0**30), flush=True)
    if on:
        recs = dm.mapq_records(n)
    dm.close()
    del dm
diff = [b - a for a, b in zip(decide["off"], decide["on"])]
print("  mapq_vote_kernel: %.3f ms per Gbp (min %.3f, max %.3f over the repeats)" % (np.mean(diff), min(diff), max(diff)))
q = recs["mapq"]
print("  records: mapq 0 %.2f %%, 1-29 %.2f %%, 30-49 %.2f %%, 50-60 %.2f %%; overflow %d; median n1 %d, reads with n2 > 0 %.1f %%" %
      (100.0 * (q == 0).mean(), 100.0 * ((q > 0) & (q < 30)).mean(), 100.0 * ((q >= 30) & (q < 50)).mean(), 100.0 * (q >= 50).mean(),
       int((recs["flags"] & 1).sum()), int(np.median(recs["n1"])), 100.0 * (recs["n2"] > 0).mean()))
di.close()
