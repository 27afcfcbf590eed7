"""Probe (run on the GPU box): what the secondary-alignment stage costs (docs/GACT_SPEC.md, "Secondary alignments").  The
bench workload (ONT reads on an E. coli-sized text with planted repeat families), HBM-resident through DeviceMapper with
launch timing, a warm-up and REPEATS timed repeats of everything.  In one run:
  mapq_vote       the decide slot of the seed stage with the mapping-quality stage minus the slot without it (the yardstick)
  rival_locus     lrm_rival_dev alone (it is the only kernel of the call, booked into the decide slot), with the default
                  thresholds -- few reads are candidates -- and with every read that has a rival forced to be one
                  (min_hits = 1, ratio_pct = 1)
  the stage       lrm_secondary_batch_dev behind seed + extension (classic), with both settings of the thresholds: all its
                  launches, per candidate where there are candidates, and the wall time of the call (it waits for the count)
Printed per Gbp of reads: mean, min and max over the repeats.
    python tools/secondary_probe.py     PROBE_READS / PROBE_LEN / PROBE_REF scale it down, PROBE_REPEATS (default 5)"""
import os
import sys
import time

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


def show(label, xs, tail=""):
    print("  %-34s %8.3f ms per Gbp (min %.3f, max %.3f)%s" % (label, np.mean(xs), min(xs), max(xs), tail), flush=True)


def decide_slot(dm, call):
    """The decide slot of REPEATS timed repeats of call(), per Gbp (the first repeat warms up and allocates) -> (times, last result)."""
    slot, res = [], None
    for rep in range(REPEATS + 1):
        dm.set_timing(rep > 0)
        res = call()
        torch.cuda.synchronize()
        if rep > 0:
            slot.append(dm.timing()["decide_kernel"][0] / gbp)
    return slot, res


def kernels():
    dm = mapper.DeviceMapper(di, n, length, mapq=False)
    try:
        off, _ = decide_slot(dm, lambda: dm.seed(d_reads, d_lens))
    finally:
        dm.close()
    dm = mapper.DeviceMapper(di, n, length, mapq=True)
    try:
        on, _ = decide_slot(dm, lambda: dm.seed(d_reads, d_lens))
        show("mapq_vote (decide slot, on - off)", [b - a for a, b in zip(off, on)])
        # the survivor lists of the batch are in dm's workspace
        for label, H, pct in (("rival_locus, default thresholds", 0, 0), ("rival_locus, every rival a candidate", 1, 1)):
            slot, e = decide_slot(dm, lambda: dm.rival(d_lens, n, H, pct))
            cand = int((e[:, 1] != 0).sum().item())
            show(label, slot, "   %d candidates of %d reads (%.2f %%)" % (cand, n, 100.0 * cand / n))
    finally:
        dm.close()


def stage(label, H, pct):
    ds = mapper.DeviceMapper(di, n, length, mapq=True, secondary=True, sec_min_hits=H, sec_ratio_pct=pct)
    try:
        total, wall, k = [], [], 0
        for rep in range(REPEATS + 1):
            back = d_reads.clone()                          # the extension turns reverse-strand reads round in place
            ds.set_timing(False)
            ds.seed(back, d_lens)
            ds.extend(back, d_lens)
            torch.cuda.synchronize()
            ds.set_timing(rep > 0)
            t0 = time.perf_counter()
            k = ds.secondary(back, d_lens)
            torch.cuda.synchronize()
            if rep > 0:
                wall.append((time.perf_counter() - t0) * 1e3)
                total.append(sum(ms for ms, _ in ds.timing().values()))
        flags = ds.secondary_results()["table"]["flags"]
        print("  the stage, classic extension, %s: %d candidates, %d reported, %d duplicates; kernels %.3f ms (min %.3f, max %.3f)%s; "
              "wall %.3f ms with launch timing on" %
              (label, k, int((flags & 1 != 0).sum()), int((flags & 2 != 0).sum()), np.mean(total), min(total), max(total),
               " = %.2f us per candidate" % (1e3 * np.mean(total) / k) if k else "", np.mean(wall)), flush=True)
    finally:
        ds.close()


try:
    kernels()
    stage("default thresholds", 0, 0)
    stage("every rival a candidate", 1, 1)
finally:
    di.close()
