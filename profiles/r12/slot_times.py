"""profiles/r12: one side of the measurement -- the library LRM_ACCEL_LIB names, or the tree's.
    python profiles/r12/slot_times.py LABEL        PROBE_READS (default 100000), PROBE_REPEATS (default 5)
The revcomp slot of the anchored extension (with and without end clipping), of the split stage and of the secondary stage on
the bench workload (ONT reads of 10 kbp on the E. coli-sized text), a warm-up and PROBE_REPEATS timed repeats each, every
repeat printed, and one SHA-256 over the results of each leg."""
import hashlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from longreadmapper_amd import index, mapper, synth

REPEATS = int(os.environ.get("PROBE_REPEATS", "5"))
n = int(os.environ.get("PROBE_READS", "100000"))
length = 10000
side = sys.argv[1]
ref = synth.reference(4641652, seed=1, repeat_frac=0.05, rep_len=300, rep_copies=1000, rep_div=0.05)
hi = index.HostIndex.build([ref], hlen=12)
di = index.DeviceIndex.upload(hi, 0)
r = synth.reads([ref], n, length, synth.ONT, seed=11)
d_lens = torch.from_numpy(r["lens"].astype(np.int32)).cuda()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def fields(m):
    return [m[f] for f in ("loc", "off", "seq_id", "strand")]


def show(leg, xs, digest, extra=""):
    print("%-9s %-10s revcomp slot ms: %s | min %.4f med %.4f max %.4f | sha %s %s" %
          (side, leg, " ".join("%.4f" % x for x in xs), min(xs), float(np.median(xs)), max(xs), digest, extra), flush=True)


# anchored extension (anchor_jobs_kernel + the locus reverse complement are its revcomp slot)
for label, clip in (("anchored", False), ("anch+clip", True)):
    dm = mapper.DeviceMapper(di, n, length, anchored=True, clip=clip)
    slot = []
    for rep in range(REPEATS + 1):
        d_reads = torch.from_numpy(r["reads"]).cuda()
        dm.seed(d_reads, d_lens)
        torch.cuda.synchronize()
        dm.set_timing(rep > 0)
        dm.extend(d_reads, d_lens)
        torch.cuda.synchronize()
        if rep > 0:
            slot.append(dm.timing()["revcomp_kernel"][0])
    res = dm.results(n)
    ops = np.concatenate([res["ops"][i, :res["n_ops"][i]] for i in range(0, n, 7)])
    show(label, slot, sha(res["n_ops"], res["score"], res["meta_r"], *fields(res["meta"]), ops, res["anchor"]))
    dm.close()
    del dm, d_reads

# split stage
rng = np.random.default_rng(5)
chim = np.flatnonzero(rng.random(n) < 0.05)
reads = r["reads"].copy()
for i in chim:
    j, ln = int(rng.integers(0, n)), int(r["lens"][i])
    cut = ln * 6 // 10
    take = min(ln - cut, int(r["lens"][j]))
    reads[i, cut:cut + take] = r["reads"][j, :take]
dm = mapper.DeviceMapper(di, n, length, clip=True, split=True, seg_cap=max(4 * len(chim), 1024))
slot, segs = [], 0
for rep in range(REPEATS + 1):
    d_reads = torch.from_numpy(reads).cuda()
    dm.seed(d_reads, d_lens)
    dm.extend(d_reads, d_lens)
    torch.cuda.synchronize()
    mapper.check(mapper.lib.lrm_workspace_set_timing(dm.ws_seg, int(rep > 0)), "lrm_workspace_set_timing")
    segs = dm.split(d_reads, d_lens)
    torch.cuda.synchronize()
    if rep > 0:
        slot.append(dm.seg_timing()["revcomp_kernel"][0])
sp = dm.results(n)["split"]
show("split", slot, sha(*[sp[k] for k in ("seg", "lens", "rows", "best", "n_ops", "score", "meta_r")]), "%d segments" % segs)
dm.close()
del dm, d_reads

# secondary stage, every rival a candidate
d_all = torch.from_numpy(r["reads"]).cuda()
ds = mapper.DeviceMapper(di, n, length, mapq=True, secondary=True, sec_min_hits=1, sec_ratio_pct=1)
slot, k = [], 0
for rep in range(REPEATS + 1):
    back = d_all.clone()
    ds.set_timing(False)
    ds.seed(back, d_lens)
    ds.extend(back, d_lens)
    torch.cuda.synchronize()
    ds.set_timing(rep > 0)
    k = ds.secondary(back, d_lens)
    torch.cuda.synchronize()
    if rep > 0:
        slot.append(ds.timing()["revcomp_kernel"][0])
sr = ds.secondary_results()
show("secondary", slot, sha(*[sr[key] for key in ("table", "rows", "lens", "rival", "n_ops", "score", "meta_r")]), "%d candidates" % k)
ds.close()
di.close()
