#!/usr/bin/env python3
"""bench.py -- aligned Gbp/s of the seed-and-extend hot path on MI355X.

A step = one pass of the hot path (lrm_seed_batch_dev + lrm_extend_batch_dev) over one batch
of synthetic reads that already sits in HBM.  Default workload = BASELINE.json configs[1]:
E. coli K-12 sized reference (4,641,652 bp, synthetic -- no FASTA on the box), 100k x 10 kbp
ONT-profile reads, seed_len 20, thres 300 (reference defaults), GACT T=320 O=120 W=128.

  python bench.py --gpus N --steps K --warmup W        (N>1: launched under torch.distributed.run)

A plain run does what the headline figure needs and nothing else: index and reads, W warm-up steps, K timed steps, then
rank 0 prints ONE JSON line on stdout (metric, value, unit, ms_per_step, higher_is_better, dtype, the workload in `config`,
the index build and the average time of every kernel inside the timed steps).  --full runs every other leg after the timed
steps and adds its figures to the same line, short enough for a log tail (compact_record(): the figures below without the
per-kernel tables, the per-leg details and the notes); --record FILE writes the whole record of either kind of run:
  value / value_hbm_resident   HBM-resident rate of the timed steps (the contract's `value`; every run)
  value_pcie_inclusive         SURVEY 8(d)'s metric: the same batches through the drop-in boundary on CALLER buffers --
                               H2D of the reads and D2H of every result inside the timed region; details in
                               `pcie_inclusive`: batches in flight (lrm_map_batch_submit / _wait), one call at a time
                               (lrm_map_batch), dense / row result layout, pinned / pageable buffers, and the host CPU
                               seconds the process spent per Gbp
  roofline         dominant kernel of a SERIALIZED replay of the same steps on one stream (every kernel has the
                   chip to itself: kernel time <= step time).  `frac` = bytes the DEVICE layout must move / time / 8 TB/s
                   (counted by the counting build of the seed kernel), `traffic_frac` = the bytes really moved (64-byte
                   lines, committed PMC passes), `random_line_rate` = L2 misses per second against the measured ceiling
                   of independent random 64-byte lines (tools/randline_bench.hip), `reference_work_rate` = the
                   reference layout's algorithmic bytes per second -- a rate of reference work, not a
                   fraction of anything
  cpu_baseline     the CPU oracle on a bounded sample of the same reads: all host cores and 1 thread
                   (the reference's own configuration: both pragmas are commented out, alnmain.c:327-328); the GPU's
                   results on that sample, and those of every PCIe-inclusive leg, are asserted equal to the oracle's
  grch38           the same measurement on the north-star configuration (GRCh38-sized text, 3.1 Gbp, 100 k x 10 kbp ONT
                   reads per step, one GPU) from a fresh child process, when the host has the memory for the index build
  kernels / isolated.kernels   per-kernel tables of the timed (overlapped) region and of the replay

--dump-outputs DIR writes what the last timed step handed its caller as DIR/<name>.npy (dump_outputs()): the workload is
seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import gc
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ECOLI_N = 4_641_652
CHR1_N = 248_956_422
GRCH38_N = 3_099_750_718    # GRCh38 primary assembly incl. unplaced scaffolds (no FASTA on the box: synthetic of this size)
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
RANDOM_LINES_PER_S = 50.4e9  # independent random 64-byte lines per second over a 64 GiB buffer, whatever the loads in
                             # flight per lane or the occupancy (tools/randline_bench.hip, profiles/r3/probes/randline_bench.jsonl)


def log(*a):
    print("[bench]", *a, file=sys.stderr, flush=True)


def usable_cpus():
    """CPUs this process may actually use: affinity mask, capped by the cgroup CPU quota (a GPU box hands a job a
    share of its host, e.g. 16 of 256 hardware threads; more OpenMP threads than that only get throttled)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return max(1, n)


def peak_rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6


def process_cpu_s():
    u = resource.getrusage(resource.RUSAGE_SELF)      # every thread of this process, user + system
    return u.ru_utime + u.ru_stime


def host_gb_available():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                gb = int(line.split()[1]) / 1e6
                break
        else:
            return 0.0
        for p in ("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"):
            try:
                v = open(p).read().strip()
                if v != "max":
                    used = 0
                    for q in ("/sys/fs/cgroup/memory.current", "/sys/fs/cgroup/memory/memory.usage_in_bytes"):
                        try:
                            used = int(open(q).read())
                            break
                        except OSError:
                            pass
                    gb = min(gb, (int(v) - used) / 1e9)
                break
            except OSError:
                pass
        return gb
    except OSError:
        return 0.0


def load_pmc_summary(args, n, Lr):
    """HBM traffic per kernel from the committed rocprofv3 PMC passes of THIS workload (profiles/rNN/
    pmc_summary.json, made by profiles/collect.sh + summarize_pmc.py); None for any other workload."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_summary.json")))
    if not files:
        return None, None
    try:
        d = json.load(open(files[-1]))
        w = d["workload"]
        if (w["reads_per_gpu"], w["read_len"], w["seed_len"], w["thres"]) != (n, Lr, args.seed_len, args.thres):
            return None, None
        if args.ref_len != ECOLI_N or args.profile != "ont":
            return None, None
        return d["kernels"], os.path.relpath(files[-1], ROOT)
    except Exception:
        return None, None


DUMP_BYTES = 64_000_000      # --dump-outputs writes at most this much


def dump_plan(n, stride, store_stride):
    """The reads --dump-outputs keeps: (those whose per-read fields are written, those whose op bytes and read rows are).
    Every read where the budget allows it, else a fixed seeded sample in ascending order."""
    rng = np.random.default_rng(0)

    def pick(k):
        return np.arange(n) if k >= n else np.sort(rng.choice(n, size=k, replace=False))
    return pick(DUMP_BYTES // 5 // (12 * 8)), pick(DUMP_BYTES * 3 // 4 // (4 * (stride + store_stride)))


def write_outputs(path, arrays):
    """DIR/<name>.npy: one-byte fields as float32, wider integers as float64; every value must survive that format."""
    os.makedirs(path, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        f = a.astype(np.float32 if a.dtype.itemsize == 1 else np.float64)
        assert np.array_equal(f.astype(a.dtype), a), "%s does not fit %s" % (name, f.dtype)
        np.save(os.path.join(path, name + ".npy"), f)
        total += f.nbytes
    assert total <= DUMP_BYTES
    return total


def dump_outputs(path, slot, n):
    """What the step that just ran on `slot` handed its caller (lrm_seed_batch_dev + lrm_extend_batch_dev): best[], score,
    n_ops, meta_r and meta (loc, off, seq_id, strand) of the reads in read_index; the op bytes (zero past n_ops: those bytes
    are not part of the result) and the batch rows as extend left them (reverse-strand reads reverse-complemented) of the
    reads in row_index."""
    import torch
    from longreadmapper_amd import mapper
    dm, reads = slot["dm"], slot["reads"]
    sel, rows = dump_plan(n, reads.shape[1], dm.store_stride)

    def take(t, idx):
        return t.index_select(0, torch.from_numpy(idx).to(t.device)).cpu().numpy()
    meta = take(dm.meta, sel).reshape(-1).view(mapper.META_DT)
    ops = take(dm.store, rows)
    ops[np.arange(ops.shape[1])[None, :] >= take(dm.n_ops, rows)[:, None]] = 0
    return write_outputs(path, dict(
        read_index=sel, row_index=rows, best=take(dm.best, sel), score=take(dm.score, sel), n_ops=take(dm.n_ops, sel),
        meta_r=take(dm.meta_r, sel), ops=ops, reads=take(reads, rows),
        meta=np.stack([meta["loc"].astype(np.int64), meta["off"].astype(np.int64), meta["seq_id"].astype(np.int64),
                       meta["strand"].astype(np.int64)], axis=1)))


def compact_record(out):
    """The stdout line: the figures of the full record without per-kernel tables, per-leg details and notes, so that the
    whole line fits a log tail (tests/test_bench_record.py holds it under 6 KB)."""
    def pick(d, *keys):
        return {k: d[k] for k in keys if k in d} if d else None
    c = pick(out, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
             "vs_baseline", "dtype", "data", "value_hbm_resident", "value_pcie_inclusive", "config", "streams",
             "speedup_vs_cpu", "speedup_pcie_inclusive_vs_cpu", "child_wall_s")
    c["roofline"] = pick(out.get("roofline"), "kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_frac",
                         "avg_launch_ms", "gcups")
    cpu = out.get("cpu_baseline")
    c["cpu_baseline"] = pick(cpu, "value", "unit", "cores", "kind")
    if cpu and "one_thread" in cpu:
        c["cpu_baseline"]["one_thread"] = cpu["one_thread"]["value"]
    pc = out.get("pcie_inclusive")
    if pc:
        c["pcie_inclusive"] = dict(steps=pc["steps"], **{k: v["value"] for k, v in pc.items() if isinstance(v, dict) and "value" in v})
    if out.get("kernels"):
        c["kernel_avg_ms"] = {k: v["avg_ms"] for k, v in out["kernels"].items()}
    c["isolated"] = pick(out.get("isolated"), "ms_per_step", "value", "kernel_ms_per_step")
    c["index"] = pick(out.get("index"), "rows", "image_bytes", "build_s", "host_cpus", "peak_rss_gb")
    g = out.get("grch38")
    if g:
        c["grch38"] = compact_record(g) if "value" in g else {k: str(v)[-400:] for k, v in g.items()}
    return c


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, run every other leg: serialized replay and roofline, request counts, "
                         "PCIe-inclusive legs, CPU baseline with its comparison against the GPU's results, GRCh38-sized "
                         "child run (minutes; the options marked --full choose among them)")
    ap.add_argument("--ref-len", type=int, default=ECOLI_N)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--profile", default="ont", choices=["ont", "pacbio", "clean"])
    ap.add_argument("--seed-len", type=int, default=20)
    ap.add_argument("--thres", type=int, default=300)
    ap.add_argument("--gact", default="320,120,128")
    ap.add_argument("--no-isolated-replay", action="store_true",
                    help="--full: skip the serialized replay of the steps on one stream that `roofline` is taken from")
    ap.add_argument("--no-pcie", action="store_true", help="--full: skip the PCIe-inclusive legs through the host-buffer boundary")
    ap.add_argument("--pcie-steps", type=int, default=0, help="--full: batches of every PCIe-inclusive leg (default: min(steps, 10))")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("LRM_BENCH_STREAMS", "3")),
                    help="HIP streams the steps alternate over (each with its own workspace); >1 overlaps the "
                         "HBM-latency-bound seed kernels of one step with the VALU-bound extension of another")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="--full: target CPU-baseline time (0: only the sample the results are checked on)")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--no-grch38", action="store_true",
                    help="--full: do not run the GRCh38-sized leg in a child process after the default workload")
    ap.add_argument("--grch38-timeout", type=float, default=400.0, help="--full: seconds after which that child is killed")
    ap.add_argument("--record", metavar="FILE",
                    help="write the whole record (with --full: per-kernel tables, every PCIe leg, notes) as JSON to FILE")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (float32 / float64, at most 64 MB; see dump_outputs)")
    ap.add_argument("--sa-sampled", type=int, default=0, help="lrm_index_options.sa_sampled (0: full suffix array)")
    return ap.parse_args(argv)


def main():
    args = parse_args()

    # OpenMP (index builder, staging copies, the CPU oracle) must not spawn one thread per hardware thread of the
    # host when the job only owns a share of it (cgroup quota): oversubscribed threads are throttled
    # (and the ranks of one node share that share)
    os.environ.setdefault("OMP_NUM_THREADS", str(max(1, usable_cpus() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))))))

    t_start = time.time()
    import torch
    import torch.distributed as tdist
    from longreadmapper_amd import dist, index, mapper, synth

    rank, world, local = dist.init_process_group()
    assert world == args.gpus, "WORLD_SIZE %d != --gpus %d (launch N>1 with torch.distributed.run)" % (world, args.gpus)
    assert torch.cuda.is_available(), "bench.py needs a GPU: the product has no CPU path"
    if os.environ.get("LRM_BENCH_ONE_DEVICE"):      # rehearsal: several ranks share cuda:0 (with LRM_DIST_BACKEND=gloo)
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    gact = tuple(int(x) for x in args.gact.split(","))
    prof = {"ont": synth.ONT, "pacbio": synth.PACBIO_CLR, "clean": synth.CLEAN}[args.profile]
    iopts = dict(sa_sampled=args.sa_sampled) if args.sa_sampled else {}

    # ---- index: built on the CPU by rank 0, one RCCL broadcast of the device image -----------------
    t0 = time.time()
    ref = synth.reference(args.ref_len, seed=1, repeat_frac=0.05, rep_len=300, rep_copies=1000, rep_div=0.05)
    hi = None
    blob = None
    t_synth = time.time() - t0
    t_build = t_pack = 0.0
    if rank == 0:
        t1 = time.time()
        hi = index.HostIndex.build([ref], names=["synth_ref"], o_ratio=32, hlen=12)
        t_build = time.time() - t1
        t1 = time.time()
        blob = hi.pack_device(local, **iopts)          # packed piece by piece straight into HBM: no host copy of the image
        torch.cuda.synchronize()
        t_pack = time.time() - t1
        log("index: N=%d L=%d: reference %.1fs, built in %.1fs, image %.2f GiB packed+uploaded in %.1fs"
            % (args.ref_len, hi.length, t_synth, t_build, blob.numel() / 2**30, t_pack))
    t1 = time.time()
    blob = dist.broadcast_blob(blob, device=dev, src=0)
    torch.cuda.synchronize()
    t_bcast = time.time() - t1
    t1 = time.time()
    di = index.DeviceIndex.adopt(blob, local)          # derives the planar text and the seed tables on the device
    di_tables = di.tables()
    di_tables["derive_s"] = round(time.time() - t1, 2)
    if rank == 0:
        log("derived tables: %s" % di_tables)

    def index_record():
        return dict(rows=hi.length, image_bytes=int(blob.numel()), reference_s=round(t_synth, 1), build_s=round(t_build, 1),
                    pack_upload_s=round(t_pack, 1), broadcast_s=round(t_bcast, 3),
                    host_cpus=usable_cpus(), peak_rss_gb=round(peak_rss_gb(), 1), tables=di_tables)

    # ---- reads: every rank maps its own batch (weak scaling), resident in HBM ----------------------
    n, Lr = args.reads, args.read_len
    r = synth.reads([ref], n, Lr, prof, seed=11 + 1000 * rank)
    pristine = torch.from_numpy(r["reads"]).to(dev)
    d_lens = torch.from_numpy(r["lens"].astype(np.int32)).to(dev)
    nstreams = max(1, args.streams)
    slots = []
    for k in range(nstreams):
        slots.append(dict(reads=torch.empty_like(pristine),
                          dm=mapper.DeviceMapper(di, n, Lr, args.seed_len, args.thres, gact, device=local),
                          stream=torch.cuda.Stream(device=dev) if nstreams > 1 else torch.cuda.current_stream(dev)))
    dm, d_reads = slots[0]["dm"], slots[0]["reads"]
    bases = int(r["lens"].sum())
    if rank == 0:
        log("reads: %d x %d (%s), workspace %.2f GiB" % (n, Lr, args.profile, dm.workspace_bytes() / 2**30))

    step_no = [0]

    def step():
        sl = slots[step_no[0] % nstreams]
        step_no[0] += 1
        with torch.cuda.stream(sl["stream"]):
            sl["reads"].copy_(pristine)      # extend rev-comps reverse-strand reads in place: restore the batch
            sl["dm"].seed(sl["reads"], d_lens)
            sl["dm"].extend(sl["reads"], d_lens)

    def barrier():
        if world > 1:
            tdist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        t = torch.tensor([x], dtype=torch.float64, device=dev if tdist.is_initialized() and tdist.get_backend() == "nccl" else "cpu")
        if world > 1:
            tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
        return float(t.item())

    for _ in range(args.warmup):
        step()
    barrier()
    if not args.no_kernel_timing:
        for sl in slots:
            sl["dm"].set_timing(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, slots[(step_no[0] - 1) % nstreams], n)
        log("outputs of the last timed step: %.1f MB under %s" % (dumped / 1e6, args.dump_outputs))
    ktimes = {}
    if not args.no_kernel_timing:
        for sl in slots:
            with torch.cuda.stream(sl["stream"]):
                for name, (ms, launches) in sl["dm"].timing().items():
                    a = ktimes.get(name, (0.0, 0))
                    ktimes[name] = (a[0] + ms, a[1] + launches)
            sl["dm"].set_timing(False)
    elapsed = max_over_ranks(elapsed)
    total_bases = bases * world * args.steps
    workload = "%s synthetic reference (%d bp, 5%% planted repeats), %d x %d bp %s-profile reads per GPU" \
               % ({ECOLI_N: "E. coli K-12 sized", CHR1_N: "human chr1 sized", GRCH38_N: "GRCh38 sized"}.get(args.ref_len, "custom"),
                  args.ref_len, n, Lr, args.profile)
    value = total_bases / elapsed / 1e9
    out = dict(metric="aligned Gbp/sec", value=value, unit="Gbp/s", n_gpus=world,
               steps=args.steps, warmup=args.warmup, ms_per_step=elapsed / args.steps * 1e3,
               higher_is_better=True, scaling="weak", vs_baseline=None, dtype="u8/u64 integer", data="synthetic",
               value_hbm_resident=value,
               config=dict(workload=workload,
                           seed_len=args.seed_len, thres=args.thres, gact_T=gact[0], gact_O=gact[1], gact_W=gact[2],
                           reads_per_gpu=n, read_len=Lr, streams=nstreams, sa_sampled=args.sa_sampled or 1,
                           parallelism="reads sharded, index replicated (1 RCCL bcast)"),
               streams=nstreams)

    def emit():
        if args.record:
            os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
            with open(args.record, "w") as f:
                json.dump(out, f)
        print(json.dumps(compact_record(out)), flush=True)
        if world > 1:
            tdist.barrier()

    if not args.full:
        # a plain run ends here: the headline figure and what the timed steps themselves left behind
        if rank != 0:
            tdist.barrier()
            return
        out.update(kernels={name: dict(ms_total=round(ms, 3), launches=launches, avg_ms=round(ms / launches, 4))
                            for name, (ms, launches) in ktimes.items() if launches},
                   index=index_record())
        emit()
        return

    # serialized replay of the same steps on ONE stream: per-kernel durations without the other streams' kernels
    # sharing the chip (the timed region above is what `value` comes from, the replay what `roofline` comes from)
    ktimes_iso = {}
    iso_wall = None
    if not args.no_isolated_replay and not args.no_kernel_timing and rank == 0:
        torch.cuda.synchronize()
        slots[0]["dm"].set_timing(True)
        ti = time.perf_counter()
        for _ in range(args.steps):
            with torch.cuda.stream(slots[0]["stream"]):
                slots[0]["reads"].copy_(pristine)
                slots[0]["dm"].seed(slots[0]["reads"], d_lens)
                slots[0]["dm"].extend(slots[0]["reads"], d_lens)
        torch.cuda.synchronize()
        iso_wall = time.perf_counter() - ti
        with torch.cuda.stream(slots[0]["stream"]):
            ktimes_iso = slots[0]["dm"].timing()
        slots[0]["dm"].set_timing(False)
    # the memory requests the DEVICE layout makes (counting build of the seed kernel, outside every timed region)
    dev_counts = None
    if rank == 0:
        with torch.cuda.stream(slots[0]["stream"]):
            slots[0]["reads"].copy_(pristine)
            slots[0]["dm"].set_counting(True)
            slots[0]["dm"].seed(slots[0]["reads"], d_lens)
            dev_counts = slots[0]["dm"].stats()
            slots[0]["dm"].set_counting(False)
            slots[0]["dm"].seed(slots[0]["reads"], d_lens)         # leaves best[] of the product kernel for the checks below
            slots[0]["dm"].extend(slots[0]["reads"], d_lens)
        torch.cuda.synchronize()
    stats = dm.stats()
    full = dm.results(n) if rank == 0 else None

    # ---- the same batch through the drop-in boundary on caller buffers (H2D + D2H timed) ----------
    pcie = None
    if not args.no_pcie:
        # the device-resident slots are no longer needed: their HBM goes back before the host path allocates its own
        for sl in slots[1:]:
            sl["dm"].close()
        del slots[1:]
        torch.cuda.empty_cache()
        ps = args.pcie_steps or min(args.steps, 10)
        stride = r["reads"].shape[1]
        sstride = (2 * Lr + 15) // 16 * 16
        NB = 3                                       # caller buffer sets: two batches on the device, one queued
        pcie = dict(steps=ps, note="every leg: H2D of the reads and D2H of every result (best[], scores, loci, op bytes, "
                                   "reverse-complemented reads) inside the timed region; the caller's own batch load (copying "
                                   "the reads into the buffer) is untimed")

        def leg(kind, layout, inflight):
            dense = layout != "rows"
            if kind == "pinned":
                bufs = [(mapper.pinned_empty((n, stride)), mapper.pinned_empty((n, sstride))) for _ in range(NB if inflight > 1 else 1)]
            else:
                bufs = [(np.empty((n, stride), dtype=np.uint8), np.empty((n, sstride), dtype=np.uint8)) for _ in range(NB if inflight > 1 else 1)]
            keep = layout.endswith("+keep_reads")
            layout = layout.split("+")[0]
            opts = dict(cigar_text=1) if layout == "text" else dict(dense_results=1) if dense else {}
            if keep:
                opts["keep_reads"] = 1
            for hr, hs in bufs:
                hs[:] = 0
                hr[:] = r["reads"]
            # warm-up: device mirrors, workspaces, both slots
            w = [mapper.map_batch_submit(di, hr, r["lens"], args.seed_len, args.thres, gact, store=hs, options=opts) for hr, hs in bufs]
            res = [x.wait() for x in w][0]
            res = dict(best=res["best"].copy(), score=res["score"].copy(), n_ops=res["n_ops"].copy(), layout=layout, keep_reads=keep,
                       ops0=[mapper.text_of(res, i) if layout == "text" else mapper.ops_of(res, i) for i in range(min(n, 64))],
                       reads0=bufs[0][0][:64].copy())
            for hr, hs in bufs:
                hr[:] = r["reads"]                                                             # untimed: the caller's batch load
            barrier()
            if inflight == 1:
                # one call at a time (submit + wait == lrm_map_batch): the batch is restored before every call, untimed
                wall = cpu = 0.0
                for s in range(ps):
                    hr, hs = bufs[0]
                    hr[:] = r["reads"]
                    barrier()
                    c0, t1 = process_cpu_s(), time.perf_counter()
                    mapper.map_batch_submit(di, hr, r["lens"], args.seed_len, args.thres, gact, store=hs, options=opts).wait()
                    barrier()
                    wall += time.perf_counter() - t1
                    cpu += process_cpu_s() - c0
            else:
                # batches in flight: the buffers are re-used as they come back.  Reads of a buffer that has been through a
                # batch are partly reverse-complemented; mapping them again is the same work -- restoring 1 GB per batch
                # inside the loop would time the host's memcpy, not the path.
                c0, t1 = process_cpu_s(), time.perf_counter()
                pend = []
                for s in range(ps):
                    hr, hs = bufs[s % len(bufs)]
                    pend.append(mapper.map_batch_submit(di, hr, r["lens"], args.seed_len, args.thres, gact, store=hs, options=opts))
                    if len(pend) >= inflight:
                        pend.pop(0).wait()
                while pend:
                    pend.pop(0).wait()
                barrier()
                wall, cpu = time.perf_counter() - t1, process_cpu_s() - c0
            wall = max_over_ranks(wall)
            out = dict(value=bases * world * ps / wall / 1e9, unit="Gbp/s", ms_per_batch=wall / ps * 1e3,
                       host_cpu_s_per_Gbp=cpu / (bases * ps / 1e9), buffers=kind, result_layout=layout,
                       batches_submitted_ahead=inflight)
            if kind == "pinned":
                for hr, hs in bufs:
                    mapper.pinned_free(hr)
                    mapper.pinned_free(hs)
            del bufs
            return out, res

        legs = [("in_flight_dense_pinned", "pinned", "dense", 3), ("in_flight_text_pinned", "pinned", "text", 3),
                ("in_flight_dense_pinned_keep_reads", "pinned", "dense+keep_reads", 3),
                ("in_flight_text_pinned_keep_reads", "pinned", "text+keep_reads", 3),
                ("one_call_dense_pinned", "pinned", "dense", 1), ("one_call_rows_pinned", "pinned", "rows", 1),
                ("one_call_rows_pageable", "pageable", "rows", 1), ("in_flight_rows_pageable", "pageable", "rows", 3)]
        pcie_res = {}
        for name, kind, layout, infl in legs:
            pcie[name], pcie_res[name] = leg(kind, layout, infl)
            if rank == 0:
                log("pcie leg %-26s %6.2f Gbp/s  %6.1f ms per batch  host CPU %.3f s per Gbp"
                    % (name, pcie[name]["value"], pcie[name]["ms_per_batch"], pcie[name]["host_cpu_s_per_Gbp"]))
        pcie["value"] = pcie["in_flight_dense_pinned"]["value"]
        pcie["unit"] = "Gbp/s"
        pcie["value_leg"] = ("in_flight_dense_pinned: lrm_map_batch_submit / lrm_map_batch_wait, two batches on the device and one "
                             "queued, dense result layout DMA'd into pinned caller memory")
        pcie["host_cpu_s_per_Gbp"] = pcie["in_flight_dense_pinned"]["host_cpu_s_per_Gbp"]
        pcie["text_layout_note"] = ("in_flight_text_pinned hands back the run-length CIGAR TEXT parse_cigar would print from the op bytes "
                                    "(lrm_map_options.cigar_text: the run-length pass runs on the device, ~0.45 instead of 1.1 bytes per read "
                                    "base come down) -- another result format, so it is reported next to the headline, not as it")
        pcie["keep_reads_note"] = ("the *_keep_reads legs set lrm_map_options.keep_reads: the caller's reads stay as they are (the reference "
                                   "reverse-complements reverse-strand reads in place, alnmain.c:437; here those copies stay on the device) -- "
                                   "0.5 bytes per read base less come down and the host places nothing; an opt-in deviation from the reference's "
                                   "side effect, reported next to the headline, not as it")
        pcie["bytes_per_batch"] = dict(h2d=int(n * stride + 4 * n), d2h_reads="reverse-strand rows only (~half of n x read_len)",
                                       d2h_ops="used op bytes (16-byte aligned per read)", d2h_small=int(n * 60))
        pcie["inversion_r2"] = ("BENCH_r02 had pinned (15.97) below pageable (16.90): the result scatter was on the call's critical "
                                "path and a memcpy into hipHostMalloc'd (mapped) memory runs at 127 GB/s against 149 into pageable "
                                "memory, 23 against 31 single-threaded reading it (profiles/r3/probes/hostlink_bench_1.jsonl); the "
                                "dense layout removes that scatter")

    if rank != 0:
        if world > 1:
            tdist.barrier()
        return

    # ---- sanity of the measured batch (cheap, outside the timed region) ----------------------------
    res = {k: (v[:min(n, 2000)] if hasattr(v, "__len__") else v) for k, v in full.items()}
    mapped = int(((res["meta_r"] == 1) & (res["score"] >= 0)).sum())
    truth_ok = 0
    for i in range(len(res["score"])):
        if res["meta_r"][i] and abs(int(res["meta"]["off"][i]) - int(r["pos"][i])) < 300 \
                and int(res["meta"]["strand"][i]) == int(r["strand"][i]):
            truth_ok += 1
    log("sanity: %d/%d mapped, %d within 300 bp of the true locus, median ED %.0f"
        % (mapped, len(res["score"]), truth_ok, float(np.median(res["score"]))))

    # ---- CPU baseline: the oracle (CPU restatement), all host cores, bounded sample ----------------
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc
    oi = orc.OracleIndex.from_host_index(hi)
    cores = min(orc.lib.orc_max_threads(), usable_cpus())          # rank 0 alone runs the CPU baseline
    cpu = None
    per_base = None
    sample_n = min(n, 4 * cores)
    rs = np.ascontiguousarray(r["reads"][:sample_n]).copy()
    tc = time.perf_counter()
    best, _, ct_seed = oi.seed_batch(rs, r["lens"][:sample_n], args.seed_len, args.thres, nthreads=cores, counters=True)
    ext = oi.extend_batch(rs, r["lens"][:sample_n], best, gact, nthreads=cores, counters=True)
    probe = time.perf_counter() - tc
    if args.cpu_seconds > 0:
        want = int(min(n, max(sample_n, sample_n * args.cpu_seconds / max(probe, 1e-3))))
        if want > sample_n:
            sample_n = want
            rs = np.ascontiguousarray(r["reads"][:sample_n]).copy()
            tc = time.perf_counter()
            best, _, ct_seed = oi.seed_batch(rs, r["lens"][:sample_n], args.seed_len, args.thres, nthreads=cores,
                                             counters=True)
            ext = oi.extend_batch(rs, r["lens"][:sample_n], best, gact, nthreads=cores, counters=True)
            probe = time.perf_counter() - tc
    sample_bases = int(r["lens"][:sample_n].sum())
    cpu = dict(value=sample_bases / probe / 1e9, unit="Gbp/s", cores=cores, kind="port",
               sample="first %d reads of the batch (%d bases), seed+extend, %.1f s wall, OpenMP dynamic over reads"
                      % (sample_n, sample_bases, probe))
    if args.cpu_seconds > 0:
        # one thread: the reference's own configuration (both parallel pragmas are commented out, alnmain.c:327-328)
        n1 = max(1, min(sample_n, int(sample_n * (args.cpu_seconds * 0.6) / max(probe * cores, 1e-3))))
        r1 = np.ascontiguousarray(r["reads"][:n1]).copy()
        tc = time.perf_counter()
        b1, _ = oi.seed_batch(r1, r["lens"][:n1], args.seed_len, args.thres, nthreads=1)
        oi.extend_batch(r1, r["lens"][:n1], b1, gact, nthreads=1)
        t1c = time.perf_counter() - tc
        b1n = int(r["lens"][:n1].sum())
        cpu["one_thread"] = dict(value=b1n / t1c / 1e9, unit="Gbp/s", cores=1,
                                 sample="first %d reads (%d bases), seed+extend, %.1f s wall" % (n1, b1n, t1c))
    # the oracle's output on the sample must equal the GPU's (same reads: the first sample_n of rank 0)
    assert np.array_equal(full["best"][:sample_n], best), "GPU best[] differs from the CPU oracle on the bench batch"
    assert np.array_equal(full["score"][:sample_n], ext["score"]), "GPU scores differ from the CPU oracle"
    assert np.array_equal(full["n_ops"][:sample_n], ext["n_ops"]), "GPU CIGAR lengths differ from the CPU oracle"
    if pcie:                                     # ... and so must the results that came back through the host boundary, in every mode
        for name, pr in pcie_res.items():
            assert np.array_equal(pr["best"], full["best"]) and np.array_equal(pr["score"], full["score"]) \
                and np.array_equal(pr["n_ops"], full["n_ops"]), "host boundary (%s) and the device-resident path disagree" % name
            assert np.array_equal(pr["best"][:sample_n], best) and np.array_equal(pr["score"][:sample_n], ext["score"])
            k0 = min(64, sample_n)
            for i in range(k0):
                want_ops = bytes(ext["ops"][i, :int(ext["n_ops"][i])])
                if pr["layout"] == "text":
                    none = not want_ops or ext["meta_r"][i] == 0 or ext["score"][i] == -1
                    assert pr["ops0"][i].decode() == ("*" if none else orc.parse_cigar(want_ops)), "host boundary (%s): CIGAR text differs from the oracle's" % name
                else:
                    assert pr["ops0"][i] == want_ops, "host boundary (%s): op bytes differ from the oracle" % name
            if pr["keep_reads"]:
                assert np.array_equal(pr["reads0"][:k0], r["reads"][:k0]), "host boundary (%s): keep_reads changed the caller's reads" % name
            else:
                assert np.array_equal(pr["reads0"][:k0], rs[:k0]), "host boundary (%s): reads not reverse-complemented like the oracle's" % name
        pcie["checked"] = ("every leg: best[], score, n_ops of all %d reads equal the device-resident path, the first %d equal the CPU "
                           "oracle; op bytes and reverse-complemented reads of the first %d reads equal the oracle's" % (n, sample_n, min(64, sample_n)))
    # algorithmic bytes per read base, counted exactly on the sample
    ce = ext["counters"]
    per_base = dict(
        seed_search=(16 * ct_seed.n_lc + 8 * ct_seed.n_occ + ct_seed.bwt_bytes) / sample_bases,
        vote=(8 * ct_seed.n_sa) / sample_bases,
        pack2bit=1.0,
        gact=(2 * sample_bases + int(ce.cigar_ops) + 32 * sample_n) / sample_bases,
        cells=int(ce.cells) / sample_bases,
        seeds=ct_seed.n_seeds / sample_bases,
    )
    # bytes the DEVICE layout must move per read base: seed_search = one 8-byte table entry per lookup + 16 bytes per rank
    # request (counting build, whole batch) + the 2-bit read (0.25 B per base and phase round) + 12 bytes per survivor
    # record written; vote = 8 bytes per SA row + the survivor records read back + 48 bytes per (read, phase) result
    dev_per_base = None
    if dev_counts and dev_counts["seeds_evaluated"]:
        dev_per_base = dict(
            seed_search=(8 * dev_counts["seed_table_lookups"] + 16 * dev_counts["seed_rank_requests"]) / bases + 0.25,
            seeds=dev_counts["seeds_evaluated"] / bases,
            table_lookups_per_seed=dev_counts["seed_table_lookups"] / dev_counts["seeds_evaluated"],
            rank_requests_per_seed=dev_counts["seed_rank_requests"] / dev_counts["seeds_evaluated"],
            vote=per_base["vote"] + 48.0 * (args.seed_len + 1) / Lr,
        )
        if di_tables.get("seed_table_len") == args.seed_len:
            # unique seeds come out of the seed table with their text position: their SA rows are not gathered, so the
            # reference's "8 B per SA hit" is an UPPER bound on what the vote kernels must move on this handle
            dev_per_base["vote_is_upper_bound"] = True

    # ---- per-kernel table and the roofline of the dominant kernel ----------------------------------
    # reference-layout algorithmic bytes per read base per kernel family; device-layout bytes next to them
    alg_of = {"pack2bit_kernel": per_base["pack2bit"], "seed_search_kernel": per_base["seed_search"],
              "gact_kernel": per_base["gact"], "gact_bs_kernel": per_base["gact"], "bs_pack_reads_kernel": 1.25}
    dev_of = {"pack2bit_kernel": 1.25, "gact_kernel": per_base["gact"], "gact_bs_kernel": per_base["gact"], "bs_pack_reads_kernel": 1.25}
    if dev_per_base:
        dev_of["seed_search_kernel"] = dev_per_base["seed_search"]
        if not dev_per_base.get("vote_is_upper_bound"):
            dev_of["vote_kernel"] = dev_per_base["vote"]
    pmc, pmc_file = load_pmc_summary(args, n, Lr)

    def kernel_table(ktimes):
        kernels, dominant = {}, None
        for name, (ms, launches) in ktimes.items():
            if launches == 0:
                continue
            alg = alg_of.get(name, per_base["vote"] if name.startswith("vote") else None)
            devb = dev_of.get(name)
            avg_ms = ms / launches
            per_launch = lambda b: b * bases * args.steps / launches if b else None
            k = dict(ms_total=round(ms, 3), launches=launches, avg_ms=round(avg_ms, 4),
                     device_bytes_per_launch=per_launch(devb), reference_bytes_per_launch=per_launch(alg))
            pk = pmc.get(name.replace("gact_kernel", "gact3_kernel")) if pmc else None
            if pk:
                k["traffic_bytes_per_launch"] = (pk["fetch_bytes"] + pk["write_bytes"]) / pk["launches_per_step"]
                if pk.get("l2_hit") is not None and (pk["l2_hit"] + pk["l2_miss"]) > 0:
                    k["l2_hit_rate"] = pk["l2_hit"] / (pk["l2_hit"] + pk["l2_miss"])
                    k["l2_misses_per_launch"] = pk["l2_miss"] / pk["launches_per_step"]
                if pk.get("valu_insts"):
                    k["valu_wave_insts_per_launch"] = pk["valu_insts"] / pk["launches_per_step"]
            kernels[name] = k
            if dominant is None or ms > ktimes[dominant][0]:
                dominant = name
        return kernels, dominant

    def roofline_of(kernels, ktimes, name):
        k = kernels[name]
        sec = k["avg_ms"] * 1e-3
        devb = k["device_bytes_per_launch"]
        ach = devb / sec / 1e9 if devb else None
        # frac: bytes the device layout MUST move / time / peak.  Every counted request is a request the kernel made, so
        # frac <= traffic_frac <= 1 by construction (a request moves at least its own bytes).
        rr = dict(kernel=name, bound="hbm", achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=(ach / HBM_PEAK_GBS) if ach else None,
                  traffic=k.get("traffic_bytes_per_launch"), avg_launch_ms=k["avg_ms"], device_bytes_per_launch=devb,
                  achieved_definition="bytes the device layout must move per launch (counting build: 8 B per seed-table lookup, "
                                      "16 B per rank request, 8 B per SA row) / average launch time of the serialized replay")
        if rr["traffic"]:
            rr["traffic_frac"] = rr["traffic"] / sec / 1e9 / HBM_PEAK_GBS      # bytes really moved (64-byte lines) vs the HBM peak
        if k.get("l2_misses_per_launch"):
            rate = k["l2_misses_per_launch"] / sec
            rr["random_line_rate"] = dict(achieved=rate, ceiling=RANDOM_LINES_PER_S, frac=rate / RANDOM_LINES_PER_S, unit="64-byte lines/s",
                                          note="L2 misses per second (committed PMC pass) against the rate of independent random "
                                               "64-byte lines this memory system delivers (tools/randline_bench.hip: 50.4 G/s over "
                                               "64 GiB, 56 G/s inside the Infinity Cache, whatever the loads in flight)")
        if k["reference_bytes_per_launch"]:
            rr["reference_work_rate"] = dict(value=k["reference_bytes_per_launch"] / sec / 1e9, unit="GB/s of reference-layout bytes",
                                             note="SURVEY 8(d)'s algorithmic bytes (16 B per lc lookup, 8 B + the scanned bwt bytes per "
                                                  "_occ_access, from the oracle's exact counters) per second: a rate of REFERENCE work -- "
                                                  "the device answers several of those accesses with one request, so this is not a "
                                                  "fraction of the device's bandwidth and has no peak")
        if "valu_wave_insts_per_launch" in k:
            # integer VALU issue: one wave64 instruction per 4 cycles per SIMD, 1024 SIMDs, 2.4 GHz peak clock
            peak_ips = 1024 * 2.4e9 / 4
            rr["valu_issue_frac"] = k["valu_wave_insts_per_launch"] / sec / peak_ips
        if name in ("gact_kernel", "gact_bs_kernel"):
            rr["gcups"] = per_base["cells"] * bases * args.steps / (ktimes[name][0] * 1e-3) / 1e9
            rr["note"] = ("integer DP (gact): bound by VALU issue, not by HBM or MFMA -- its HBM fraction is small by "
                          "construction (%.1f B/base, %.0f cells/base); see valu_issue_frac / gcups"
                          % (per_base["gact"], per_base["cells"]))
            if "valu_issue_frac" in rr:
                # The roofline this kernel really has: integer vector-instruction issue (no matrix work, 3 bytes per base of HBM
                # traffic).  `bound` steps outside the contract's hbm|mfma on purpose -- neither is what limits a bit-sliced
                # integer DP -- and the HBM figures stay next to it under hbm_*.
                rr.update(hbm_achieved=rr["achieved"], hbm_peak=rr["peak"], hbm_frac=rr["frac"], hbm_unit=rr["unit"],
                          bound="valu", achieved=k["valu_wave_insts_per_launch"] / sec / 1e9, peak=1024 * 2.4 / 4,
                          unit="G wave64 instructions/s", frac=rr["valu_issue_frac"],
                          achieved_definition="vector wave-instructions per launch (committed rocprofv3 --pmc pass, SQ_INSTS_VALU) / average "
                                              "launch time of the serialized replay; peak = 1024 SIMDs x 2.4 GHz / 4 cycles per wave64 instruction")
        return rr

    kernels, dominant = kernel_table(ktimes)
    traffic_note = ("`traffic`, L2 misses and VALU instruction counts per launch come from the committed rocprofv3 --pmc passes of this "
                    "workload (%s), not from this run; null for other workloads" % (pmc_file or "none for this workload"))
    isolated = None
    if ktimes_iso:
        # the roofline comes from the serialized replay: every kernel has the chip to itself, so kernel time <= step time
        k_iso, dom_iso = kernel_table(ktimes_iso)
        roofline = roofline_of(k_iso, ktimes_iso, dom_iso)
        roofline["source"] = ("serialized replay of the same %d steps on ONE stream right after the timed region (HIP events on "
                              "that stream); the timed region itself overlaps steps on %d streams" % (args.steps, nstreams))
        roofline["traffic_source"] = traffic_note
        roofline_hbm = roofline_of(k_iso, ktimes_iso, "seed_search_kernel") if "seed_search_kernel" in k_iso else None
        isolated = dict(note="serialized replay: per-kernel durations without kernels of other steps sharing the chip",
                        ms_per_step=iso_wall / args.steps * 1e3, value=bases * args.steps / iso_wall / 1e9,
                        kernel_ms_per_step=sum(v["ms_total"] for v in k_iso.values()) / args.steps,
                        roofline_gact=roofline_of(k_iso, ktimes_iso, "gact_bs_kernel") if "gact_bs_kernel" in k_iso else None,
                        roofline_vote=roofline_of(k_iso, ktimes_iso, "vote_kernel") if "vote_kernel" in k_iso else None,
                        kernels=k_iso)
    else:
        roofline = roofline_of(kernels, ktimes, dominant) if dominant else None
        roofline_hbm = roofline_of(kernels, ktimes, "seed_search_kernel") if "seed_search_kernel" in kernels else None
        if roofline and nstreams > 1:
            roofline["source"] = ("timed region, steps alternating over %d HIP streams: durations include the time a kernel "
                                  "shared the chip with kernels of other steps" % nstreams)
    out.update(value_pcie_inclusive=pcie["value"] if pcie else None,
               roofline=roofline, roofline_hbm_kernel=roofline_hbm, cpu_baseline=cpu, pcie_inclusive=pcie,
               value_note="`value` = `value_hbm_resident`: the batch is in device memory when the timed region starts (the contract's "
                          "definition); SURVEY 8(d)'s metric with H2D of reads and D2H of results timed is `value_pcie_inclusive` "
                          "(details in `pcie_inclusive`)",
               kernels=kernels, isolated=isolated,
               algorithmic_bytes_per_base=dict(reference_layout=per_base, device_layout=dev_per_base), stats=stats,
               index=index_record(),
               speedup_vs_cpu=value / cpu["value"],
               speedup_pcie_inclusive_vs_cpu=(pcie["value"] / cpu["value"]) if pcie else None)

    # ---- the north-star configuration in a fresh child process (GRCh38-sized text on this one GPU) ----------------
    if world == 1 and not args.no_grch38 and args.ref_len == ECOLI_N:
        avail = host_gb_available()
        spent = time.time() - t_start
        if avail < 110:
            out["grch38"] = dict(skipped="host memory: %.0f GB available, the index build of the 6.2 G-row text peaks at 93 GB" % avail)
        elif spent > 170:
            out["grch38"] = dict(skipped="time guard: the default workload took %.0f s" % spent)
        else:
            # everything this process holds on the device and in host RAM goes back first
            dm.close()
            di.close()
            del slots, dm, di, blob, pristine, d_lens, d_reads, hi, oi, full, r, rs, ref
            gc.collect()
            torch.cuda.empty_cache()
            tmp = tempfile.TemporaryDirectory()
            child_record = os.path.join(tmp.name, "grch38.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--full", "--no-grch38", "--ref-len", str(GRCH38_N), "--steps", "10", "--warmup", "3",
                   "--pcie-steps", "6", "--cpu-seconds", "6", "--reads", str(args.reads), "--read-len", str(args.read_len),
                   "--seed-len", str(args.seed_len), "--thres", str(args.thres), "--gact", args.gact, "--record", child_record]
            tg = time.time()
            pr = None
            try:
                pr = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.grch38_timeout)
                if pr.returncode == 0 and os.path.exists(child_record):
                    with open(child_record) as f:
                        g = json.load(f)
                    for k in ("kernels", "isolated", "algorithmic_bytes_per_base"):       # the per-kernel tables stay in the child's own record
                        if k == "isolated" and g.get(k):
                            g[k] = dict(ms_per_step=g[k]["ms_per_step"], value=g[k]["value"], kernel_ms_per_step=g[k]["kernel_ms_per_step"],
                                        kernel_avg_ms={kn: kv["avg_ms"] for kn, kv in g[k]["kernels"].items()})
                        elif k == "kernels":
                            g.pop(k, None)
                    g["child_wall_s"] = round(time.time() - tg, 1)
                    out["grch38"] = g
                else:
                    out["grch38"] = dict(failed="child exit code %d" % pr.returncode, stderr_tail=pr.stderr[-1500:])
            except subprocess.TimeoutExpired:
                out["grch38"] = dict(failed="child exceeded %.0f s" % args.grch38_timeout)
            for l in (pr.stderr.splitlines()[-12:] if pr is not None else []):
                if l.startswith("[bench]"):
                    log("grch38 child:", l[8:])
            tmp.cleanup()
    emit()


if __name__ == "__main__":
    main()
