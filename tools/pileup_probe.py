"""Probe (run on the GPU box): what the pileup costs (docs/GACT_SPEC.md, "Pileup").  The bench workload (ONT reads on an
E. coli-sized text with planted repeat families) is seeded and extended once through DeviceMapper, so that its op rows sit in
HBM; the window is the whole text.  Then, with events on the stream, a warm-up and REPEATS timed launches each of
pileup_add_kernel, of the read-back of the whole window (tile sums, their scan, the records), and -- as yardsticks of the same
stream shape -- of aln_diff_kernel and aln_summary_kernel; next to the read-back, in the same process, the call stage
(docs/GACT_SPEC.md, "Pileup calls": lrm_pileup_sites_dev over the whole window, with and without the cons bytes) and the bytes
each path would bring down the link, and the variant stage (docs/GACT_SPEC.md, "Pileup variants and VCF": lrm_pileup_variants_dev)
launched in turn with the sites call on the same window.  Printed: ms per Gbp of reads (mean, min, max), the number of
atomic adds of one pileup_add launch (from the accumulator itself) and the adds per second at the fastest launch.  Then the
insertion side (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus"): the add on two plain accumulators
launched in turn (this build's spread against itself; with PROBE_PARENT_LIB also the parent commit's library on accumulators
of its own, in the same process), the add with K = 4 and K = 8 insertion columns, the polish next to the sites + cons bytes,
the site alleles and the insertion read-back.  Last, the host-buffer path (ms per batch with two batches in flight on pinned
buffers with dense results: without an accumulator, with a plain one and with K = 8; PROBE_HOST_BATCHES timed batches a leg) and
the merge of two accumulators over the window on both routes.
    python tools/pileup_probe.py       PROBE_READS / PROBE_LEN / PROBE_REF scale it down, PROBE_REPEATS (default 10),
                                       PROBE_PARENT_LIB=<path of the parent commit's liblrm_accel.so>,
                                       PROBE_UNTIL=variants ends the probe behind the call and variant stages"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longreadmapper_amd import capi, index, mapper, synth
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
window = (0, int(hi.h.con_len))
W = window[1] - window[0]
print("bench workload (ONT %d bp): %d reads, %.3f Gbp, window of %d positions (%.1f MB of counters), %d timed repeats" %
      (length, n, gbp, W, (32 * W + 4) / 1e6, REPEATS), flush=True)
dm = mapper.DeviceMapper(di, n, length, md=True, pileup=window)
dm.seed(d_reads, d_lens)
dm.extend(d_reads, d_lens)                                   # (runs the stages once: the warm-up; the accumulator holds one batch)
torch.cuda.synchronize()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
n_ops = dm.n_ops[:n].cpu().numpy()
cols = int(n_ops[n_ops > 0].sum())
off, ev = dm.diff_records(n)
total = int(off[n])
# the adds of one launch, counted from the accumulator: every event word is the number of adds that hit it, and a covered
# read made two adds to the difference plane
raw = np.zeros(8 * W + 1, dtype=np.uint32)
check(lib.lrm_debug_pileup_raw(dm.pileup, raw.ctypes.data, len(raw), stream), "lrm_debug_pileup_raw")
event_adds = int(raw[W + 1:].astype(np.int64).sum())
covered = int(((dm.meta_r[:n].cpu().numpy() != 0) & (dm.score[:n].cpu().numpy() != -1) & (n_ops > 0)).sum())
adds = event_adds + 2 * covered
print("  op rows in HBM: %.3f G columns; %.3f G 'X' / 'D' events (%.3f per column); one pileup_add launch: %.4f G event adds "
      "(%.4f per column: %s) + 2 x %d depth adds" % (cols / 1e9, total / 1e9, total / max(cols, 1), event_adds / 1e9, event_adds / max(cols, 1),
      ", ".join("%s %.4f G" % (name, raw[W + 1 + k * W:W + 1 + (k + 1) * W].astype(np.int64).sum() / 1e9) for k, name in enumerate(capi.PILEUP_PLANES)),
      covered), flush=True)
hot = raw[W + 1:].max()
print("  the hottest event word took %d adds; mean depth %.1f" % (int(hot), float(np.cumsum(raw[:W].astype(np.int32), dtype=np.int64).mean())), flush=True)
d_out = torch.zeros((W, 8), dtype=torch.int32, device="cuda")


def timed(what, call, per=None):
    call()                                                   # warm-up
    torch.cuda.synchronize()
    ms = []
    for rep in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    tail = "" if per is None else "; %.2f G %s per second at the fastest" % (per[0] / (min(ms) * 1e-3) / 1e9, per[1])
    print("  %s: %.3f ms per Gbp (min %.3f, max %.3f over the repeats; %.3f ms per launch)%s" %
          (what, np.mean(ms) / gbp, min(ms) / gbp, max(ms) / gbp, np.mean(ms), tail), flush=True)
    return ms


def alternated(legs):
    """legs: [(name, call)], launched in turn REPEATS times after one warm-up each -> {name: [ms]}"""
    for _, call in legs:
        call()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for rep in range(REPEATS):
        for name, call in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    for name, _ in legs:
        print("  %s: %.3f ms per Gbp (min %.3f, max %.3f; alternated)" % (name, np.mean(ms[name]) / gbp, min(ms[name]) / gbp, max(ms[name]) / gbp), flush=True)
    return ms


timed("pileup_add_kernel", lambda: check(lib.lrm_pileup_add_dev(
    dm.pileup, d_reads.data_ptr(), d_reads.stride(0), d_lens.data_ptr(), dm.store.data_ptr(), dm.store_stride, dm.n_ops.data_ptr(),
    dm.score.data_ptr(), dm.meta_r.data_ptr(), dm.meta.data_ptr(), n, None, 0, stream), "lrm_pileup_add_dev"), per=(adds, "adds"))
timed("pileup read-back, whole window", lambda: check(lib.lrm_pileup_read_dev(dm.pileup, 0, W, d_out.data_ptr(), stream), "lrm_pileup_read_dev"),
      per=(64 * W, "bytes (32 read, 32 written per position)"))
# the call stage over the same window: the site table and the count word, with and without one cons byte per position
SITE_CAP = 1 << 20
d_sites = torch.zeros((SITE_CAP, 8), dtype=torch.int32, device="cuda")
d_n_sites = torch.zeros(1, dtype=torch.int64, device="cuda")
d_cons = torch.zeros(W, dtype=torch.uint8, device="cuda")
for what, cons in (("pileup calls, whole window, sites only", None), ("pileup calls, whole window, sites + cons bytes", d_cons.data_ptr())):
    timed(what, lambda cons=cons: check(lib.lrm_pileup_sites_dev(dm.pileup, None, 0, W, d_sites.data_ptr(), SITE_CAP, d_n_sites.data_ptr(), cons, stream),
                                        "lrm_pileup_sites_dev"))
n_sites = int(d_n_sites.cpu()[0])
kinds = d_sites[:min(n_sites, SITE_CAP), 7].cpu().numpy().view(np.uint32) >> 24
letters = np.bincount(d_cons.cpu().numpy(), minlength=256)
print("  %d sites under the default options (SNV %d, DEL %d, INS %d; table of %d records); cons letters: %s" %
      (n_sites, int((kinds & 1 != 0).sum()), int((kinds & 2 != 0).sum()), int((kinds & 4 != 0).sum()), SITE_CAP,
       ", ".join("%s %d" % (ch, letters[ord(ch)]) for ch in "ACGTN-")), flush=True)
print("  down the link: the records %.1f MB; the site table %.3f MB + 8 bytes; the cons bytes %.1f MB" %
      (32 * W / 1e6, 32 * min(n_sites, SITE_CAP) / 1e6, W / 1e6), flush=True)
# the variant stage (docs/GACT_SPEC.md, "Pileup variants and VCF") next to the sites call of the same build, in turn, on the same window
VAR_CAP = 1 << 20
d_vars = torch.zeros((VAR_CAP, 12), dtype=torch.int32, device="cuda")
d_n_vars = torch.zeros(1, dtype=torch.int64, device="cuda")


def variant_legs(handle, what):
    ms = alternated([("pileup calls, whole window, sites only (%s)" % what, lambda: check(lib.lrm_pileup_sites_dev(
                         handle, None, 0, W, d_sites.data_ptr(), SITE_CAP, d_n_sites.data_ptr(), None, stream), "lrm_pileup_sites_dev")),
                     ("pileup variants, whole window (%s)" % what, lambda: check(lib.lrm_pileup_variants_dev(
                         handle, None, 0, W, d_vars.data_ptr(), VAR_CAP, d_n_vars.data_ptr(), stream), "lrm_pileup_variants_dev"))])
    a, b = (float(np.mean(v)) for v in ms.values())
    n_vars = int(d_n_vars.cpu()[0])
    vk = d_vars[:min(n_vars, VAR_CAP), 7].cpu().numpy().view(np.uint32) & 0xFF
    print("  variants / sites: %.3f ms / %.3f ms per launch = %.3f; %d records (DEL %d, SNV %d, INS %d) from %d sites; the table %.3f MB" %
          (b, a, b / a, n_vars, int((vk == 2).sum()), int((vk == 1).sum()), int((vk == 4).sum()), int(d_n_sites.cpu()[0]), 48 * min(n_vars, VAR_CAP) / 1e6), flush=True)


variant_legs(dm.pileup, "plain accumulator")
if os.environ.get("PROBE_UNTIL") == "variants":                # the call and variant stages only: one more K = 8 accumulator, then the end
    acc8 = C.c_void_p()
    check(lib.lrm_pileup_create_ins(C.byref(acc8), di.handle, window[0], window[1], 8), "lrm_pileup_create_ins")
    check(lib.lrm_pileup_add_dev(acc8, d_reads.data_ptr(), d_reads.stride(0), d_lens.data_ptr(), dm.store.data_ptr(), dm.store_stride, dm.n_ops.data_ptr(),
                                 dm.score.data_ptr(), dm.meta_r.data_ptr(), dm.meta.data_ptr(), n, None, 0, stream), "lrm_pileup_add_dev")
    variant_legs(acc8, "K = 8 accumulator")
    lib.lrm_pileup_free(acc8)
    dm.close()
    di.close()
    sys.exit(0)
timed("aln_diff_kernel", lambda: check(lib.lrm_aln_diff_dev(
    di.handle, dm.store.data_ptr(), dm.store_stride, dm.n_ops.data_ptr(), dm.score.data_ptr(), dm.meta_r.data_ptr(), dm.meta.data_ptr(), n,
    dm.diff_off.data_ptr(), total, dm.diff_events.data_ptr(), stream), "lrm_aln_diff_dev"))
timed("aln_summary_kernel", lambda: check(lib.lrm_aln_summary_dev(
    di.handle, dm.store.data_ptr(), dm.store_stride, dm.n_ops.data_ptr(), dm.score.data_ptr(), dm.meta_r.data_ptr(), n, dm.summary.data_ptr(),
    stream), "lrm_aln_summary_dev"))
# the accumulator now holds 2 + REPEATS launches of the same batch (extend's, the warm-up, the timed ones): every counter is that multiple of the first launch's
cols_now = dm.pileup_columns()
k = 2 + REPEATS
raw2 = np.zeros(8 * W + 1, dtype=np.uint32)
check(lib.lrm_debug_pileup_raw(dm.pileup, raw2.ctypes.data, len(raw2), stream), "lrm_debug_pileup_raw")
print("  after %d launches every counter word is %d times the first launch's: %s; deepest position %d" %
      (k, k, bool(np.array_equal(raw2, raw * np.uint32(k))), int(cols_now["depth"].max())), flush=True)
# ---- the insertion side (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus") ----
def add_to(library, handle):
    return lambda: check(library.lrm_pileup_add_dev(
        handle, d_reads.data_ptr(), d_reads.stride(0), d_lens.data_ptr(), dm.store.data_ptr(), dm.store_stride, dm.n_ops.data_ptr(),
        dm.score.data_ptr(), dm.meta_r.data_ptr(), dm.meta.data_ptr(), n, None, 0, stream), "lrm_pileup_add_dev")


def accumulator(library, ins_cols=None):
    h = C.c_void_p()
    if ins_cols is None:
        check(library.lrm_pileup_create(C.byref(h), di.handle, window[0], window[1]), "lrm_pileup_create")
    else:
        check(library.lrm_pileup_create_ins(C.byref(h), di.handle, window[0], window[1], ins_cols), "lrm_pileup_create_ins")
    return h


# the add on a plain accumulator: this build against itself (the spread) and, with PROBE_PARENT_LIB=<liblrm_accel.so of the
# parent commit>, against the parent's kernel on an accumulator of the parent's own -- all in this process, launched in turn
plain_a, plain_b = accumulator(lib), accumulator(lib)
legs = [("pileup_add_kernel, plain accumulator, this build (a)", add_to(lib, plain_a)), ("pileup_add_kernel, plain accumulator, this build (b)", add_to(lib, plain_b))]
parent_path = os.environ.get("PROBE_PARENT_LIB")
if parent_path:
    parent = C.CDLL(parent_path)
    for name in ("lrm_pileup_create", "lrm_pileup_add_dev", "lrm_pileup_free"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = capi.SYMBOLS[name]
    parent_a, parent_b = C.c_void_p(), C.c_void_p()
    for h in (parent_a, parent_b):
        check(parent.lrm_pileup_create(C.byref(h), di.handle, window[0], window[1]), "lrm_pileup_create (parent)")
    legs += [("pileup_add_kernel, the parent's library (a)", add_to(parent, parent_a)), ("pileup_add_kernel, the parent's library (b)", add_to(parent, parent_b))]
alternated(legs)
for h in (plain_a, plain_b):
    lib.lrm_pileup_free(h)
if parent_path:
    for h in (parent_a, parent_b):
        parent.lrm_pileup_free(h)
# the add with insertion planes, the polish next to the sites + cons bytes, the site alleles
for ins_cols in (4, 8):
    acc = accumulator(lib, ins_cols)
    timed("pileup_add_ins_kernel, K = %d (%.1f MB of insertion planes)" % (ins_cols, 16 * ins_cols * W / 1e6), add_to(lib, acc))
    if ins_cols == 8:
        ins_raw = np.zeros(4 * ins_cols * W, dtype=np.uint32)
        check(lib.lrm_debug_pileup_ins_raw(acc, ins_raw.ctypes.data, len(ins_raw), stream), "lrm_debug_pileup_ins_raw")
        per_col = ins_raw.reshape(ins_cols, 4 * W).astype(np.int64).sum(axis=1) // (1 + REPEATS)
        print("  insertion adds of one launch per column: %s (%.4f G in all, next to %.4f G event adds)" %
              (" ".join(str(int(v)) for v in per_col), per_col.sum() / 1e9, event_adds / 1e9), flush=True)
        d_seq = torch.zeros(W + W // 8, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        alternated([("pileup calls, whole window, sites + cons bytes (K = 8 accumulator)", lambda: check(lib.lrm_pileup_sites_dev(
                        acc, None, 0, W, d_sites.data_ptr(), SITE_CAP, d_n_sites.data_ptr(), d_cons.data_ptr(), stream), "lrm_pileup_sites_dev")),
                    ("pileup polish, whole window (K = 8 accumulator)", lambda: check(lib.lrm_pileup_polish_dev(
                        acc, None, 0, W, d_seq.data_ptr(), d_seq.numel(), d_len.data_ptr(), stream), "lrm_pileup_polish_dev")),
                    ("pileup polish, whole window (plain accumulator)", lambda: check(lib.lrm_pileup_polish_dev(
                        dm.pileup, None, 0, W, d_seq.data_ptr(), d_seq.numel(), d_len.data_ptr(), stream), "lrm_pileup_polish_dev"))])
        variant_legs(acc, "K = 8 accumulator")
        check(lib.lrm_pileup_polish_dev(acc, None, 0, W, d_seq.data_ptr(), d_seq.numel(), d_len.data_ptr(), stream), "lrm_pileup_polish_dev")
        n_sites8 = int(d_n_sites.cpu()[0])
        print("  polished length %d of %d positions; %d sites" % (int(d_len.cpu()[0]), W, n_sites8), flush=True)
        d_alleles = torch.zeros((max(min(n_sites8, SITE_CAP), 1), 4), dtype=torch.int32, device="cuda")
        timed("pileup site alleles, %d sites" % min(n_sites8, SITE_CAP), lambda: check(lib.lrm_pileup_site_alleles_dev(
            acc, None, d_sites.data_ptr(), min(n_sites8, SITE_CAP), d_alleles.data_ptr(), stream), "lrm_pileup_site_alleles_dev"))
        d_words = torch.zeros((1 << 20, ins_cols, 4), dtype=torch.int32, device="cuda")
        timed("pileup insertion read-back, 2^20 positions", lambda: check(lib.lrm_pileup_ins_read_dev(acc, 0, 1 << 20, d_words.data_ptr(), stream),
                                                                         "lrm_pileup_ins_read_dev"))
    lib.lrm_pileup_free(acc)
dm.close()
# ---- the host-buffer path and the merge (docs/GACT_SPEC.md, "Pileup on the host-buffer path and across replicas") ----
# The same batch through map_batch_submit on pinned buffers with dense results, two batches in flight, HOST_BATCHES timed
# batches a leg after two warm-up ones: without an accumulator, with a plain one, with K = 8.  Wall time per batch.
import time

from longreadmapper_amd.pileup import Pileup

HOST_BATCHES = int(os.environ.get("PROBE_HOST_BATCHES", "8"))
stride_s = max(mapper.units16(mapper.store_need(length, False)), 16)
pin = [(mapper.pinned_empty(r["reads"].shape), mapper.pinned_empty((n, stride_s))) for _ in range(2)]
for reads_p, _ in pin:
    reads_p[:] = r["reads"]


def host_leg(what, acc):
    pending, t0, done = [], None, 0
    for k in range(HOST_BATCHES + 2):
        reads_p, store_p = pin[k & 1]
        if len(pending) == 2:
            pending.pop(0).wait()
            done += 1
            if done == 2:                                    # two warm-up batches are through: the clock starts
                t0 = time.perf_counter()
        pending.append(mapper.map_batch_submit(di, reads_p, r["lens"], store=store_p, options=dict(dense_results=1), pileup=acc))
    for pb in pending:
        pb.wait()
    ms = (time.perf_counter() - t0) * 1e3 / HOST_BATCHES
    print("  host path, pinned + dense, two batches in flight, %s: %.2f ms per batch of %.3f Gbp (%d batches)" % (what, ms, gbp, HOST_BATCHES), flush=True)
    return ms


for rep in range(2):                                         # the legs in turn, twice: the second round is the spread
    host_leg("no accumulator", None)
    for ins_cols in (0, 8):
        acc = Pileup(di, window[0], window[1], ins_cols)
        host_leg("accumulator, K = %d" % ins_cols, acc)
        acc.close()
for reads_p, store_p in pin:
    mapper.pinned_free(reads_p)
    mapper.pinned_free(store_p)
# the merge of two accumulators over the window, both routes (the staged one forced on this device: its copies are device to device)
for ins_cols in (0, 8):
    dst, src = Pileup(di, window[0], window[1], ins_cols), Pileup(di, window[0], window[1], ins_cols)
    words = 8 * W + 1 + 4 * ins_cols * W
    timed("pileup merge, direct, K = %d (%.1f MB a side)" % (ins_cols, 4 * words / 1e6), lambda: dst.merge(src), per=(12 * words, "bytes (8 read, 4 written per word)"))
    timed("pileup merge, staged in chunks of 4 Mi words, K = %d" % ins_cols, lambda: dst.merge(src, staged_chunk=4 << 20))
    dst.close()
    src.close()
di.close()
