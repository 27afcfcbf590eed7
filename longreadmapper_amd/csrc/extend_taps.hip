// extend_taps.hip -- debug taps of the extension stage (tests only): one read through the extension kernels
// (lrm_debug_gact, lrm_debug_gact_impl) or through the anchor scan (lrm_debug_anchor), without an index walk or a workspace
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "lrm_hip_util.h"
#include "extend_stage.h"
#include "anchor_plan.h"

namespace {
// one read as a device batch of one job: its bytes, {length, target length}, its meta, {meta_r = 1, n_ops, score}
struct TapRead {
    DevBuf reads, lens, meta, res;
    int upload(const char *q, uint32_t n, uint32_t m, const lrm_seq_meta &hm) {
        if (reads.alloc((size_t) n + 32) || lens.alloc(16) || meta.alloc(sizeof(hm)) || res.alloc(16)) { lrm_set_error("device allocation failed"); return -1; }
        const uint32_t hl[2] = {n, m};
        const int32_t hr[3] = {1, 0, 0};
        HIPCHK(hipMemcpy(reads.p, q, n, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(lens.p, hl, 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(meta.p, &hm, sizeof(hm), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(res.p, hr, 12, hipMemcpyHostToDevice));
        return 0;
    }
    char *d_reads() const { return (char *) reads.p; }
    uint32_t *d_lens() const { return (uint32_t *) lens.p; }
    lrm_seq_meta *d_meta() const { return (lrm_seq_meta *) meta.p; }
    int32_t *d_res() const { return (int32_t *) res.p; }
};
}  // namespace

// direct kernel tap (tests only): simple_gact on one (q, d) pair, m may differ from n
extern "C" int lrm_debug_gact(const char *q, int n, const char *d, int m, lrm_gact_params gp, uint8_t *ops,
                              int *n_ops, int *score, int device) {
    LrmEnv env;                                  // a tap without a handle: LRM_GACT_IMPL as it stands now
    lrm_env_snapshot(&env);
    long long impl = 0;
    (void) env.get("LRM_GACT_IMPL", &impl);
    return lrm_debug_gact_impl(q, n, d, m, gp, (int) impl, ops, n_ops, score, device);
}

extern "C" int lrm_debug_gact_impl(const char *q, int n, const char *d, int m, lrm_gact_params gp, int impl, uint8_t *ops,
                                   int *n_ops, int *score, int device) {
    if (!q || !d || !ops || !n_ops || !score || n < 0 || m < 0) { lrm_set_error("bad argument"); return -1; }
    if (lrm_require_device(device) || lrm_gact_resolve_params(&gp)) return -1;
    TapRead t;
    DevBuf bd, bops, bc, bcpl, btf;
    lrm_seq_meta hm = {};
    if (t.upload(q, (uint32_t) n, (uint32_t) m, hm)) return -1;
    if (bd.alloc((size_t) m + 16) || bops.alloc((size_t) n + m + 16) || bc.alloc(sizeof(LrmDevCounters))) { lrm_set_error("device allocation failed"); return -1; }
    char *dd = (char *) bd.p;
    int32_t *dr = t.d_res();
    LrmDevCounters *dc = (LrmDevCounters *) bc.p;
    HIPCHK(hipMemset(dc, 0, sizeof(LrmDevCounters)));
    HIPCHK(hipMemcpy(dd, d, (size_t) m, hipMemcpyHostToDevice));
    LrmGactJobs jobs = {t.d_reads(), 0, t.d_lens(), t.d_lens() + 1, t.d_meta(), dr, dd, nullptr, 1, (uint8_t *) bops.p, 0, dr + 1, dr + 2};
    struct BsGuard { LrmBsScratch s = {}; ~BsGuard() { lrm_bs_scratch_free(&s); } } bs;
    LrmGactPlan plan;
    if (lrm_gact_plan(jobs, gp, impl, true, &plan)) return -1;
    if (plan.kernel == LRM_GACT_BS) {                       // planar image of the text; one that is not pure ACGT plans again
        uint64_t bytes = 0;
        if (lrm_bs_scratch_alloc(&bs.s, 1, (uint32_t) n, (uint32_t) (n > m ? n : m), &bytes)) return -1;
        if (bcpl.alloc(lrm_bs_planar_words((uint64_t) m) * 8 + 16) || btf.alloc(4)) { lrm_set_error("device allocation failed"); return -1; }
        if (lrm_bs_pack_text(dd, (uint64_t) m, (uint64_t *) bcpl.p, (uint32_t *) btf.p, nullptr)) return -1;
        uint32_t tf = 0;
        HIPCHK(hipMemcpy(&tf, btf.p, 4, hipMemcpyDeviceToHost));
        if (!tf) jobs.cpl = (const uint64_t *) bcpl.p;
        else if (lrm_gact_plan(jobs, gp, impl, false, &plan)) return -1;
    }
    if (lrm_gact_run_jobs(nullptr, jobs, (uint32_t) n, gp, plan, bs.s, dc, 0, nullptr)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    int32_t hr[3];
    HIPCHK(hipMemcpy(hr, dr, 12, hipMemcpyDeviceToHost));
    *n_ops = hr[1];
    *score = hr[2];
    if (hr[1] > 0) HIPCHK(hipMemcpy(ops, jobs.store, (size_t) hr[1], hipMemcpyDeviceToHost));
    return 0;
}

// the record of one read straight from its key
__global__ void anchor_record_kernel(const uint32_t *lens, const lrm_seq_meta *meta, const LrmMtaDev *mta,
                                     const unsigned long long *keys, lrm_anchor *out) {
    const lrm_seq_meta m = meta[0];
    out[0] = an_record(an_plan(keys[0], m.loc, lens[0], mta[m.seq_id].offset, mta[m.seq_id].seq_len), 0, 0);
}

// the scan of one read around the locus `loc` of the forward half of a sequence
extern "C" int lrm_debug_anchor(lrm_index *idx, const char *read, uint32_t len, uint64_t loc, uint32_t min_len,
                                lrm_anchor *out) {
    if (!idx || !read || !out || len == 0) { lrm_set_error("bad argument"); return -1; }
    if (lrm_require_device(idx->device) || lrm_anchor_min_len(min_len, &min_len)) return -1;
    const int nm = idx->view.mta_len;
    LrmMtaDev *hm = (LrmMtaDev *) malloc(sizeof(LrmMtaDev) * (size_t) (nm > 0 ? nm : 1));
    if (!hm) { lrm_set_error("out of memory"); return -1; }
    lrm_seq_meta m = {};
    m.seq_id = -1;
    if (hipMemcpy(hm, idx->view.mta, sizeof(LrmMtaDev) * (size_t) nm, hipMemcpyDeviceToHost) == hipSuccess)
        for (int i = 0; i < nm && m.seq_id < 0; ++i)
            if (loc >= hm[i].offset && loc < hm[i].offset + hm[i].seq_len) { m.seq_id = i; m.loc = loc; m.off = loc - hm[i].offset; }
    free(hm);
    if (m.seq_id < 0) { lrm_set_error("locus %llu is not on the forward half of a sequence", (unsigned long long) loc); return -1; }
    const bool planar = idx->d_cpl && idx->cpl_ok;              // (no workspace: the read's planar image is the tap's own)
    LrmBsScratch pl = {};
    pl.wpr = lrm_bs_planar_words(len);
    TapRead t;
    DevBuf bk, ba, bq, bf;
    if (t.upload(read, len, len, m)) return -1;
    if (bk.alloc(16) || ba.alloc(sizeof(lrm_anchor)) || bq.alloc(pl.wpr * 8 + 16) || bf.alloc(16)) { lrm_set_error("device allocation failed"); return -1; }
    pl.qpl = (uint64_t *) bq.p; pl.rflags = (uint32_t *) bf.p;
    LrmExtendBatch b = {};
    b.reads = t.d_reads(); b.lens = t.d_lens(); b.n = 1; b.max_len = len;
    b.meta = t.d_meta(); b.meta_r = t.d_res();
    if (planar && lrm_bs_pack_reads(b.reads, 0, b.lens, 1, len, pl, nullptr)) return -1;
    if (lrm_anchor_scan(b, idx->view, pl, planar ? idx->d_cpl : nullptr, min_len, (uint64_t *) bk.p, nullptr)) return -1;
    hipLaunchKernelGGL(anchor_record_kernel, dim3(1), dim3(1), 0, nullptr, b.lens, b.meta, idx->view.mta,
                       (const unsigned long long *) bk.p, (lrm_anchor *) ba.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, ba.p, sizeof(lrm_anchor), hipMemcpyDeviceToHost));
    return 0;
}
