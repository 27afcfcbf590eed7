// extend_taps.hip -- debug taps of the extension stage (tests only): a table of (read, target) jobs through the extension
// kernels (lrm_debug_gact_jobs; one pair: lrm_debug_gact, lrm_debug_gact_impl) or one read through the anchor scan
// (lrm_debug_anchor), without an index walk or a workspace
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <vector>
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

// One job table through the plan and the launch path of the product (lrm_gact_plan, lrm_bs_pack_reads, lrm_gact_launch_jobs),
// with tlens set: job k is read row k against text[toffs[k], toffs[k] + tlens[k])
extern "C" int lrm_debug_gact_jobs(const lrm_debug_gact_table *t, lrm_gact_params gp, int impl, uint32_t bs_waves, int count,
                                   int device) {
    if (!t || !t->reads || !t->lens || !t->text || !t->toffs || !t->tlens || !t->store || !t->n_ops || !t->score || t->n == 0 ||
        t->n > (1u << 24)) { lrm_set_error("bad argument"); return -1; }
    if (lrm_require_device(device) || lrm_gact_resolve_params(&gp)) return -1;
    const uint64_t n = t->n;
    uint32_t max_len = 0, ops_len = 0;
    std::vector<lrm_seq_meta> hm(n);
    std::vector<int32_t> hr(n, 1);
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t nk = t->lens[k], mk = t->tlens[k];
        if (nk > t->stride || t->toffs[k] > t->text_len || mk > t->text_len - t->toffs[k] || nk + mk > t->store_stride ||
            nk > 0x3fffffffu || mk > 0x3fffffffu) {
            lrm_set_error("job %llu: read, target or op row out of bounds", (unsigned long long) k);
            return -1;
        }
        max_len = nk > max_len ? (uint32_t) nk : max_len;
        ops_len = (nk > mk ? nk : mk) > ops_len ? (uint32_t) (nk > mk ? nk : mk) : ops_len;
        hm[k] = lrm_seq_meta{};
        hm[k].loc = t->toffs[k];
        if (t->meta_r) hr[k] = t->meta_r[k];
    }
    DevBuf reads, lens, tlens, meta, res, nops, score, text, store, bc, bcpl, btf;
    const uint64_t store_bytes = n * t->store_stride;
    if (reads.alloc(n * t->stride + 32) || lens.alloc(n * 4) || tlens.alloc(n * 4) || meta.alloc(n * sizeof(lrm_seq_meta)) ||
        res.alloc(n * 4) || nops.alloc(n * 4) || score.alloc(n * 4) || text.alloc(t->text_len + 16) || store.alloc(store_bytes + 16) ||
        bc.alloc(sizeof(LrmDevCounters))) { lrm_set_error("device allocation failed"); return -1; }
    LrmDevCounters *dc = (LrmDevCounters *) bc.p;
    HIPCHK(hipMemset(dc, 0, sizeof(LrmDevCounters)));
    HIPCHK(hipMemcpy(reads.p, t->reads, n * t->stride, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(lens.p, t->lens, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(tlens.p, t->tlens, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(meta.p, hm.data(), n * sizeof(lrm_seq_meta), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(res.p, hr.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(nops.p, t->n_ops, n * 4, hipMemcpyHostToDevice));      // what a kernel leaves alone comes back as it went in
    HIPCHK(hipMemcpy(score.p, t->score, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(store.p, t->store, store_bytes, hipMemcpyHostToDevice));
    if (t->text_len) HIPCHK(hipMemcpy(text.p, t->text, t->text_len, hipMemcpyHostToDevice));
    LrmGactJobs jobs = {(const char *) reads.p, t->stride, (const uint32_t *) lens.p, (const uint32_t *) tlens.p,
                        (const lrm_seq_meta *) meta.p, (const int32_t *) res.p, (const char *) text.p, nullptr, n,
                        (uint8_t *) store.p, t->store_stride, (int32_t *) nops.p, (int32_t *) score.p};
    struct BsGuard { LrmBsScratch s = {}; ~BsGuard() { lrm_bs_scratch_free(&s); } } bs;
    LrmGactPlan plan;
    if (lrm_gact_plan(jobs, gp, impl, true, &plan)) return -1;
    if (plan.kernel == LRM_GACT_BS) {                       // planar image of the text; one that is not pure ACGT plans again
        uint64_t bytes = 0;
        if (lrm_bs_scratch_alloc(&bs.s, n, max_len, ops_len, &bytes)) return -1;
        if (bcpl.alloc(lrm_bs_planar_words(t->text_len) * 8 + 16) || btf.alloc(4)) { lrm_set_error("device allocation failed"); return -1; }
        if (lrm_bs_pack_text((const char *) text.p, t->text_len, (uint64_t *) bcpl.p, (uint32_t *) btf.p, nullptr)) return -1;
        uint32_t tf = 0;
        HIPCHK(hipMemcpy(&tf, btf.p, 4, hipMemcpyDeviceToHost));
        if (!tf) jobs.cpl = (const uint64_t *) bcpl.p;
        else if (lrm_gact_plan(jobs, gp, impl, false, &plan)) return -1;
    }
    if (plan.kernel == LRM_GACT_BS && lrm_bs_pack_reads(jobs.reads, jobs.stride, jobs.lens, n, max_len, bs.s, nullptr)) return -1;
    if (lrm_gact_launch_jobs(jobs, gp, plan, &bs.s, dc, bs_waves, count != 0, nullptr)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(t->n_ops, nops.p, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(t->score, score.p, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(t->store, store.p, store_bytes, hipMemcpyDeviceToHost));
    if (t->counters) {
        LrmDevCounters hc;
        HIPCHK(hipMemcpy(&hc, dc, sizeof(hc), hipMemcpyDeviceToHost));
        t->counters[0] = hc.gact_tiles;
        for (int e = 0; e < LRM_BSC_N; ++e) t->counters[1 + e] = hc.bs_count[e];
    }
    return 0;
}

// ... and its one-pair call
extern "C" int lrm_debug_gact_impl(const char *q, int n, const char *d, int m, lrm_gact_params gp, int impl, uint8_t *ops,
                                   int *n_ops, int *score, int device) {
    if (!q || !d || !ops || !n_ops || !score || n < 0 || m < 0) { lrm_set_error("bad argument"); return -1; }
    const uint32_t len = (uint32_t) n, tlen = (uint32_t) m;
    const uint64_t toff = 0;
    std::vector<uint8_t> row(((size_t) n + m + 19) & ~(size_t) 3);    // a row the bit-sliced kernel's expansion may store words into
    int32_t hn = 0, hs = 0;
    lrm_debug_gact_table t = {};
    t.n = 1; t.reads = q; t.stride = len; t.lens = &len;
    t.text = d; t.text_len = tlen; t.toffs = &toff; t.tlens = &tlen;
    t.store = row.data(); t.store_stride = row.size(); t.n_ops = &hn; t.score = &hs;
    if (lrm_debug_gact_jobs(&t, gp, impl, 0, 0, device)) return -1;
    *n_ops = hn;
    *score = hs;
    if (hn > 0) memcpy(ops, row.data(), (size_t) hn);
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
