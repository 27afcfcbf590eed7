// extend_launch.hip -- host side of the extension stage: parameters, THE choice of the kernel of a job table, its launch,
// and the classic mode (lrm_launch_extend: every read against the text at its voted locus).  The kernels are in
// gact_kernels.hip and gact_bs_kernels.hip; the anchored mode (anchor_kernels.hip) runs its job table through the same
// plan and launch.
#include <hip/hip_runtime.h>
#include "lrm_hip_util.h"
#include "extend_stage.h"

// {0,0,0} selects the defaults; the limits are those of the kernels
int lrm_gact_resolve_params(lrm_gact_params *gp) {
    if (gp->T == 0 && gp->O == 0 && gp->W == 0) {
        gp->T = LRM_GACT_T_DEFAULT; gp->O = LRM_GACT_O_DEFAULT; gp->W = LRM_GACT_W_DEFAULT;
    }
    if (gp->T < 16 || gp->T > 512 || gp->O < 0 || gp->O >= gp->T || gp->W < 2 || (gp->W & 1) || gp->W > 1024) {
        lrm_set_error("unsupported GACT parameters T=%d O=%d W=%d (need 16<=T<=512, 0<=O<T, even 2<=W<=1024)",
                      gp->T, gp->O, gp->W);
        return -1;
    }
    return 0;
}

// THE choice of the extension kernel (gact_impl: lrm_map_options in lrm_accel.h; the rule as a table: INTEGRATION.md)
int lrm_gact_plan(const LrmGactJobs &j, lrm_gact_params gp, int impl, bool planar, LrmGactPlan *out) {
    LrmGactPlan p = {};
    const int nblk = lrm_gact_tb_blocks(gp.T, gp.O);
    // Bit-sliced kernel: a wavefront carries 64 reads, so it needs a large batch to fill the chip (below ~16 k reads
    // the two-reads-per-wavefront kernel finishes first); it stores CIGAR bytes four at a time.
    if (gp.W <= 128 && planar && (((uintptr_t) j.store | (uintptr_t) j.store_stride) & 3u) == 0 &&
        (impl == 4 || (impl == 0 && j.n >= LRM_BS_MIN_READS)))
        p.kernel = LRM_GACT_BS;
    else if (gp.W <= 128 && impl != 1 && nblk <= 32)
        p.kernel = LRM_GACT_PACKED;
    else                                  // W > 128, T - O > 256 (more traceback planes than the packed kernel keeps in registers), impl 1
        p.kernel = LRM_GACT_WIDE;
    p.slot = p.kernel == LRM_GACT_BS ? LRM_K_GACT_BS : LRM_K_GACT;
    if (p.kernel == LRM_GACT_PACKED) {
        p.nb = nblk <= 26 ? 26 : 32;
        p.fullband = gp.W >= 128;
        p.lds = LrmPackedLds(gp.T).total();
    } else {                              // DPL diagonal pairs per lane for the band W
        p.dpl = gp.W <= 128 ? 1 : gp.W <= 256 ? 2 : gp.W <= 512 ? 4 : 8;
        p.lds = LrmWideLds(p.dpl, gp.T, gp.O).total();
        if (p.lds > 160 * 1024) { lrm_set_error("GACT T=%d O=%d W=%d needs %zu B of LDS (> 160 KiB)", gp.T, gp.O, gp.W, p.lds); return -1; }
    }
    *out = p;
    return 0;
}

// the extension proper over a table of jobs (anchor_kernels.hip builds one; the classic mode's table is the batch itself)
int lrm_gact_launch_jobs(const LrmGactJobs &j, lrm_gact_params gp, const LrmGactPlan &plan, const LrmBsScratch *bs,
                         LrmDevCounters *counters, uint32_t bs_waves, bool count, void *stream) {
    if (plan.kernel == LRM_GACT_BS) {
        if (lrm_bs_launch(j, gp, *bs, counters, bs_waves, count, stream)) return -1;
        // reads holding a byte other than ACGT (rare): one read per wavefront, flagged reads only
        return lrm_gact_launch_wide(j, gp, plan, counters, bs->rflags, stream);
    }
    if (plan.kernel == LRM_GACT_PACKED) return lrm_gact_launch_packed(j, gp, plan, counters, stream);
    return lrm_gact_launch_wide(j, gp, plan, counters, nullptr, stream);
}

int lrm_gact_run_jobs(lrm_workspace *ws, const LrmGactJobs &j, uint32_t max_len, lrm_gact_params gp, const LrmGactPlan &plan,
                      const LrmBsScratch &bs, LrmDevCounters *counters, uint32_t bs_waves, void *stream) {
    if (plan.kernel == LRM_GACT_BS) {
        lrm_time_begin(ws, LRM_K_PACK_PLANAR, stream);
        if (lrm_bs_pack_reads(j.reads, j.stride, j.lens, j.n, max_len, bs, stream)) return -1;
        lrm_time_end(ws, stream);
    }
    lrm_time_begin(ws, plan.slot, stream);
    if (lrm_gact_launch_jobs(j, gp, plan, &bs, counters, bs_waves, ws && ws->counting, stream)) return -1;
    lrm_time_end(ws, stream);
    return 0;
}

int lrm_launch_extend(lrm_index *idx, lrm_workspace *ws, const LrmExtendBatch &b, lrm_gact_params gp, const LrmMapTune &mt,
                      void *stream) {
    if (b.n == 0) return 0;
    if (mt.anchored)                                       // anchor_kernels.hip; nothing below is reached
        return lrm_launch_extend_anchored(idx, ws, b, gp, nullptr, mt.anchor_min_len, lrm_clip_of(mt), mt, stream);
    if (mt.clip) { lrm_set_error("lrm_map_options.clip needs lrm_map_options.anchored"); return -1; }
    if (lrm_gact_resolve_params(&gp)) return -1;
    if (b.store_stride < 2ull * b.max_len) {
        lrm_set_error("store_stride %llu < 2*max_len %u", (unsigned long long) b.store_stride, b.max_len);
        return -1;
    }
    const bool planar = lrm_planar_ready(idx, ws) && b.n <= ws->n_max && b.max_len <= ws->max_len;     // ... and the scratch holds the batch
    const LrmGactJobs jobs = {b.reads, b.stride, b.lens, nullptr, b.meta, b.meta_r, idx->view.content, idx->d_cpl, b.n,
                              b.store, b.store_stride, b.n_ops, b.score};
    LrmGactPlan plan;
    if (lrm_gact_plan(jobs, gp, mt.gact_impl, planar, &plan)) return -1;
    if (lrm_launch_locus_revcomp(idx, ws, b, stream)) return -1;
    if (lrm_gact_run_jobs(ws, jobs, b.max_len, gp, plan, ws->bs, ws->d_counters, mt.bs_waves, stream)) return -1;
    HIPCHK(hipGetLastError());
    return 0;
}
