// workspace.hip -- lrm_workspace: the device scratch of a batch shape, its sticky error word, per-kernel timing and stats
#include <hip/hip_runtime.h>
#include <cstring>
#include <new>
#include <vector>
#include "lrm_hip_util.h"
#include "extend_stage.h"

// ------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------
extern "C" void lrm_workspace_free(lrm_workspace *ws) {
    if (!ws) return;
    (void) hipSetDevice(ws->device);
    lrm_dev_free({ws->d_reads2, ws->d_rec, ws->d_phase, ws->d_decided, ws->d_hcount, ws->d_counters, ws->d_recq, ws->d_cnt, ws->d_kc_key,
                  ws->d_kc_ord, ws->d_redo, ws->d_big, ws->d_gtab, ws->d_glock, ws->d_mq_phase});
    lrm_bs_scratch_free(&ws->bs);
    lrm_anchor_scratch_free(ws);
    lrm_split_scratch_free(ws);
    lrm_sec_scratch_free(ws);
    if (ws->h_err) (void) hipHostFree((void *) ws->h_err);
    for (int i = 0; i < LRM_MAX_TIMED; ++i) {
        if (ws->ev_start[i]) (void) hipEventDestroy((hipEvent_t) ws->ev_start[i]);
        if (ws->ev_stop[i]) (void) hipEventDestroy((hipEvent_t) ws->ev_stop[i]);
    }
    delete ws;
}

extern "C" uint64_t lrm_workspace_bytes(const lrm_workspace *ws) { return ws ? ws->bytes : 0; }

extern "C" int lrm_workspace_create(lrm_workspace **out, lrm_index *idx, uint64_t n_max, uint32_t max_len,
                                    uint32_t seed_len, uint32_t thres) {
    return lrm_workspace_create_parts(out, idx, n_max, max_len, seed_len, thres, LRM_WS_SEED | LRM_WS_EXTEND);
}

// parts: LRM_WS_SEED (packed reads, survivor lists, phase results), LRM_WS_EXTEND (planar reads, checkpoints, codes);
// the host pipeline seeds in small sub-batches and extends in larger groups, each with the scratch it needs
int lrm_workspace_create_parts(lrm_workspace **out, lrm_index *idx, uint64_t n_max, uint32_t max_len,
                               uint32_t seed_len, uint32_t thres, int parts) {
    if (!out || !idx) { lrm_set_error("null argument"); return -1; }
    if (seed_len < 1 || seed_len > 32) { lrm_set_error("seed_len %u outside [1,32]", seed_len); return -1; }
    if (thres >= (1u << 24)) { lrm_set_error("thres %u >= 2^24 unsupported", thres); return -1; }
    if (n_max == 0) n_max = 1;
    if (lrm_require_device(idx->device)) return -1;
    lrm_workspace *ws = new (std::nothrow) lrm_workspace;
    if (!ws) { lrm_set_error("out of memory"); return -1; }
    memset(ws, 0, sizeof(*ws));
    ws->idx = idx; ws->device = idx->device; ws->n_max = n_max; ws->max_len = max_len;
    ws->seed_len = seed_len; ws->thres = thres;
    ws->P = seed_len + 1;
    uint32_t jl = max_len > seed_len ? max_len - seed_len : 0;
    ws->cap_q = (jl + ws->P - 1) / ws->P;
    if (ws->cap_q == 0) ws->cap_q = 1;
    ws->words_per_read = (uint64_t) max_len / 32 + 2;
    ws->parts = parts;
    {   // pool of global vote tables: a slice holds 2^k >= 2 x the most hits one (read, phase) item can have
        const uint64_t hmax = (uint64_t) ws->cap_q * (thres > 1 ? thres - 1 : 1);
        uint64_t gs = 1024;
        while (gs < 2 * hmax && gs < (1ull << 26)) gs <<= 1;
        uint64_t nsl = (256ull << 20) / (gs * 16);
        ws->g_slots = (uint32_t) gs;
        ws->g_slices = (uint32_t) (nsl < 2 ? 2 : nsl > 32 ? 32 : nsl);
    }
    const LrmDevAlloc seed[] = {
        {(void **) &ws->d_reads2, n_max * ws->words_per_read * 8 + 128},   // + slack: seed_search's scalar window loads reach 6 words
        {(void **) &ws->d_rec, n_max * (uint64_t) ws->P * ws->cap_q * 8},
        {(void **) &ws->d_recq, n_max * (uint64_t) ws->P * ws->cap_q * 4},
        {(void **) &ws->d_cnt, n_max * (uint64_t) ws->P * 4},
        {(void **) &ws->d_kc_key, (uint64_t) LRM_VOTE_GRID * LRM_VOTE_KC_CAP * 8},
        {(void **) &ws->d_kc_ord, (uint64_t) LRM_VOTE_GRID * LRM_VOTE_KC_CAP * 4},
        {(void **) &ws->d_redo, n_max * (uint64_t) ws->P * 8},
        {(void **) &ws->d_big, n_max * (uint64_t) ws->P * 8},
        {(void **) &ws->d_gtab, (uint64_t) ws->g_slices * ws->g_slots * 16},
        {(void **) &ws->d_glock, 64 * 4},
        {(void **) &ws->d_phase, n_max * (uint64_t) ws->P * sizeof(LrmPhaseRes)},
        {(void **) &ws->d_decided, n_max},
        {(void **) &ws->d_hcount, n_max * (uint64_t) ws->P * 4},
    };
    const LrmDevAlloc both[] = {{(void **) &ws->d_counters, sizeof(LrmDevCounters)}};
    if (((parts & LRM_WS_SEED) && lrm_dev_alloc_table(seed, "workspace bytes", &ws->bytes)) ||
        ((parts & (LRM_WS_SEED | LRM_WS_EXTEND)) && lrm_dev_alloc_table(both, "workspace bytes", &ws->bytes))) {
        lrm_workspace_free(ws);
        return -1;
    }
    if ((parts & LRM_WS_EXTEND) && lrm_bs_scratch_alloc(&ws->bs, n_max, max_len, max_len, &ws->bytes)) { lrm_workspace_free(ws); return -1; }
    if (hipMemset(ws->d_counters, 0, sizeof(LrmDevCounters)) != hipSuccess) { lrm_workspace_free(ws); lrm_set_error("memset failed"); return -1; }
    if (ws->d_glock && hipMemset(ws->d_glock, 0, 64 * 4) != hipSuccess) { lrm_workspace_free(ws); lrm_set_error("memset failed"); return -1; }
    {   // error word: host-coherent pinned memory the kernels store to (never reset by a launch)
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            if (h) (void) hipHostFree(h);
            lrm_workspace_free(ws);
            lrm_set_error("allocation of the workspace error word failed");
            return -1;
        }
        memset(h, 0, 64);
        ws->h_err = (volatile uint32_t *) h;
        ws->d_err = (uint32_t *) d;
    }
    *out = ws;
    return 0;
}

// Reads and clears the sticky error word.  Kernels that raised it have completed only if the caller has
// synchronised with them; a later call sees the rest ("the next call after the faulty batch fails").
int lrm_ws_take_error(lrm_workspace *ws) {
    if (!ws || !ws->h_err) return 0;
    const uint32_t e = *ws->h_err;
    if (!e) return 0;
    *ws->h_err = 0;
    if (e & LRM_ERR_VOTE_OVERFLOW)
        lrm_set_error("vote table overflow in the multi-pass tier: results of some phases of an earlier batch on this workspace are invalid");
    else lrm_set_error("device error word 0x%x", e);
    return -2;
}

extern "C" int lrm_workspace_stats(lrm_workspace *ws, lrm_stats *out, void *stream) {
    if (!ws || !out) { lrm_set_error("null argument"); return -1; }
    HIPCHK(hipSetDevice(ws->device));
    LrmDevCounters c;
    HIPCHK(hipMemcpyAsync(&c, ws->d_counters, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t) stream));
    HIPCHK(hipStreamSynchronize((hipStream_t) stream));
    {   // tier occupancy from the per-(read,phase) hit counts of the last seed call (host-side count)
        std::vector<uint32_t> hc((size_t) ws->n_last * ws->P);
        if (!hc.empty() && ws->d_hcount) HIPCHK(hipMemcpy(hc.data(), ws->d_hcount, hc.size() * 4, hipMemcpyDeviceToHost));
        else hc.clear();
        uint64_t t2 = 0, t3 = 0;
        for (uint32_t h : hc) { t2 += (h > LRM_VOTE_T1_LIMIT && h <= LRM_VOTE_T3_LIMIT); t3 += (h > LRM_VOTE_T3_LIMIT); }
        out->vote_tier2_items = t2;
        out->vote_tier3_items = t3;
    }
    out->reads_decided_phase0 = c.decided_phase0;
    out->gact_tiles = c.gact_tiles;
    out->vote_redo_items = c.vote_redo_n[0] + c.vote_redo_n[1];
    out->seeds_evaluated = c.seed_traffic[0];
    out->seed_table_lookups = c.seed_traffic[1];
    out->seed_rank_requests = c.seed_traffic[2];
    out->bs_wave_tiles = c.bs_count[LRM_BSC_WAVE_TILES];
    out->bs_pass1_pairs_masked = c.bs_count[LRM_BSC_P1_MASKED];
    out->bs_pass1_pairs_plain = c.bs_count[LRM_BSC_P1_PLAIN];
    out->bs_blocks_full = c.bs_count[LRM_BSC_P2_FULL];
    out->bs_blocks_windowed = c.bs_count[LRM_BSC_P2_WINDOWED];
    out->bs_blocks_skipped = c.bs_count[LRM_BSC_P2_SKIPPED];
    out->bs_refill_rounds = c.bs_count[LRM_BSC_REFILLS];
    return lrm_ws_take_error(ws);
}

extern "C" int lrm_debug_vote_results(lrm_workspace *ws, uint64_t n, uint64_t *out, void *stream) {
    if (!ws || !out || !ws->d_phase) { lrm_set_error("null argument"); return -1; }
    if (n > ws->n_last) { lrm_set_error("the last seed call on this workspace had %llu reads", (unsigned long long) ws->n_last); return -1; }
    HIPCHK(hipSetDevice(ws->device));
    HIPCHK(hipMemcpyAsync(out, ws->d_phase, n * (uint64_t) ws->P * sizeof(LrmPhaseRes), hipMemcpyDeviceToHost, (hipStream_t) stream));
    HIPCHK(hipStreamSynchronize((hipStream_t) stream));
    return 0;
}

// ------------------------------------------------------------------------------------------
// per-kernel timing
// ------------------------------------------------------------------------------------------
void lrm_time_begin(lrm_workspace *ws, int kernel, void *stream) {
    if (!ws || !ws->timing || ws->n_timed >= LRM_MAX_TIMED) return;
    int i = ws->n_timed;
    if (!ws->ev_start[i]) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        ws->ev_start[i] = a; ws->ev_stop[i] = b;
    }
    ws->ev_kernel[i] = kernel;
    (void) hipEventRecord((hipEvent_t) ws->ev_start[i], (hipStream_t) stream);
}

void lrm_time_end(lrm_workspace *ws, void *stream) {
    if (!ws || !ws->timing || ws->n_timed >= LRM_MAX_TIMED || !ws->ev_stop[ws->n_timed]) return;
    (void) hipEventRecord((hipEvent_t) ws->ev_stop[ws->n_timed], (hipStream_t) stream);
    ws->n_timed++;
}

extern "C" int lrm_workspace_set_counting(lrm_workspace *ws, int enable) {
    if (!ws) { lrm_set_error("null argument"); return -1; }
    ws->counting = enable ? 1 : 0;
    return 0;
}

extern "C" int lrm_workspace_set_timing(lrm_workspace *ws, int enable) {
    if (!ws) { lrm_set_error("null argument"); return -1; }
    ws->timing = enable ? 1 : 0;
    ws->n_timed = 0;
    return 0;
}

extern "C" int lrm_workspace_timing(lrm_workspace *ws, double *ms, uint64_t *launches, void *stream) {
    if (!ws || !ms || !launches) { lrm_set_error("null argument"); return -1; }
    HIPCHK(hipSetDevice(ws->device));
    HIPCHK(hipStreamSynchronize((hipStream_t) stream));
    for (int i = 0; i < ws->n_timed; ++i) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, (hipEvent_t) ws->ev_start[i], (hipEvent_t) ws->ev_stop[i]));
        ms[ws->ev_kernel[i]] += (double) t;
        launches[ws->ev_kernel[i]] += 1;
    }
    ws->n_timed = 0;
    return 0;
}

extern "C" const char *lrm_kernel_name(int k) {
    static const char *names[LRM_K_COUNT] = {"pack2bit_kernel", "seed_search_kernel", "vote_kernel", "decide_kernel",
                                             "locus_resolve_kernel", "revcomp_kernel", "gact_kernel",
                                             "bs_pack_reads_kernel", "gact_bs_kernel"};
    return k >= 0 && k < LRM_K_COUNT ? names[k] : "?";
}

