// pileup.hip -- the pileup accumulator (lrm_pileup; docs/GACT_SPEC.md, "Pileup" and "Pileup calls"): the object's lifetime, its
// device-buffer entry points, the host rules' entries.  Host code only: the kernels are pileup_kernels.hip, the rules pileup_step.h and pileup_call_step.h.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "lrm_hip_util.h"
#include "pileup_step.h"
#include "pileup_call_step.h"

// positions [first, first + count) lie inside a window of W positions (W == 0: no window at all)
static int pile_range_check(uint64_t W, uint64_t first, uint64_t count) {
    if (W != 0 && first <= W && count <= W - first) return 0;
    lrm_set_error("pileup: positions [%llu, +%llu) outside a window of %llu", (unsigned long long) first, (unsigned long long) count, (unsigned long long) W);
    return -1;
}

// The host rule is pileup_step.h's: the row walked as a lane of pileup_add_kernel walks it, through pile_word_step.
extern "C" void lrm_pileup_add_host(const uint8_t *ops, int n_ops, const uint8_t *read, uint32_t read_len, uint64_t loc, uint64_t lo,
                                    uint64_t hi, uint32_t *planes) {
    if (!ops || n_ops <= 0 || !planes || lo >= hi) return;
    pile_host_add(ops, (uint64_t) n_ops, read, read ? read_len : 0u, loc, lo, hi, planes);
}

extern "C" int lrm_pileup_cols_host(const uint32_t *planes, uint64_t lo, uint64_t hi, uint64_t first, uint64_t count, lrm_pileup_col *out) {
    if (pile_range_check(hi > lo ? hi - lo : 0, first, count)) return -1;
    if (!planes || (count && !out)) { lrm_set_error("null argument"); return -1; }
    pile_host_cols(planes, hi - lo, first, count, out);
    return 0;
}

extern "C" void lrm_pileup_free(lrm_pileup *pl) {
    if (!pl) return;
    if (hipSetDevice(pl->device) == hipSuccess) lrm_dev_free({pl->d_planes, pl->d_tiles, pl->d_call});
    free(pl);
}

extern "C" int lrm_pileup_create(lrm_pileup **out, lrm_index *idx, uint64_t lo, uint64_t hi) {
    if (!out || !idx) { lrm_set_error("null argument"); return -1; }
    *out = nullptr;
    if (idx->n_peers > 1) { lrm_set_error("pileup: a group handle holds one text per replica; create the accumulator on one replica (lrm_index_replica)"); return -1; }
    const uint64_t con_len = idx->view.con_len;
    if (lo >= hi || hi > con_len) { lrm_set_error("pileup: window [%llu, %llu) is empty or ends behind the text (%llu positions)", (unsigned long long) lo, (unsigned long long) hi, (unsigned long long) con_len); return -1; }
    if (lrm_require_device(idx->device)) return -1;
    lrm_pileup *pl;
    if (!lrm_alloc(pl, 1, "pileup", true)) return -1;
    pl->idx = idx;
    pl->device = idx->device;
    pl->lo = lo; pl->hi = hi; pl->W = hi - lo;
    pl->n_tiles = (pl->W + LRM_PILEUP_TILE - 1) / LRM_PILEUP_TILE;
    const uint64_t plane_bytes = 4ull * LRM_PILEUP_WORDS(pl->W), guard_bytes = 4ull * LRM_PILEUP_GUARD_WORDS;
    const LrmDevAlloc table[] = {{(void **) &pl->d_planes, plane_bytes + guard_bytes}, {(void **) &pl->d_tiles, 8ull * pl->n_tiles}};
    if (lrm_dev_alloc_table(table, "pileup bytes", &pl->bytes)) { lrm_pileup_free(pl); return -1; }
    if (hipMemset(pl->d_planes, 0, plane_bytes) != hipSuccess || hipMemset((char *) pl->d_planes + plane_bytes, LRM_PILEUP_GUARD & 0xFF, guard_bytes) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        lrm_set_error("pileup: clearing %llu bytes failed", (unsigned long long) plane_bytes);
        lrm_pileup_free(pl);
        return -1;
    }
    *out = pl;
    return 0;
}

extern "C" uint64_t lrm_pileup_bytes(const lrm_pileup *pl) { return pl ? pl->bytes : 0; }
extern "C" int lrm_pileup_reset(lrm_pileup *pl, void *stream) {
    if (!pl) { lrm_set_error("null argument"); return -1; }
    if (lrm_require_device(pl->device)) return -1;
    HIPCHK(hipMemsetAsync(pl->d_planes, 0, 4ull * LRM_PILEUP_WORDS(pl->W), (hipStream_t) stream));
    return 0;
}

extern "C" int lrm_pileup_add_dev(lrm_pileup *pl, const char *d_reads, uint64_t stride, const uint32_t *d_lens, const uint8_t *d_store,
                                  uint64_t store_stride, const int32_t *d_n_ops, const int32_t *d_score, const int32_t *d_meta_r,
                                  const lrm_seq_meta *d_meta, uint64_t n, const lrm_mapq *d_mapq, uint32_t min_mapq, void *stream) {
    if (!pl || (n && (!d_reads || !d_lens || !d_store || !d_n_ops || !d_score || !d_meta_r || !d_meta))) { lrm_set_error("null argument"); return -1; }
    if (store_stride > LRM_PILEUP_MAX_STRIDE) { lrm_set_error("pileup: store_stride %llu above 2^31 (the column counts of a row are 32-bit)", (unsigned long long) store_stride); return -1; }
    if (lrm_require_device(pl->device)) return -1;
    return lrm_launch_pileup_add(pl, (const uint8_t *) d_reads, stride, d_lens, LrmOpRows{d_store, store_stride, d_n_ops, d_score, d_meta_r, d_meta, n},
                                 d_mapq, min_mapq, stream);
}

extern "C" int lrm_pileup_read_dev(lrm_pileup *pl, uint64_t first, uint64_t count, lrm_pileup_col *d_out, void *stream) {
    if (!pl || (count && !d_out)) { lrm_set_error("null argument"); return -1; }
    if (pile_range_check(pl->W, first, count)) return -1;
    if ((uintptr_t) d_out & 15u) { lrm_set_error("pileup records must be 16-byte aligned"); return -1; }
    if (count == 0) return 0;
    if (lrm_require_device(pl->device)) return -1;
    return lrm_launch_pileup_read(pl, first, count, d_out, stream);
}

// the call stage (docs/GACT_SPEC.md, "Pileup calls"): the options checked and their zero fields replaced by the defaults
static int lrm_pileup_call_check(const lrm_pileup_call_options *opt, PileCallRule *rule) {
    const lrm_pileup_call_options o = opt ? *opt : lrm_pileup_call_options{0, 0, 0, 0};
    if (o.min_pct > 100u) { lrm_set_error("pileup calls: min_pct %u above 100", o.min_pct); return -1; }
    if (o.reserved != 0u) { lrm_set_error("pileup calls: lrm_pileup_call_options.reserved is %u, not 0", o.reserved); return -1; }
    *rule = pile_call_rule(o.min_depth, o.min_count, o.min_pct);
    return 0;
}

extern "C" int64_t lrm_pileup_sites_host(const lrm_pileup_col *cols, const char *content, uint64_t pos0, uint64_t count,
                                         const lrm_pileup_call_options *opt, lrm_pileup_site *out, uint64_t cap, uint8_t *cons) {
    PileCallRule rule;
    if (lrm_pileup_call_check(opt, &rule)) return -1;
    if ((count && (!cols || !content)) || (cap && !out)) { lrm_set_error("null argument"); return -1; }
    return (int64_t) pile_host_sites(cols, content, pos0, count, rule, out, cap, cons);
}

extern "C" int lrm_pileup_sites_dev(lrm_pileup *pl, const lrm_pileup_call_options *opt, uint64_t first, uint64_t count,
                                    lrm_pileup_site *d_sites, uint64_t cap, uint64_t *d_n_sites, uint8_t *d_cons, void *stream) {
    if (!pl || !d_n_sites || (cap && !d_sites)) { lrm_set_error("null argument"); return -1; }
    PileCallRule rule;
    if (lrm_pileup_call_check(opt, &rule)) return -1;
    if (pile_range_check(pl->W, first, count)) return -1;
    if (count > 0xFFFFFFFFull) { lrm_set_error("pileup calls: %llu positions in one call (site ranks are 32-bit: at most 2^32 - 1)", (unsigned long long) count); return -1; }
    if ((uintptr_t) d_sites & 15u) { lrm_set_error("pileup sites must be 16-byte aligned"); return -1; }
    if ((uintptr_t) d_n_sites & 7u) { lrm_set_error("the pileup site count must be 8-byte aligned"); return -1; }
    if (lrm_require_device(pl->device)) return -1;
    if (count == 0) {                                                  // no tile holds a position: the total is 0
        HIPCHK(hipMemsetAsync(d_n_sites, 0, 8, (hipStream_t) stream));
        return 0;
    }
    if (!pl->d_call) {                                                 // the stage's scratch, on the first call that asks
        const LrmDevAlloc table[] = {{(void **) &pl->d_call, 8ull * pl->n_tiles}};
        if (lrm_dev_alloc_table(table, "pileup call bytes", &pl->bytes)) return -1;
    }
    return lrm_launch_pileup_sites(pl, rule, first, count, d_sites, cap, d_n_sites, d_cons, stream);
}

extern "C" int lrm_debug_pileup_raw(lrm_pileup *pl, uint32_t *out, uint64_t words, void *stream) {
    if (!pl || !out) { lrm_set_error("null argument"); return -1; }
    if (words > LRM_PILEUP_WORDS(pl->W) + LRM_PILEUP_GUARD_WORDS) { lrm_set_error("pileup: the accumulator holds %llu words", (unsigned long long) (LRM_PILEUP_WORDS(pl->W) + LRM_PILEUP_GUARD_WORDS)); return -1; }
    if (lrm_require_device(pl->device)) return -1;
    HIPCHK(hipMemcpyAsync(out, pl->d_planes, 4ull * words, hipMemcpyDeviceToHost, (hipStream_t) stream));
    HIPCHK(hipStreamSynchronize((hipStream_t) stream));
    return 0;
}
