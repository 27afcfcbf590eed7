// pileup.hip -- the pileup accumulator (lrm_pileup; docs/GACT_SPEC.md, "Pileup" and "Pileup calls"): the object's lifetime, its
// device-buffer entry points, the host rules' entries.  Host code only: the kernels are pileup_kernels.hip, the rules pileup_step.h,
// pileup_call_step.h, pileup_ins_step.h ("Pileup insertions and the polished consensus") and pileup_var_step.h ("Pileup variants and VCF").
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include "lrm_hip_util.h"
#include "pileup_step.h"
#include "pileup_call_step.h"
#include "pileup_ins_step.h"
#include "pileup_var_step.h"

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
    if (hipSetDevice(pl->device) == hipSuccess) lrm_dev_free({pl->d_planes, pl->d_tiles, pl->d_call, pl->d_ins, pl->d_stage, pl->d_var});
    free(pl);
}

// ins_cols == 0: the accumulator of lrm_pileup_create, nothing more allocated or booked.  as_replica: idx was named as one
// replica of its handle (lrm_pileup_create_replica) -- replica 0 of a group handle is the group handle itself
static int pile_create(lrm_pileup **out, lrm_index *idx, uint64_t lo, uint64_t hi, uint32_t ins_cols, bool as_replica) {
    if (!out || !idx) { lrm_set_error("null argument"); return -1; }
    *out = nullptr;
    if (ins_cols > LRM_PILEUP_INS_COLS_MAX) { lrm_set_error("pileup: %u insertion columns, at most %d", ins_cols, LRM_PILEUP_INS_COLS_MAX); return -1; }
    if (!as_replica && idx->n_peers > 1) { lrm_set_error("pileup: a group handle holds one text per replica; create the accumulator on one replica (lrm_index_replica)"); return -1; }
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
    if (ins_cols) {                                                    // the insertion planes: guarded and zeroed like the first allocation
        const uint64_t ins_bytes = 4ull * LRM_PILEUP_INS_WORDS(pl->W, ins_cols);
        const LrmDevAlloc ins_table[] = {{(void **) &pl->d_ins, ins_bytes + guard_bytes}};
        if (lrm_dev_alloc_table(ins_table, "pileup insertion bytes", &pl->bytes)) { lrm_pileup_free(pl); return -1; }
        pl->ins_cols = ins_cols;
        if (hipMemset(pl->d_ins, 0, ins_bytes) != hipSuccess || hipMemset((char *) pl->d_ins + ins_bytes, LRM_PILEUP_GUARD & 0xFF, guard_bytes) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess) {
            lrm_set_error("pileup: clearing %llu bytes failed", (unsigned long long) ins_bytes);
            lrm_pileup_free(pl);
            return -1;
        }
    }
    *out = pl;
    return 0;
}
extern "C" int lrm_pileup_create_ins(lrm_pileup **out, lrm_index *idx, uint64_t lo, uint64_t hi, uint32_t ins_cols) { return pile_create(out, idx, lo, hi, ins_cols, false); }
extern "C" int lrm_pileup_create(lrm_pileup **out, lrm_index *idx, uint64_t lo, uint64_t hi) { return pile_create(out, idx, lo, hi, 0u, false); }
extern "C" int lrm_pileup_create_replica(lrm_pileup **out, lrm_index *idx, int r, uint64_t lo, uint64_t hi, uint32_t ins_cols) {
    if (!out || !idx) { lrm_set_error("null argument"); return -1; }
    *out = nullptr;
    lrm_index *rep = lrm_index_replica(idx, r);
    if (!rep) { lrm_set_error("pileup: replica %d of a handle of %d", r, lrm_index_replicas(idx)); return -1; }
    return pile_create(out, rep, lo, hi, ins_cols, true);
}
extern "C" uint32_t lrm_pileup_ins_cols(const lrm_pileup *pl) { return pl ? pl->ins_cols : 0u; }

extern "C" uint64_t lrm_pileup_bytes(const lrm_pileup *pl) { return pl ? pl->bytes : 0; }
extern "C" int lrm_pileup_reset(lrm_pileup *pl, void *stream) {
    if (!pl) { lrm_set_error("null argument"); return -1; }
    if (lrm_require_device(pl->device)) return -1;
    HIPCHK(hipMemsetAsync(pl->d_planes, 0, 4ull * LRM_PILEUP_WORDS(pl->W), (hipStream_t) stream));
    if (pl->d_ins) HIPCHK(hipMemsetAsync(pl->d_ins, 0, 4ull * LRM_PILEUP_INS_WORDS(pl->W, pl->ins_cols), (hipStream_t) stream));
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

// the stage's scratch (two words per tile), allocated by the first call that asks -- the sites or the polish -- and booked then
static int lrm_pileup_call_scratch(lrm_pileup *pl) {
    if (pl->d_call) return 0;
    const LrmDevAlloc table[] = {{(void **) &pl->d_call, 8ull * pl->n_tiles}};
    return lrm_dev_alloc_table(table, "pileup call bytes", &pl->bytes);
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
    if (lrm_pileup_call_scratch(pl)) return -1;
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

// ---- the merge (docs/GACT_SPEC.md, "Pileup on the host-buffer path and across replicas") ----
// dst += src over both allocations.  chunk == 0: the kernel reads src's planes directly (one device).  Otherwise src's words
// cross chunk by chunk into dst's staging buffer and the kernel adds each chunk; copy and add alternate by stream order.
static int pile_merge(lrm_pileup *dst, const lrm_pileup *src, uint64_t chunk, void *stream) {
    if (!dst || !src) { lrm_set_error("null argument"); return -1; }
    if (dst == src) { lrm_set_error("pileup merge: dst and src are the same accumulator"); return -1; }
    if (dst->lo != src->lo || dst->hi != src->hi) {
        lrm_set_error("pileup merge: windows [%llu, %llu) and [%llu, %llu) differ", (unsigned long long) dst->lo, (unsigned long long) dst->hi,
                      (unsigned long long) src->lo, (unsigned long long) src->hi);
        return -1;
    }
    if (dst->ins_cols != src->ins_cols) { lrm_set_error("pileup merge: %u and %u insertion columns", dst->ins_cols, src->ins_cols); return -1; }
    if (chunk > LRM_PILEUP_MERGE_CHUNK) { lrm_set_error("pileup merge: a chunk of %llu words, the staging buffer holds %llu", (unsigned long long) chunk, (unsigned long long) LRM_PILEUP_MERGE_CHUNK); return -1; }
    if (lrm_require_device(dst->device)) return -1;
    if (chunk && !dst->d_stage) {
        const LrmDevAlloc table[] = {{(void **) &dst->d_stage, 4ull * LRM_PILEUP_MERGE_CHUNK}};
        if (lrm_dev_alloc_table(table, "pileup merge staging bytes", &dst->bytes)) return -1;
    }
    const hipStream_t st = (hipStream_t) stream;
    const struct { uint32_t *d; const uint32_t *s; uint64_t words; } parts[2] = {
        {dst->d_planes, src->d_planes, LRM_PILEUP_WORDS(dst->W)}, {dst->d_ins, src->d_ins, dst->ins_cols ? LRM_PILEUP_INS_WORDS(dst->W, dst->ins_cols) : 0u}};
    for (const auto &p : parts) {
        if (!chunk) { if (lrm_launch_pileup_merge(p.d, p.s, p.words, stream)) return -1; continue; }
        for (uint64_t off = 0; off < p.words; off += chunk) {
            const uint64_t n = p.words - off < chunk ? p.words - off : chunk;
            if (src->device == dst->device) HIPCHK(hipMemcpyAsync(dst->d_stage, p.s + off, 4ull * n, hipMemcpyDeviceToDevice, st));
            else HIPCHK(hipMemcpyPeerAsync(dst->d_stage, dst->device, p.s + off, src->device, 4ull * n, st));
            if (lrm_launch_pileup_merge(p.d + off, dst->d_stage, n, stream)) return -1;
        }
    }
    return 0;
}
extern "C" int lrm_pileup_merge_dev(lrm_pileup *dst, const lrm_pileup *src, void *stream) {
    return pile_merge(dst, src, dst && src && dst->device != src->device ? LRM_PILEUP_MERGE_CHUNK : 0u, stream);
}
extern "C" int lrm_debug_pileup_merge_staged(lrm_pileup *dst, const lrm_pileup *src, uint64_t chunk_words, void *stream) {
    if (chunk_words < 4u || (chunk_words & 3u)) { lrm_set_error("pileup merge: a chunk of %llu words, not a multiple of 4 of at least 4", (unsigned long long) chunk_words); return -1; }
    return pile_merge(dst, src, chunk_words, stream);
}

// ---- the insertion side (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus"; the rules: pileup_ins_step.h) ----
static int pile_ins_check(const lrm_pileup *pl, const char *what) {
    if (pl->ins_cols) return 0;
    lrm_set_error("%s: the accumulator has no insertion planes (lrm_pileup_create_ins)", what);
    return -1;
}

extern "C" void lrm_pileup_ins_add_host(const uint8_t *ops, int n_ops, const uint8_t *read, uint32_t read_len, uint64_t loc, uint64_t lo,
                                        uint64_t hi, uint32_t ins_cols, uint32_t *ins_planes) {
    if (!ops || n_ops <= 0 || !ins_planes || lo >= hi || ins_cols == 0 || ins_cols > LRM_PILEUP_INS_COLS_MAX) return;
    pile_ins_host_add(ops, (uint64_t) n_ops, read, read ? read_len : 0u, loc, lo, hi, ins_cols, ins_planes);
}

extern "C" int64_t lrm_pileup_polish_host(const lrm_pileup_col *cols, const uint32_t *ins_words, uint32_t ins_cols, const char *content,
                                          uint64_t count, const lrm_pileup_call_options *opt, uint8_t *out, uint64_t cap) {
    PileCallRule rule;
    if (lrm_pileup_call_check(opt, &rule)) return -1;
    if (ins_cols > LRM_PILEUP_INS_COLS_MAX) { lrm_set_error("pileup: %u insertion columns, at most %d", ins_cols, LRM_PILEUP_INS_COLS_MAX); return -1; }
    if ((count && (!cols || !content || (ins_cols && !ins_words))) || (cap && !out)) { lrm_set_error("null argument"); return -1; }
    return (int64_t) pile_host_polish(cols, ins_words, ins_cols, content, count, rule, out, cap);
}

extern "C" int lrm_pileup_ins_allele_host(uint32_t depth, uint32_t n_ins, const uint32_t *ins_words, uint32_t ins_cols,
                                          const lrm_pileup_call_options *opt, lrm_pileup_ins_allele *out) {
    PileCallRule rule;
    if (lrm_pileup_call_check(opt, &rule)) return -1;
    if (ins_cols == 0 || ins_cols > LRM_PILEUP_INS_COLS_MAX) { lrm_set_error("pileup: %u insertion columns, 1 to %d", ins_cols, LRM_PILEUP_INS_COLS_MAX); return -1; }
    if (!ins_words || !out) { lrm_set_error("null argument"); return -1; }
    uint32_t w[4];
    pile_ins_allele_words(pile_ins_allele(rule, depth, n_ins, ins_words, 1u, ins_cols), w);
    memcpy(out, w, sizeof(w));
    return 0;
}

extern "C" int lrm_pileup_ins_read_dev(lrm_pileup *pl, uint64_t first, uint64_t count, uint32_t *d_out, void *stream) {
    if (!pl || (count && !d_out)) { lrm_set_error("null argument"); return -1; }
    if (pile_ins_check(pl, "pileup insertion read-back")) return -1;
    if (pile_range_check(pl->W, first, count)) return -1;
    if ((uintptr_t) d_out & 15u) { lrm_set_error("pileup insertion words must be 16-byte aligned"); return -1; }
    if (count == 0) return 0;
    if (lrm_require_device(pl->device)) return -1;
    return lrm_launch_pileup_ins_read(pl, first, count, d_out, stream);
}

extern "C" int lrm_pileup_polish_dev(lrm_pileup *pl, const lrm_pileup_call_options *opt, uint64_t first, uint64_t count, uint8_t *d_seq,
                                     uint64_t cap, uint64_t *d_len, void *stream) {
    if (!pl || !d_len || (cap && !d_seq)) { lrm_set_error("null argument"); return -1; }
    PileCallRule rule;
    if (lrm_pileup_call_check(opt, &rule)) return -1;
    if (pile_range_check(pl->W, first, count)) return -1;
    if (count * (uint64_t) (pl->ins_cols + 1u) > 0xFFFFFFFFull) { lrm_set_error("pileup polish: %llu positions of up to %u bytes in one call (byte ranks are 32-bit: below 2^32 bytes)", (unsigned long long) count, pl->ins_cols + 1u); return -1; }
    if ((uintptr_t) d_len & 7u) { lrm_set_error("the polished length must be 8-byte aligned"); return -1; }
    if (lrm_require_device(pl->device)) return -1;
    if (count == 0) {                                                  // no tile holds a position: the length is 0
        HIPCHK(hipMemsetAsync(d_len, 0, 8, (hipStream_t) stream));
        return 0;
    }
    if (lrm_pileup_call_scratch(pl)) return -1;
    return lrm_launch_pileup_polish(pl, rule, first, count, d_seq, cap, d_len, stream);
}

extern "C" int lrm_pileup_site_alleles_dev(lrm_pileup *pl, const lrm_pileup_call_options *opt, const lrm_pileup_site *d_sites, uint64_t n,
                                           lrm_pileup_ins_allele *d_out, void *stream) {
    if (!pl || (n && (!d_sites || !d_out))) { lrm_set_error("null argument"); return -1; }
    PileCallRule rule;
    if (lrm_pileup_call_check(opt, &rule)) return -1;
    if (pile_ins_check(pl, "pileup site alleles")) return -1;
    if (((uintptr_t) d_sites | (uintptr_t) d_out) & 15u) { lrm_set_error("pileup sites and alleles must be 16-byte aligned"); return -1; }
    if (n == 0) return 0;
    if (lrm_require_device(pl->device)) return -1;
    return lrm_launch_pileup_site_alleles(pl, rule, d_sites, n, d_out, stream);
}

extern "C" int lrm_debug_pileup_ins_raw(lrm_pileup *pl, uint32_t *out, uint64_t words, void *stream) {
    if (!pl || !out) { lrm_set_error("null argument"); return -1; }
    if (pile_ins_check(pl, "pileup")) return -1;
    const uint64_t held = LRM_PILEUP_INS_WORDS(pl->W, pl->ins_cols) + LRM_PILEUP_GUARD_WORDS;
    if (words > held) { lrm_set_error("pileup: the insertion planes hold %llu words", (unsigned long long) held); return -1; }
    if (lrm_require_device(pl->device)) return -1;
    HIPCHK(hipMemcpyAsync(out, pl->d_ins, 4ull * words, hipMemcpyDeviceToHost, (hipStream_t) stream));
    HIPCHK(hipStreamSynchronize((hipStream_t) stream));
    return 0;
}

// ---- the variant stage (docs/GACT_SPEC.md, "Pileup variants and VCF"; the rule: pileup_var_step.h) ----
static_assert(sizeof(lrm_pileup_variant) == 48, "lrm_pileup_variant is three 16-byte parts");
static int lrm_pileup_variant_check(const lrm_pileup_variant_options *opt, PileVarRule *rule) {
    const lrm_pileup_variant_options o = opt ? *opt : lrm_pileup_variant_options{{0, 0, 0, 0}, 0, {0, 0, 0}};
    PileCallRule call;
    if (lrm_pileup_call_check(&o.call, &call)) return -1;
    if (o.hom_pct > 100u) { lrm_set_error("pileup variants: hom_pct %u above 100", o.hom_pct); return -1; }
    if (o.reserved[0] | o.reserved[1] | o.reserved[2]) { lrm_set_error("pileup variants: lrm_pileup_variant_options.reserved is not 0"); return -1; }
    *rule = pile_var_rule(call, o.hom_pct);
    return 0;
}

extern "C" int64_t lrm_pileup_variants_host(const lrm_pileup_col *cols, const uint32_t *ins_words, uint32_t ins_cols, const char *content,
                                            uint64_t pos0, uint64_t count, const lrm_pileup_variant_options *opt, lrm_pileup_variant *out,
                                            uint64_t cap) {
    PileVarRule rule;
    if (lrm_pileup_variant_check(opt, &rule)) return -1;
    if (ins_cols > LRM_PILEUP_INS_COLS_MAX) { lrm_set_error("pileup: %u insertion columns, at most %d", ins_cols, LRM_PILEUP_INS_COLS_MAX); return -1; }
    if ((count && (!cols || !content || (ins_cols && !ins_words))) || (cap && !out)) { lrm_set_error("null argument"); return -1; }
    return (int64_t) pile_host_variants(cols, ins_words, ins_cols, content, pos0, count, rule, reinterpret_cast<uint32_t *>(out), cap);
}

extern "C" int lrm_pileup_variants_dev(lrm_pileup *pl, const lrm_pileup_variant_options *opt, uint64_t first, uint64_t count,
                                       lrm_pileup_variant *d_vars, uint64_t cap, uint64_t *d_n_vars, void *stream) {
    if (!pl || !d_n_vars || (cap && !d_vars)) { lrm_set_error("null argument"); return -1; }
    PileVarRule rule;
    if (lrm_pileup_variant_check(opt, &rule)) return -1;
    if (count > 0xFFFFFFFFull / 3u) { lrm_set_error("pileup variants: %llu positions of up to 3 records in one call (record ranks are 32-bit: below 2^32 records)", (unsigned long long) count); return -1; }
    if (pile_range_check(pl->W, first, count)) return -1;
    if ((uintptr_t) d_vars & 15u) { lrm_set_error("pileup variants must be 16-byte aligned"); return -1; }
    if ((uintptr_t) d_n_vars & 7u) { lrm_set_error("the pileup variant count must be 8-byte aligned"); return -1; }
    if (lrm_require_device(pl->device)) return -1;
    if (count == 0) {                                                  // no tile holds a position: the total is 0
        HIPCHK(hipMemsetAsync(d_n_vars, 0, 8, (hipStream_t) stream));
        return 0;
    }
    if (lrm_pileup_call_scratch(pl)) return -1;
    if (!pl->d_var) {                                                  // the stage's own two words per tile, booked once
        const LrmDevAlloc table[] = {{(void **) &pl->d_var, 8ull * pl->n_tiles}};
        if (lrm_dev_alloc_table(table, "pileup variant bytes", &pl->bytes)) return -1;
    }
    return lrm_launch_pileup_variants(pl, rule, first, count, d_vars, cap, d_n_vars, stream);
}
