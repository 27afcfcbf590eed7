// lrm_api.hip -- C-ABI glue of liblrm_accel.so (include/lrm_accel.h): error string, options and their LRM_* overrides,
// the device-buffer batch calls, result flags, debug taps.  (The index image is index_image.hip, group handles
// index_group.hip, workspaces workspace.hip, the accumulator of the position counts pileup.hip, the host-buffer calls
// lrm_host.hip.)
// No CPU fallback anywhere: without a HIP device every batch entry point returns an error.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
#include <sched.h>
#include <omp.h>
#include "lrm_hip_util.h"
#include "extend_stage.h"
#include "aln_diff_step.h"
#include "rival_rule.h"

static thread_local char g_err[512] = "";

void lrm_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *lrm_last_error(void) { return g_err; }
int lrm_host_threads(void) {
    // the CPUs this process may use (affinity mask, cgroup quota) are read once; the caller's OpenMP thread limit is
    // followed on every call (a host program may lower it between calls)
    static const int cap = []() {
        int m = 1 << 20;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c >= 1 && c < m) m = c; }
        long long quota = -1, period = 0;
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {                       // cgroup v2: "<quota|max> <period>"
            char q[64];
            if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
            fclose(f);
        } else {                                                                    // cgroup v1
            FILE *fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"), *fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
            if (fq && fp && fscanf(fq, "%lld", &quota) == 1 && fscanf(fp, "%lld", &period) == 1) {} else quota = -1;
            if (fq) fclose(fq);
            if (fp) fclose(fp);
        }
        if (quota > 0 && period > 0) { const int c = (int) (quota / period); if (c >= 1 && c < m) m = c; }
        return m < 1 ? 1 : m;
    }();
    const int m = omp_get_max_threads();
    const int n = m < cap ? m : cap;
    return n < 1 ? 1 : n;
}

extern "C" int lrm_abi_version(void) { return LRM_ABI_VERSION; }

extern "C" int lrm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------
// options: the caller's structs, then the LRM_* environment overrides as they stood when the handle was created
// ------------------------------------------------------------------------------------------
static const char *const k_env_names[] = {
    "LRM_SA_SAMPLED", "LRM_LC_LONG", "LRM_LC_PAIR", "LRM_LC_BYTES", "LRM_LC_CORE", "LRM_LCX_THRESHOLD", "LRM_SD", "LRM_SD_SHARE", "LRM_SD_BITS", "LRM_SD_FILTER_KB",   // index
    "LRM_GACT_IMPL", "LRM_SEED_ROUNDS", "LRM_HOST_DENSE", "LRM_HOST_SLICE", "LRM_HOST_SUBS",
    "LRM_HOST_GROUP", "LRM_BS_WAVES", "LRM_SS_ITEMS", "LRM_VOTE_VG", "LRM_VOTE_T1", "LRM_VOTE_U", "LRM_VOTE_LOAD",
    "LRM_HOST_EXT_STREAMS", "LRM_HOST_SEED_STREAMS", "LRM_HOST_VERBOSE", "LRM_VOTE_FAST", "LRM_HOST_SLOTS", "LRM_SS_PAD"};
static_assert(sizeof(k_env_names) / sizeof(k_env_names[0]) <= LrmEnv::MAXV, "LrmEnv too small");

void lrm_env_snapshot(LrmEnv *e) {
    e->n = 0;
    for (const char *name : k_env_names)
        if (const char *v = getenv(name)) {
            e->name[e->n] = name;
            e->val[e->n] = *v ? strtoll(v, nullptr, 0) : 1;            // a variable set to the empty string counts as 1
            e->n++;
        }
}
bool LrmEnv::get(const char *key, long long *out) const {
    for (int i = 0; i < n; ++i) if (strcmp(name[i], key) == 0) { *out = val[i]; return true; }
    return false;
}

extern "C" void lrm_index_options_init(lrm_index_options *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t) sizeof(*o);
    o->lc_long = -1;
    o->lc_pair = -1;
    o->lc_core = -1;
    o->seed_table = -1;
}
extern "C" void lrm_map_options_init(lrm_map_options *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t) sizeof(*o);
}

static inline bool valid_sa_ratio(long long r) { return r >= 2 && r <= 64 && (r & (r - 1)) == 0; }

// sa_sampled = r (a power of two, 2..64): keep only SA rows i*r in the image -- the reference's `csa` table
// (fmidx.c:153-163, csa_ratio 4) -- and locate the other rows by LF steps on the device (csa_access,
// fmidx.c:315-331: expected r steps per row, no fixed bound: the walk ends at a stored row or at the '$' row).
void lrm_resolve_index_tune(const lrm_index_options *opt, const LrmEnv &env, LrmIndexTune *t) {
    lrm_index_options o;
    lrm_index_options_init(&o);
    lrm_options_over_defaults(&o, opt);
    t->sa_ratio = valid_sa_ratio(o.sa_sampled) ? o.sa_sampled : 1;
    t->lc_long = o.lc_long; t->lc_long_max = o.lc_long_max; t->lc_pair = o.lc_pair;
    t->lc_entry_bytes = o.lc_entry_bytes == 5 || o.lc_entry_bytes == 8 ? (int) o.lc_entry_bytes : 0;
    t->lc_count_bits = o.lc_count_bits >= 2 && o.lc_count_bits <= 24 ? (int) o.lc_count_bits : 0;
    t->lc_core = o.lc_core;
    t->sd = o.seed_table;
    t->sd_len = o.seed_table_len >= 16 && o.seed_table_len <= 24 ? (int) o.seed_table_len : 20;        // alnmain.c:577-580: seed_len 20
    t->sd_f = o.seed_table_share == 2 || o.seed_table_share == 4 ? (int) o.seed_table_share : 0;
    t->sd_bits = o.seed_table_bits >= 4 && o.seed_table_bits <= 32 ? (int) o.seed_table_bits : 0;
    t->sd_cbits = o.seed_table_count_bits >= 2 && o.seed_table_count_bits <= 24 ? (int) o.seed_table_count_bits : 0;
    t->lcx_threshold = o.lcx_threshold >= 1 && o.lcx_threshold <= 0xFFFFFFu ? o.lcx_threshold : 0xFFFFFFull;
    long long v;
    if (env.get("LRM_SA_SAMPLED", &v)) t->sa_ratio = valid_sa_ratio(v) ? (int) v : 1;
    if (env.get("LRM_LC_LONG", &v)) t->lc_long = (int) v;
    if (env.get("LRM_LC_PAIR", &v)) t->lc_pair = v != 0;
    if (env.get("LRM_LC_BYTES", &v) && (v == 5 || v == 8)) t->lc_entry_bytes = (int) v;
    if (env.get("LRM_LC_CORE", &v)) t->lc_core = v != 0;
    if (env.get("LRM_SD", &v)) t->sd = v != 0;
    if (env.get("LRM_SD_SHARE", &v) && (v == 2 || v == 4)) t->sd_f = (int) v;
    if (env.get("LRM_SD_BITS", &v) && v >= 4 && v <= 32) t->sd_bits = (int) v;
    t->sd_filter_kb = LRM_SD_FILTER_KB_DEFAULT;
    if (env.get("LRM_SD_FILTER_KB", &v) && v >= 0 && v <= 65536) t->sd_filter_kb = (int) v;
    if (env.get("LRM_LCX_THRESHOLD", &v) && v >= 1 && v <= 0xFFFFFFll) t->lcx_threshold = (uint64_t) v;
}

void lrm_resolve_map_tune(const lrm_map_options *opt, const LrmEnv &env, LrmMapTune *t) {
    lrm_map_options o;
    lrm_map_options_init(&o);
    lrm_options_over_defaults(&o, opt);
    memset(t, 0, sizeof(*t));
    t->cigar_text = o.cigar_text != 0;
    t->dense = o.dense_results != 0 || t->cigar_text;
    t->gact_impl = o.gact_impl; t->seed_rounds = o.seed_rounds;
    t->slice_reads = o.slice_reads; t->sub_batches = o.sub_batches; t->group_subs = o.group_subs; t->bs_waves = o.bs_waves;
    t->copy_threads = o.copy_threads <= 16 ? o.copy_threads : 16;
    t->keep_reads = o.keep_reads != 0;
    t->anchored = o.anchored != 0;
    t->anchor_min_len = o.anchor_min_len;
    t->clip = o.clip != 0; t->clip_penalty = o.clip_penalty; t->clip_end_bonus = o.clip_end_bonus;
    t->split = o.split != 0; t->split_min_len = o.split_min_len;
    // measured defaults of the kernel knobs (tools/seed_probe.py sweeps them through the environment)
    t->ss_items = 2048; t->vote_vg = 16; t->vote_t1 = LRM_VOTE_T1_LIMIT; t->vote_u = 2; t->vote_load = 50; t->vote_fast = o.vote_exact_only ? 0 : 1;
    t->ext_streams = 2; t->seed_streams = 2;
    long long v;
    if (env.get("LRM_GACT_IMPL", &v)) t->gact_impl = (int) v;
    if (env.get("LRM_SEED_ROUNDS", &v)) t->seed_rounds = (int) v;
    if (env.get("LRM_HOST_DENSE", &v)) t->dense = v != 0 || t->cigar_text;
    if (env.get("LRM_HOST_SLICE", &v) && v >= 1) t->slice_reads = (uint32_t) v;
    if (env.get("LRM_HOST_SUBS", &v) && v >= 1) t->sub_batches = (uint32_t) v;
    if (env.get("LRM_HOST_GROUP", &v) && v >= 1) t->group_subs = (uint32_t) v;
    if (env.get("LRM_BS_WAVES", &v) && v >= 1) t->bs_waves = (uint32_t) v;
    if (env.get("LRM_SS_ITEMS", &v) && (v == 1024 || v == 2048 || v == 4096)) t->ss_items = (uint32_t) v;
    if (env.get("LRM_SS_PAD", &v) && v >= 0 && v <= 60000) t->ss_lds_pad = (uint32_t) v;
    if (env.get("LRM_VOTE_VG", &v) && v >= 1 && v <= 64) t->vote_vg = (uint32_t) v;
    if (env.get("LRM_VOTE_T1", &v) && v >= 0 && v <= LRM_VOTE_T1_LIMIT) t->vote_t1 = (uint32_t) v;
    if (env.get("LRM_VOTE_U", &v)) t->vote_u = (uint32_t) v;
    if (env.get("LRM_VOTE_LOAD", &v) && v >= 10 && v <= 95) t->vote_load = (uint32_t) v;
    if (env.get("LRM_VOTE_FAST", &v)) t->vote_fast = v != 0;
    if (env.get("LRM_HOST_EXT_STREAMS", &v) && v >= 1 && v <= 4) t->ext_streams = (int) v;
    if (env.get("LRM_HOST_SEED_STREAMS", &v) && v >= 1 && v <= 3) t->seed_streams = (int) v;
    if (env.get("LRM_HOST_VERBOSE", &v)) t->verbose = v != 0;
}

int lrm_require_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        lrm_set_error("no HIP device available (%s): liblrm_accel has no CPU fallback", e == hipSuccess ? "count 0" : hipGetErrorString(e));
        return -1;
    }
    if (device < 0 || device >= n) { lrm_set_error("device %d out of range (have %d)", device, n); return -1; }
    HIPCHK(hipSetDevice(device));
    return 0;
}

void lrm_call_map_tune(const lrm_index *ix, const lrm_map_options *opt, LrmMapTune *out) {
    lrm_resolve_map_tune(opt, ix->env, out);
    out->t3_limit = ix->dbg_t3_limit; out->t3_slots = ix->dbg_t3_slots;
}

// f(replica) for the handle itself, or for every replica of a group handle
template <typename F>
static void for_each_replica(lrm_index *idx, F f) {
    for (int r = 0; r < idx->n_peers; ++r) f(idx->peers ? idx->peers[r] : idx);
}

extern "C" int lrm_index_set_map_options(lrm_index *idx, const lrm_map_options *opt) {
    if (!idx) { lrm_set_error("null argument"); return -1; }
    for_each_replica(idx, [&](lrm_index *ix) { lrm_call_map_tune(ix, opt, &ix->mtune); });
    return 0;
}
// tuning sessions (tools/*_probe.py): take the LRM_* variables as they stand NOW for the batch calls of this handle
extern "C" int lrm_debug_reload_env(lrm_index *idx) {
    if (!idx) { lrm_set_error("null argument"); return -1; }
    for_each_replica(idx, [](lrm_index *ix) {
        lrm_env_snapshot(&ix->env);
        lrm_call_map_tune(ix, nullptr, &ix->mtune);
    });
    return 0;
}
extern "C" int lrm_debug_set_vote_limits(lrm_index *idx, uint32_t t3_limit, uint32_t t3_slots) {
    if (!idx) { lrm_set_error("null argument"); return -1; }
    if (t3_slots && (t3_slots < 8 || t3_slots > LRM_VOTE_T3_SLOTS)) { lrm_set_error("t3_slots outside [8, %d]", LRM_VOTE_T3_SLOTS); return -1; }
    for_each_replica(idx, [&](lrm_index *ix) {
        ix->dbg_t3_limit = ix->mtune.t3_limit = t3_limit;
        ix->dbg_t3_slots = ix->mtune.t3_slots = t3_slots;
    });
    return 0;
}

extern "C" int lrm_debug_set_mapq_slots(lrm_index *idx, uint32_t slots) {
    if (!idx) { lrm_set_error("null argument"); return -1; }
    if (slots && (slots < 16 || slots > LRM_MAPQ_SLOTS || (slots & (slots - 1u)))) {
        lrm_set_error("mapq slots %u: not a power of two in [16, %d]", slots, LRM_MAPQ_SLOTS);
        return -1;
    }
    for_each_replica(idx, [&](lrm_index *ix) { ix->dbg_mapq_slots = slots; });
    return 0;
}

// alnmain.c:554-557: the paired-end entry is declared and unimplemented in the reference ("todo"); it returns -1.
extern "C" int lrm_pair_end(int argc, const char *argv[]) { (void) argc; (void) argv; return -1; }

static int check_ws(lrm_workspace *ws, lrm_index *idx, uint64_t n, uint32_t max_len, uint32_t seed_len, uint32_t thres) {
    if (!ws || ws->idx != idx) { lrm_set_error("workspace does not belong to this index"); return -1; }
    if (n > ws->n_max || max_len > ws->max_len || seed_len != ws->seed_len || thres > ws->thres) {
        lrm_set_error("workspace too small: have n=%llu len=%u seed=%u thres=%u, need n=%llu len=%u seed=%u thres=%u",
                      (unsigned long long) ws->n_max, ws->max_len, ws->seed_len, ws->thres,
                      (unsigned long long) n, max_len, seed_len, thres);
        return -1;
    }
    return 0;
}

// d_mapq != null: the mapping-quality stage right behind the seed stage, over the lists that stage leaves in the workspace
extern "C" int lrm_seed_batch_mapq_dev(lrm_index *idx, lrm_workspace *ws, const char *d_reads, uint64_t stride,
                                       const uint32_t *d_lens, uint64_t n, uint32_t max_len, lrm_params p,
                                       lrm_entry *d_best, lrm_mapq *d_mapq, void *stream) {
    if (!idx || !d_reads || !d_lens || !d_best) { lrm_set_error("null argument"); return -1; }
    if (check_ws(ws, idx, n, max_len, p.seed_len, p.thres)) return -1;
    if (!(ws->parts & LRM_WS_SEED)) { lrm_set_error("workspace has no seed-stage scratch"); return -1; }
    if (stride < max_len) { lrm_set_error("stride %llu < max_len %u", (unsigned long long) stride, max_len); return -1; }
    if (lrm_ws_take_error(ws)) return -2;
    HIPCHK(hipSetDevice(idx->device));
    uint8_t *d_phase = nullptr;
    if (d_mapq && !(d_phase = lrm_mapq_phase_buf(ws))) return -1;
    if (int rc = lrm_launch_seed(idx, ws, d_reads, stride, d_lens, n, p.seed_len, p.thres, d_best, idx->mtune, stream, d_phase)) return rc;
    if (!d_mapq) return 0;
    return lrm_launch_mapq(idx, ws, d_lens, n, p.seed_len, p.thres, d_best, d_mapq, stream);
}
extern "C" int lrm_seed_batch_dev(lrm_index *idx, lrm_workspace *ws, const char *d_reads, uint64_t stride,
                                  const uint32_t *d_lens, uint64_t n, uint32_t max_len, lrm_params p,
                                  lrm_entry *d_best, void *stream) {
    return lrm_seed_batch_mapq_dev(idx, ws, d_reads, stride, d_lens, n, max_len, p, d_best, nullptr, stream);
}

// what the device-buffer extension entry points check before they launch
static int extend_dev_ready(lrm_index *idx, lrm_workspace *ws, const LrmExtendBatch &b) {
    if (!idx || !ws || !b.reads || !b.lens || !b.best || !b.store || !b.n_ops || !b.score || !b.meta || !b.meta_r) {
        lrm_set_error("null argument");
        return -1;
    }
    if (ws->idx != idx) { lrm_set_error("workspace does not belong to this index"); return -1; }
    if (lrm_ws_take_error(ws)) return -2;
    HIPCHK(hipSetDevice(idx->device));
    return 0;
}

extern "C" int lrm_extend_batch_dev(lrm_index *idx, lrm_workspace *ws, char *d_reads, uint64_t stride,
                                    const uint32_t *d_lens, uint64_t n, uint32_t max_len, const lrm_entry *d_best,
                                    lrm_gact_params gp, uint8_t *d_store, uint64_t store_stride, int32_t *d_n_ops,
                                    int32_t *d_score, lrm_seq_meta *d_meta, int32_t *d_meta_r, void *stream) {
    const LrmExtendBatch b = {d_reads, stride, d_lens, n, max_len, d_best, d_store, store_stride, d_n_ops, d_score, d_meta, d_meta_r};
    if (int rc = extend_dev_ready(idx, ws, b)) return rc;
    return lrm_launch_extend(idx, ws, b, gp, idx->mtune, stream);
}

extern "C" int lrm_extend_batch_anchored_dev(lrm_index *idx, lrm_workspace *ws, char *d_reads, uint64_t stride,
                                             const uint32_t *d_lens, uint64_t n, uint32_t max_len, const lrm_entry *d_best,
                                             lrm_gact_params gp, uint8_t *d_store, uint64_t store_stride, int32_t *d_n_ops,
                                             int32_t *d_score, lrm_seq_meta *d_meta, int32_t *d_meta_r, lrm_anchor *d_anchor,
                                             uint32_t min_len, void *stream) {
    const LrmExtendBatch b = {d_reads, stride, d_lens, n, max_len, d_best, d_store, store_stride, d_n_ops, d_score, d_meta, d_meta_r};
    if (int rc = extend_dev_ready(idx, ws, b)) return rc;
    return lrm_launch_extend_anchored(idx, ws, b, gp, d_anchor, min_len, LrmClipOpt{}, idx->mtune, stream);
}
extern "C" int lrm_extend_batch_clipped_dev(lrm_index *idx, lrm_workspace *ws, char *d_reads, uint64_t stride,
                                            const uint32_t *d_lens, uint64_t n, uint32_t max_len, const lrm_entry *d_best,
                                            lrm_gact_params gp, uint8_t *d_store, uint64_t store_stride, int32_t *d_n_ops,
                                            int32_t *d_score, lrm_seq_meta *d_meta, int32_t *d_meta_r, lrm_anchor *d_anchor,
                                            uint32_t min_len, uint32_t clip_penalty, uint32_t clip_end_bonus, lrm_clip *d_clip,
                                            void *stream) {
    const LrmExtendBatch b = {d_reads, stride, d_lens, n, max_len, d_best, d_store, store_stride, d_n_ops, d_score, d_meta, d_meta_r};
    if (int rc = extend_dev_ready(idx, ws, b)) return rc;
    return lrm_launch_extend_anchored(idx, ws, b, gp, d_anchor, min_len, LrmClipOpt{1, clip_penalty, clip_end_bonus, d_clip},
                                      idx->mtune, stream);
}

// ------------------------------------------------------------------------------------------
// alignment summary (docs/GACT_SPEC.md, "Alignment summary and PAF"): the rule on the host, and the device-buffer entry point
// ------------------------------------------------------------------------------------------
extern "C" void lrm_aln_summary_host(const uint8_t *ops, int n_ops, lrm_aln_summary *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    if (!ops || n_ops <= 0) return;
    int first = -1, last = -1;                                       // the first and the last column that is not 'S'
    uint8_t before = 0;                                              // the column before this one; column -1 is no op
    for (int i = 0; i < n_ops; ++i) {
        const uint8_t o = ops[i];
        switch (o) {
            case '=': out->n_eq++; break;
            case 'X': out->n_x++; break;
            case 'I': out->n_ins++; out->ins_runs += before != 'I'; break;
            case 'D': out->n_del++; out->del_runs += before != 'D'; break;
            default: break;                                          // 'S', or a byte outside the alphabet: counted nowhere
        }
        if (o != 'S') { if (first < 0) first = i; last = i; }
        before = o;
    }
    out->clip_left = first < 0 ? (uint32_t) n_ops : (uint32_t) first;
    out->clip_right = first < 0 ? 0u : (uint32_t) (n_ops - 1 - last);
}

extern "C" int lrm_aln_summary_dev(lrm_index *idx, const uint8_t *d_store, uint64_t store_stride, const int32_t *d_n_ops,
                                   const int32_t *d_score, const int32_t *d_meta_r, uint64_t n, lrm_aln_summary *d_out, void *stream) {
    if (!idx || (n && (!d_store || !d_n_ops || !d_score || !d_meta_r || !d_out))) { lrm_set_error("null argument"); return -1; }
    if ((uintptr_t) d_out & 15u) { lrm_set_error("alignment summary records must be 16-byte aligned"); return -1; }
    if (lrm_require_device(idx->device)) return -1;
    return lrm_launch_aln_summary(LrmOpRows{d_store, store_stride, d_n_ops, d_score, d_meta_r, nullptr, n}, d_out, stream);
}

// ------------------------------------------------------------------------------------------
// difference events (docs/GACT_SPEC.md, "Difference events and MD:Z"): the rule on the host, and the device-buffer entry points
// ------------------------------------------------------------------------------------------
// The host rule is aln_diff_step.h's: the row walked as a lane of aln_diff_kernel walks it, through diff_word_step.
extern "C" int64_t lrm_aln_diff_host(const uint8_t *ops, int n_ops, const uint8_t *target, uint64_t target_len, uint32_t *events_out) {
    if (!ops || n_ops <= 0) return 0;
    return (int64_t) diff_host_events(ops, (uint64_t) n_ops, target, target ? target_len : 0, events_out);
}

extern "C" int lrm_aln_diff_offsets_dev(const lrm_aln_summary *d_summary, uint64_t n, uint64_t *d_off, void *stream) {
    if (!d_off || (n && !d_summary)) { lrm_set_error("null argument"); return -1; }
    return lrm_launch_aln_diff_offsets(d_summary, n, d_off, stream);
}

extern "C" int lrm_aln_diff_dev(lrm_index *idx, const uint8_t *d_store, uint64_t store_stride, const int32_t *d_n_ops,
                                const int32_t *d_score, const int32_t *d_meta_r, const lrm_seq_meta *d_meta, uint64_t n,
                                const uint64_t *d_off, uint64_t cap, uint32_t *d_events, void *stream) {
    if (!idx || (n && (!d_store || !d_n_ops || !d_score || !d_meta_r || !d_meta || !d_off)) || (cap && !d_events)) { lrm_set_error("null argument"); return -1; }
    if (store_stride > LRM_DIFF_MAX_STRIDE) { lrm_set_error("difference events: store_stride %llu above 2^22 (the '=' count of an event has 22 bits)", (unsigned long long) store_stride); return -1; }
    if ((uintptr_t) d_events & 3u) { lrm_set_error("difference events must be 4-byte aligned"); return -1; }
    if (lrm_require_device(idx->device)) return -1;
    return lrm_launch_aln_diff(LrmOpRows{d_store, store_stride, d_n_ops, d_score, d_meta_r, d_meta, n}, idx->view.content, idx->view.con_len, d_off,
                               cap, d_events, stream);
}

// ------------------------------------------------------------------------------------------
// split reads (docs/GACT_SPEC.md, "Split reads"): the rule on the host, and the device-buffer entry point
// ------------------------------------------------------------------------------------------
int lrm_split_min_len(uint32_t m, uint32_t *out) {
    if (m == 0) m = LRM_SPLIT_MIN_DEFAULT;
    if (m < 50 || m > (1u << 20)) { lrm_set_error("split_min_len %u outside [50, 2^20]", m); return -1; }
    *out = m;
    return 0;
}

extern "C" int lrm_split_plan(const uint32_t *lens, const lrm_clip *clip, uint64_t n, uint32_t split_min_len,
                              lrm_segment *seg_out, uint64_t cap, uint64_t *n_seg) {
    uint32_t M;
    if (!n_seg || (n && (!lens || !clip)) || (cap && !seg_out)) { lrm_set_error("null argument"); return -1; }
    if (n > 0xFFFFFFFFull) { lrm_set_error("batch too large"); return -1; }
    if (lrm_split_min_len(split_min_len, &M)) return -1;
    uint64_t total = 0;
    lrm_segment two[2];
    for (uint64_t i = 0; i < n; ++i) total += lrm_split_segments((uint32_t) i, lens[i], clip[i].left, clip[i].right, M, two);
    *n_seg = total;
    if (total > cap) {
        lrm_set_error("%llu segments, room for %llu", (unsigned long long) total, (unsigned long long) cap);
        return -3;
    }
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) at += lrm_split_segments((uint32_t) i, lens[i], clip[i].left, clip[i].right, M, seg_out + at);
    return 0;
}

extern "C" int lrm_clip_of_cigar(const lrm_cigar *cig, int is_text, uint32_t *left, uint32_t *right) {
    if (!cig || !left || !right) { lrm_set_error("null argument"); return -1; }
    *left = *right = 0;
    if (cig->n_cigar_op <= 0 || !cig->cigar) return 0;
    if (!is_text) {
        const uint8_t *o = cig->cigar;
        const int k = cig->n_cigar_op;
        int l = 0, r = 0;
        while (l < k && o[l] == 'S') ++l;
        while (r < k - l && o[k - 1 - r] == 'S') ++r;
        *left = (uint32_t) l; *right = (uint32_t) r;
        return 0;
    }
    // run-length text: <count><op>...; the first run and the last run
    const char *t = (const char *) cig->cigar;
    uint64_t run = 0, first = 0, last = 0;
    int runs = 0;
    char last_op = 0;
    for (const char *c = t; *c; ++c) {
        if (*c >= '0' && *c <= '9') { run = run * 10 + (uint64_t) (*c - '0'); continue; }
        if (runs == 0 && *c == 'S') first = run;
        last = run; last_op = *c;
        ++runs;
        run = 0;
    }
    *left = (uint32_t) first;
    if (runs > 1 && last_op == 'S') *right = (uint32_t) last;
    return 0;
}

void lrm_clips_of_batch(const lrm_cigar *cig, const int *meta_r, const int *score, int is_text, uint64_t n, lrm_clip *out) {
    for (uint64_t i = 0; i < n; ++i) {
        out[i].left = out[i].right = 0;
        if (meta_r[i] != 0 && (score ? score[i] : cig[i].score) != -1) (void) lrm_clip_of_cigar(&cig[i], is_text, &out[i].left, &out[i].right);
    }
}

extern "C" int lrm_split_batch_dev(lrm_index *idx, lrm_workspace *ws_seg, const char *d_reads, uint64_t stride,
                                   const uint32_t *d_lens, uint64_t n, const lrm_clip *d_clip, lrm_params p, lrm_gact_params gp,
                                   uint32_t anchor_min_len, uint32_t clip_penalty, uint32_t clip_end_bonus, uint32_t split_min_len,
                                   const lrm_split_dev *out, uint64_t *n_seg, void *stream) {
    if (!idx || !ws_seg || !out || !n_seg || (n && (!d_reads || !d_lens || !d_clip))) { lrm_set_error("null argument"); return -1; }
    *n_seg = 0;
    if (out->cap && (!out->seg || !out->rows || !out->lens || !out->best || !out->store || !out->n_ops || !out->score || !out->meta ||
                     !out->meta_r || !out->anchor || !out->clip)) { lrm_set_error("null array in lrm_split_dev"); return -1; }
    if (n > 0x7fffffffull) { lrm_set_error("batch too large"); return -1; }
    if (ws_seg->idx != idx) { lrm_set_error("workspace does not belong to this index"); return -1; }
    if ((ws_seg->parts & (LRM_WS_SEED | LRM_WS_EXTEND)) != (LRM_WS_SEED | LRM_WS_EXTEND)) { lrm_set_error("segment workspace needs seed and extension scratch"); return -1; }
    if (p.seed_len != ws_seg->seed_len || p.thres > ws_seg->thres) {
        lrm_set_error("segment workspace was made for seed=%u thres=%u, the batch has seed=%u thres=%u", ws_seg->seed_len, ws_seg->thres, p.seed_len, p.thres);
        return -1;
    }
    if (out->cap && (((uintptr_t) out->rows | out->row_stride) & 15u)) { lrm_set_error("segment rows must be 16-byte aligned, row_stride a multiple of 16"); return -1; }
    if (out->cap && (out->store_stride & 3u)) { lrm_set_error("segment store_stride must be a multiple of 4"); return -1; }
    LrmSplitArgs a = {d_reads, stride, d_lens, n, d_clip, p.seed_len, p.thres, gp, anchor_min_len, clip_penalty, clip_end_bonus, 0};
    if (lrm_split_min_len(split_min_len, &a.split_min_len)) return -1;
    if (lrm_ws_take_error(ws_seg)) return -2;
    HIPCHK(hipSetDevice(idx->device));
    if (n == 0) return 0;
    return lrm_launch_split(idx, ws_seg, a, *out, n_seg, stream);
}

// ------------------------------------------------------------------------------------------
// secondary alignments (docs/GACT_SPEC.md, "Secondary alignments"): the rules on the host, and the device-buffer entry points
// ------------------------------------------------------------------------------------------
// The host rule sorts where the kernel hashes: the hits outside the winner's window as (bucket << 1 | histogram) words,
// their runs are the pairs; then the offsets of the fullest pair's hits, their runs per sub-bucket.
extern "C" int lrm_rival_host(const uint64_t *keys, uint64_t n_keys, const lrm_entry *best, uint32_t len, uint32_t min_hits,
                              uint32_t ratio_pct, uint32_t slots, lrm_entry *out) {
    if (!out || !best || (n_keys && !keys)) { lrm_set_error("null argument"); return -1; }
    uint32_t H, pct;
    if (lrm_rival_options(min_hits, ratio_pct, &H, &pct)) return -1;
    if (slots == 0) slots = LRM_MAPQ_SLOTS;
    out->key = out->val = out->bucket = 0;
    if (best->val == 0) return 0;
    const uint32_t r = mq_radius_log2(len);
    struct Pair { uint64_t bucket; uint32_t h; uint64_t key; };
    std::vector<Pair> hits;
    uint32_t n1 = 0;
    for (uint64_t i = 0; i < n_keys; ++i) {
        if (mq_inside(keys[i], best->key, r)) { ++n1; continue; }
        for (uint32_t h = 0; h < 2; ++h) hits.push_back(Pair{mq_bucket(keys[i], r, h), h, keys[i]});
    }
    std::sort(hits.begin(), hits.end(), [](const Pair &a, const Pair &b) { return a.bucket != b.bucket ? a.bucket < b.bucket : a.h < b.h; });
    uint64_t pairs = 0, lo = 0, n2 = 0;                       // the first fullest run in (bucket, histogram) order
    for (uint64_t i = 0, j; i < hits.size(); i = j, ++pairs) {
        for (j = i + 1; j < hits.size() && hits[j].bucket == hits[i].bucket && hits[j].h == hits[i].h; ++j) {}
        if (j - i > n2) { n2 = j - i; lo = i; }
    }
    const uint32_t flags = pairs > slots ? LRM_MAPQ_OVERFLOW : 0u;
    if (!rv_candidate(n1, flags ? n1 : (uint32_t) n2, flags, H, pct)) return 0;
    const uint32_t s = rv_sub_shift(r), h = hits[lo].h;
    std::vector<uint32_t> offs;
    for (uint64_t i = lo; i < lo + n2; ++i) offs.push_back(rv_off(hits[i].key, r, h));
    std::sort(offs.begin(), offs.end());
    uint64_t best_at = 0, best_n = 0;
    for (uint64_t i = 0, j; i < offs.size(); i = j) {
        for (j = i + 1; j < offs.size() && (offs[j] >> s) == (offs[i] >> s); ++j) {}
        if (j - i > best_n) { best_n = j - i; best_at = i; }
    }
    out->key = rv_key_of(mq_tag(hits[lo].key, r, h), r, offs[best_at]);
    out->val = best_n;
    out->bucket = out->key >> 4;
    return 1;
}

extern "C" int lrm_secondary_plan(const lrm_mapq *mapq, uint64_t n, uint32_t min_hits, uint32_t ratio_pct, lrm_secondary *table,
                                  uint64_t cap, uint64_t *n_sec) {
    if (!n_sec || (n && !mapq) || (cap && !table)) { lrm_set_error("null argument"); return -1; }
    if (n > 0xFFFFFFFFull) { lrm_set_error("batch too large"); return -1; }
    uint32_t H, pct;
    if (lrm_rival_options(min_hits, ratio_pct, &H, &pct)) return -1;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) total += rv_candidate(mapq[i].n1, mapq[i].n2, mapq[i].flags, H, pct) != 0;
    *n_sec = total;
    if (total > cap) {
        lrm_set_error("%llu secondary candidates, room for %llu", (unsigned long long) total, (unsigned long long) cap);
        return -3;
    }
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (rv_candidate(mapq[i].n1, mapq[i].n2, mapq[i].flags, H, pct)) table[at++] = lrm_secondary{(uint32_t) i, 0u, 0u, 0u};
    return 0;
}

extern "C" int lrm_rival_dev(lrm_index *idx, lrm_workspace *ws, const uint32_t *d_lens, uint64_t n, lrm_params p,
                             const lrm_entry *d_best, const lrm_mapq *d_mapq, uint32_t min_hits, uint32_t ratio_pct,
                             lrm_entry *d_rival, void *stream) {
    if (!idx || !ws || (n && (!d_lens || !d_best || !d_mapq || !d_rival))) { lrm_set_error("null argument"); return -1; }
    if (ws->idx != idx) { lrm_set_error("workspace does not belong to this index"); return -1; }
    if ((uintptr_t) d_mapq & 15u) { lrm_set_error("mapping-quality records must be 16-byte aligned"); return -1; }
    if (lrm_ws_take_error(ws)) return -2;
    HIPCHK(hipSetDevice(idx->device));
    return lrm_launch_rival(idx, ws, d_lens, n, p.seed_len, d_best, d_mapq, min_hits, ratio_pct, d_rival, stream);
}

extern "C" int lrm_secondary_batch_dev(lrm_index *idx, lrm_workspace *ws, const char *d_reads, uint64_t stride, const uint32_t *d_lens,
                                       uint64_t n, const lrm_entry *d_best, const lrm_mapq *d_mapq, const lrm_seq_meta *d_meta,
                                       const int32_t *d_meta_r, lrm_params p, lrm_gact_params gp, const lrm_secondary_options *so,
                                       const lrm_secondary_dev *out, uint64_t *n_sec, void *stream) {
    if (!idx || !ws || !out || !n_sec || (n && (!d_reads || !d_lens || !d_best || !d_mapq))) { lrm_set_error("null argument"); return -1; }
    *n_sec = 0;
    if ((d_meta == nullptr) != (d_meta_r == nullptr)) { lrm_set_error("secondary: d_meta and d_meta_r come together"); return -1; }
    lrm_secondary_options o;
    memset(&o, 0, sizeof(o));
    lrm_options_over_defaults(&o, so);
    const uint32_t anchored = o.anchored || o.clip;
    if (out->cap && (!out->table || !out->rows || !out->lens || !out->rival || !out->store || !out->n_ops || !out->score || !out->meta ||
                     !out->meta_r || (anchored && !out->anchor) || (o.clip && !out->clip))) { lrm_set_error("null array in lrm_secondary_dev"); return -1; }
    if (n > 0x7fffffffull) { lrm_set_error("batch too large"); return -1; }
    if (ws->idx != idx) { lrm_set_error("workspace does not belong to this index"); return -1; }
    if ((ws->parts & (LRM_WS_SEED | LRM_WS_EXTEND)) != (LRM_WS_SEED | LRM_WS_EXTEND)) { lrm_set_error("secondary: the workspace needs seed and extension scratch"); return -1; }
    if (out->cap && (((uintptr_t) out->rows | out->row_stride | (uintptr_t) out->table) & 15u)) { lrm_set_error("secondary: table and rows must be 16-byte aligned, row_stride a multiple of 16"); return -1; }
    if (out->cap && (out->store_stride & 3u)) { lrm_set_error("secondary: store_stride must be a multiple of 4"); return -1; }
    if ((uintptr_t) d_mapq & 15u) { lrm_set_error("mapping-quality records must be 16-byte aligned"); return -1; }
    const LrmSecArgs a = {d_reads, stride, d_lens, n, d_best, d_mapq, d_meta, d_meta_r, p.seed_len, gp, o.min_hits, o.ratio_pct, anchored,
                          o.anchor_min_len, o.clip, o.clip_penalty, o.clip_end_bonus};
    if (lrm_ws_take_error(ws)) return -2;
    HIPCHK(hipSetDevice(idx->device));
    if (n == 0) return 0;
    return lrm_launch_secondary(idx, ws, a, *out, n_sec, stream);
}

extern "C" void lrm_result_flags(const int *score, const int *meta_r, const lrm_seq_meta *meta, uint64_t n,
                                 int *flag_out, int *mapq_out, int *valid_out) {
    for (uint64_t i = 0; i < n; ++i) {                     // alnmain.c:460-474
        int flag = 0, mapq = 255, valid = score[i] >= 0;
        if (meta_r[i] == 0 || score[i] == -1) { valid = 0; flag += 0x4; mapq = 0; }
        else if (meta[i].strand == 1) flag += 16;
        flag_out[i] = flag; mapq_out[i] = mapq; valid_out[i] = valid;
    }
}
extern "C" void lrm_result_flags_mapq(const int *score, const int *meta_r, const lrm_seq_meta *meta, const lrm_mapq *mq, uint64_t n,
                                      int *flag_out, int *mapq_out, int *valid_out) {
    lrm_result_flags(score, meta_r, meta, n, flag_out, mapq_out, valid_out);
    if (!mq) return;
    for (uint64_t i = 0; i < n; ++i)
        if (mapq_out[i] != 0) mapq_out[i] = mq[i].mapq;        // mapped reads: the record's value instead of 255
}

// ------------------------------------------------------------------------------------------
// debug taps (tests only)
// ------------------------------------------------------------------------------------------
extern "C" int lrm_debug_seed_search(lrm_index *idx, const char *read, uint32_t len, uint32_t seed_len, uint32_t thres,
                                     int32_t *j_out, uint64_t *rr_out, uint64_t *k_out, uint64_t *l_out, uint64_t cap,
                                     uint64_t *n_out) {
    (void) thres;
    if (!idx || !read || !n_out) { lrm_set_error("null argument"); return -1; }
    if (seed_len < 1 || seed_len > 32) { lrm_set_error("seed_len %u outside [1,32]", seed_len); return -1; }
    if (lrm_require_device(idx->device)) return -1;
    uint64_t words = (uint64_t) len / 32 + 2;
    DevBuf d_read, d_r2, d_j, d_rr, d_k, d_l;
    if (d_read.alloc(len + 1) || d_r2.alloc((words + 1) * 8) || d_j.alloc(cap * 4) || d_rr.alloc(cap * 8) ||
        d_k.alloc(cap * 8) || d_l.alloc(cap * 8)) { lrm_set_error("device allocation failed"); return -1; }
    HIPCHK(hipMemcpy(d_read.p, read, len, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_j.p, 0xff, cap * 4));
    int cap_q = lrm_launch_debug_seed(idx, (const char *) d_read.p, len, seed_len, (uint64_t *) d_r2.p, words,
                                      (int32_t *) d_j.p, (uint64_t *) d_rr.p, (uint64_t *) d_k.p, (uint64_t *) d_l.p,
                                      cap, nullptr);
    if (cap_q < 0) return -1;
    HIPCHK(hipDeviceSynchronize());
    uint64_t total = (uint64_t) cap_q * (seed_len + 1);
    HIPCHK(hipMemcpy(j_out, d_j.p, total * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rr_out, d_rr.p, total * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(k_out, d_k.p, total * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(l_out, d_l.p, total * 8, hipMemcpyDeviceToHost));
    *n_out = total;
    return cap_q;
}
