// extend_stage.h -- the extension stage of liblrm_accel.so: job tables, the choice of the kernel that runs one, tile and
// LDS geometry shared by host and device, and the launchers of the stage's files
//
//   locus_kernels.hip        locus resolve + in-place reverse complement (what both modes start with)
//   gact_kernels.hip         the two byte kernels (two reads / one read per wavefront) and the launch of each
//   planar_pack_kernels.hip  bit-planar images of reads and text (bit-sliced kernel, anchor scan)
//   gact_bs_kernels.hip      the bit-sliced kernel, its expansion, its scratch
//   extend_launch.hip        parameters, plan, launch of a job table, the classic mode
//   anchor_kernels.hip       the anchored mode;  split_kernels.hip  the split stage
//   extend_taps.hip          debug taps (tests)
//
// Also read by plain C++ (lrm_split_segments for lrm_split_plan): nothing here needs the HIP runtime.
#pragma once
#include "lrm_internal.h"
#include "rival_rule.h"

#if defined(__HIPCC__)
#define LRM_HD __host__ __device__
#else
#define LRM_HD
#endif

// ---- tile geometry and walk bound (docs/GACT_SPEC.md): ONE copy for the byte kernels and the plan -------------------------
// 16-step traceback blocks of a tile: the walk never passes anti-diagonal 2(T-O)
LRM_HD static inline int lrm_gact_tb_blocks(int T, int O) { return ((2 * (T - O) - 1) >> 4) + 1; }
struct LrmGactTile { int tq, tt; bool last; };         // read / text bases of the tile; last: it reaches the read's end
// the tile anchored at (i, j) of an n x m alignment (act = false: a read that takes no tile, all zero)
LRM_HD static inline LrmGactTile lrm_gact_tile(int T, int i, int n, int j, int m, bool act = true) {
    LrmGactTile t;
    t.tq = act ? ((n - i) < T ? (n - i) : T) : 0;
    t.tt = act ? ((m - j) < T ? (m - j) : T) : 0;
    t.last = i + t.tq == n;
    return t;
}
// may the walk at (a, b) of the tile take another step?  cap = T - O bases of either sequence; the last tile runs on to
// the edge but not past anti-diagonal 2 cap
LRM_HD static inline bool lrm_gact_walk_more(const LrmGactTile &t, int a, int b, int cap) {
    return a < t.tq && b < t.tt && (t.last ? (a + b < 2 * cap) : (a < cap && b < cap));
}

// ---- dynamic LDS of the byte kernels: the kernel addresses it and the plan sizes it from the same description -------------
#define LRM_G2_PAD 40                      // guard positions on both sides of gact3_kernel's staged sequences (>= 33)
struct LrmPackedLds {                      // gact3_kernel: per wavefront a read row and a text row of packed words
    uint32_t seq_words;                    // words of a row, guards included
    LRM_HD explicit LrmPackedLds(int T) : seq_words((uint32_t) T + 2 * LRM_G2_PAD) {}
    LRM_HD size_t q_word(int wave) const { return (size_t) wave * 2 * seq_words + LRM_G2_PAD; }   // base 0 of the read row; the text row: + seq_words
    LRM_HD size_t total() const { return (size_t) 4 * 2 * seq_words * 4; }                        // 4 wavefronts
};
struct LrmWideLds {                        // gact_wide_kernel<DPL>: traceback words | read | text | the tile's op bytes
    int nx, padw, tb_words, seq_bytes, ops_bytes;
    LRM_HD LrmWideLds(int dpl, int T, int O)
        : nx(64 * dpl),                    // diagonal indices per parity
          padw(nx / 2 + 40),               // guard bytes on both sides of the staged sequences
          tb_words(lrm_gact_tb_blocks(T, O)), seq_bytes((T + 2 * padw + 15) & ~15), ops_bytes((2 * (T - O) + 15) & ~15) {}
    LRM_HD size_t tb_bytes() const { return (size_t) tb_words * nx * 4; }
    LRM_HD size_t q_off() const { return tb_bytes() + padw; }
    LRM_HD size_t d_off() const { return q_off() + seq_bytes; }
    LRM_HD size_t ops_off() const { return tb_bytes() + 2 * (size_t) seq_bytes; }
    LRM_HD size_t total() const { return ops_off() + (size_t) ops_bytes; }
};

// ---- a table of jobs, the kernel that runs it, the bit-sliced kernel's scratch (all host only) ------------------------------
#define LRM_BS_PADW 24       // planar words of padding on either side of a packed sequence
#define LRM_BS_MIN_READS 16384
// buffers for `jobs` reads of up to max_len bases whose alignments have up to 2 * ops_len ops; adds what it allocated to *bytes
int lrm_bs_scratch_alloc(LrmBsScratch *s, uint64_t jobs, uint32_t max_len, uint32_t ops_len, uint64_t *bytes);
void lrm_bs_scratch_free(LrmBsScratch *s);

struct LrmGactJobs {                       // n extension jobs: read i against the text at meta[i].loc
    const char *reads; uint64_t stride; const uint32_t *lens;
    const uint32_t *tlens;                 // null: target length = read length
    const lrm_seq_meta *meta; const int32_t *meta_r;
    const char *content;                   // the text, one byte per base
    const uint64_t *cpl;                   // its planar copy (lrm_bs_pack_text); null: none, or the text is not pure ACGT
    uint64_t n;
    uint8_t *store; uint64_t store_stride; int32_t *n_ops, *score;
};
enum LrmGactKernel {
    LRM_GACT_WIDE,                         // gact_wide_kernel, one read per wavefront
    LRM_GACT_PACKED,                       // gact3_kernel, two reads per wavefront
    LRM_GACT_BS                            // gact_bs_kernel, then gact_wide_kernel on the reads holding a byte other than ACGT
};
struct LrmGactPlan {                       // lrm_gact_plan: which kernel runs a job table
    int kernel;                            // LrmGactKernel
    int dpl;                               // gact_wide_kernel<DPL> (also the flagged reads of LRM_GACT_BS)
    int nb; bool fullband;                 // gact3_kernel<FULLBAND, NB>
    size_t lds;                            // dynamic LDS bytes of gact3_kernel (LRM_GACT_PACKED) or gact_wide_kernel
    int slot;                              // timing slot: LRM_K_GACT / LRM_K_GACT_BS
};
// "planar is available": the text has a pure-ACGT planar copy and the workspace has scratch to pack reads into
static inline bool lrm_planar_ready(const lrm_index *idx, const lrm_workspace *ws) { return idx->d_cpl && idx->cpl_ok && ws->bs.qpl; }
// extend_launch.hip.  {0,0,0} selects the default parameters; the limits are those of the kernels
int lrm_gact_resolve_params(lrm_gact_params *gp);
// THE choice of the extension kernel for a job table.  planar: lrm_planar_ready, and the scratch holds this table
int lrm_gact_plan(const LrmGactJobs &j, lrm_gact_params gp, int gact_impl, bool planar, LrmGactPlan *out);
// the launch the plan names (bs: packed reads and scratch, used by LRM_GACT_BS only; bs_waves: 0 or a smaller grid, tests;
// count: the counting build of the bit-sliced kernel)
int lrm_gact_launch_jobs(const LrmGactJobs &j, lrm_gact_params gp, const LrmGactPlan &plan, const LrmBsScratch *bs,
                         LrmDevCounters *counters, uint32_t bs_waves, bool count, void *stream);
// running a job table: the planar image of its reads (up to max_len bases) when the plan is LRM_GACT_BS, in the
// LRM_K_PACK_PLANAR slot, then lrm_gact_launch_jobs in the plan's slot.  ws: whose timing records the slots (null: none)
LRM_LOCAL int lrm_gact_run_jobs(lrm_workspace *ws, const LrmGactJobs &j, uint32_t max_len, lrm_gact_params gp,
                                const LrmGactPlan &plan, const LrmBsScratch &bs, LrmDevCounters *counters, uint32_t bs_waves,
                                void *stream);
// gact_kernels.hip: gact3_kernel<plan.fullband, plan.nb>; gact_wide_kernel<plan.dpl> (flags != null: flagged reads only)
LRM_LOCAL int lrm_gact_launch_packed(const LrmGactJobs &j, lrm_gact_params gp, const LrmGactPlan &plan, LrmDevCounters *counters,
                                     void *stream);
LRM_LOCAL int lrm_gact_launch_wide(const LrmGactJobs &j, lrm_gact_params gp, const LrmGactPlan &plan, LrmDevCounters *counters,
                                   const uint32_t *flags, void *stream);
// planar_pack_kernels.hip
uint64_t lrm_bs_planar_words(uint64_t len);
int lrm_bs_pack_reads(const char *d_reads, uint64_t stride, const uint32_t *d_lens, uint64_t n, uint32_t max_len,
                      const LrmBsScratch &bs, void *stream);
int lrm_bs_pack_text(const char *d_text, uint64_t len, uint64_t *d_out, uint32_t *d_flag, void *stream);
int lrm_bs_prepare_index(lrm_index *idx);
void lrm_bs_free_index(lrm_index *idx);
// gact_bs_kernels.hip
uint64_t lrm_bs_code_words(uint32_t max_len);
uint64_t lrm_bs_ckpt_words(uint64_t n);
int lrm_bs_launch(const LrmGactJobs &j, lrm_gact_params gp, const LrmBsScratch &bs, LrmDevCounters *counters,
                  uint32_t max_waves, bool count, void *stream);

// ---- the modes -------------------------------------------------------------------------------------------------------------
// a batch as the extension entry points receive it (device pointers; field order of the extern "C" parameter lists)
struct LrmExtendBatch {
    char *reads; uint64_t stride; const uint32_t *lens; uint64_t n; uint32_t max_len;
    const lrm_entry *best;
    uint8_t *store; uint64_t store_stride; int32_t *n_ops, *score;
    lrm_seq_meta *meta; int32_t *meta_r;
};
int lrm_launch_extend(lrm_index *idx, lrm_workspace *ws, const LrmExtendBatch &b, lrm_gact_params gp, const LrmMapTune &mt,
                      void *stream);
// locus_kernels.hip: locus_resolve + in-place reverse complement
int lrm_launch_locus_revcomp(lrm_index *idx, lrm_workspace *ws, const LrmExtendBatch &b, void *stream);
// anchored extension (anchor_kernels.hip)
#define LRM_ANCHOR_MIN_DEFAULT 20
#define LRM_CLIP_PENALTY_DEFAULT 2
#define LRM_CLIP_END_BONUS_DEFAULT 6
// end clipping (docs/GACT_SPEC.md, "End clipping"): on = 0 is the mode as it is without the step
struct LrmClipOpt { uint32_t on, penalty, end_bonus; lrm_clip *d_clip; };
static inline LrmClipOpt lrm_clip_of(const LrmMapTune &mt) { return LrmClipOpt{mt.clip, mt.clip_penalty, mt.clip_end_bonus, nullptr}; }
int lrm_launch_extend_anchored(lrm_index *idx, lrm_workspace *ws, const LrmExtendBatch &b, lrm_gact_params gp,
                               lrm_anchor *d_anchor, uint32_t min_len, const LrmClipOpt &clip, const LrmMapTune &mt, void *stream);
// 0 -> the default; -1 + message outside 12..64
LRM_LOCAL int lrm_anchor_min_len(uint32_t min_len, uint32_t *out);
// the scan over the reads at their loci into keys[b.n]; cpl: the text's planar image and pl the reads' (lrm_bs_pack_reads),
// null: from bytes
LRM_LOCAL int lrm_anchor_scan(const LrmExtendBatch &b, const LrmIndexView &ix, const LrmBsScratch &pl, const uint64_t *cpl,
                              uint32_t min_len, uint64_t *keys, void *stream);
void lrm_anchor_scratch_free(lrm_workspace *ws);
static inline uint64_t lrm_anchored_store_stride(uint32_t max_len) { return 2ull * max_len + max_len / 8 + 2; }
// split reads (split_kernels.hip; docs/GACT_SPEC.md, "Split reads")
int lrm_split_min_len(uint32_t m, uint32_t *out);          // 0 -> the default; -1 + message outside 50..2^20
// the two sides of a read of n bases from its clip counts: the left segment is R[0 .. left), the right one
// R[right_start .. right_start + right); a side shorter than M (> 0) does not qualify and has length 0.  THE rule: the
// device kernels, lrm_split_plan and the host gather all go through it
struct LrmSplitSides { uint32_t left, right_start, right; };
LRM_HD static inline LrmSplitSides lrm_split_sides(uint32_t n, uint32_t cl, uint32_t cr, uint32_t M) {
    if (cl > n) cl = n;                                    // (clip counts never exceed the read: keeps a bad input inside its row)
    if (cr > n) cr = n;
    return LrmSplitSides{cl >= M ? cl : 0u, n - cr, cr >= M ? cr : 0u};
}
// ... as the records of read i, appended at out (room for two); returns how many
LRM_HD static inline uint32_t lrm_split_segments(uint32_t read, uint32_t n, uint32_t cl, uint32_t cr, uint32_t M, lrm_segment *out) {
    const LrmSplitSides s = lrm_split_sides(n, cl, cr, M);
    uint32_t k = 0;
    if (s.left) out[k++] = lrm_segment{read, 0u, s.left, 0u};
    if (s.right) out[k++] = lrm_segment{read, s.right_start, s.right, LRM_SEG_RIGHT};
    return k;
}
struct LrmSplitArgs {                                      // lrm_split_batch_dev after its checks
    const char *reads; uint64_t stride; const uint32_t *lens; uint64_t n; const lrm_clip *clip;
    uint32_t seed_len, thres; lrm_gact_params gp;
    uint32_t anchor_min_len, clip_penalty, clip_end_bonus, split_min_len;
};
int lrm_launch_split(lrm_index *idx, lrm_workspace *ws_seg, const LrmSplitArgs &a, const lrm_split_dev &out, uint64_t *n_seg,
                     void *stream);
void lrm_split_scratch_free(lrm_workspace *ws);
// secondary alignments (secondary_kernels.hip; docs/GACT_SPEC.md, "Secondary alignments")
struct LrmSecArgs {                                        // lrm_secondary_batch_dev after its checks
    const char *reads; uint64_t stride; const uint32_t *lens; uint64_t n;
    const lrm_entry *best; const lrm_mapq *mapq;
    const lrm_seq_meta *meta; const int32_t *meta_r;       // the primary's; null: the reads are as sequenced
    uint32_t seed_len; lrm_gact_params gp;
    uint32_t min_hits, ratio_pct, anchored, anchor_min_len, clip, clip_penalty, clip_end_bonus;
};
// lrm_secondary.flags of one candidate of `len` bases from the primary's locus (has_p: there is one to compare with) and its
// own results; anchored: LRM_SEC_ALIGNED needs an anchor of the candidate's own.  THE rule: sec_flag_kernel and the
// host-buffer path both go through it
LRM_HD static inline uint32_t lrm_sec_flags(bool has_p, int32_t meta_r_p, const lrm_seq_meta &mp, int32_t meta_r, const lrm_seq_meta &m,
                                            int32_t score, uint32_t len, bool anchored, uint32_t anchor_flags) {
    uint32_t flags = 0;
    if (has_p && meta_r_p != 0 && meta_r != 0 && m.seq_id == mp.seq_id && m.strand == mp.strand) {
        const uint64_t a = m.off, b = mp.off;
        if ((a > b ? a - b : b - a) < (uint64_t) (len / 2u)) flags |= LRM_SEC_DUPLICATE;
    }
    if (meta_r != 0 && score != -1 && !flags && (!anchored || (anchor_flags & LRM_ANCHOR_ANCHORED))) flags |= LRM_SEC_ALIGNED;
    return flags;
}
// H and pct (rival_rule.h) from the caller's min_hits / ratio_pct; -1 + message for a word outside its range
static inline int lrm_rival_options(uint32_t min_hits, uint32_t ratio_pct, uint32_t *H, uint32_t *pct) {
    *H = rv_min_hits(min_hits); *pct = rv_ratio_pct(ratio_pct);
    if (*H && *pct) return 0;
    lrm_set_error("secondary: min_hits %u outside [1, 65535] or ratio_pct %u outside [1, 100]", min_hits, ratio_pct);
    return -1;
}
// the rival entries of the batch whose survivor lists are in ws, right behind lrm_launch_mapq; -1 before any launch if the
// lists are not those of (d_best, n) with the deciding phases (lrm_seed_stamp_is)
int lrm_launch_rival(lrm_index *idx, lrm_workspace *ws, const uint32_t *d_lens, uint64_t n, uint32_t seed_len, const lrm_entry *d_best,
                     const lrm_mapq *d_mapq, uint32_t min_hits, uint32_t ratio_pct, lrm_entry *d_rival, void *stream);
int lrm_launch_secondary(lrm_index *idx, lrm_workspace *ws, const LrmSecArgs &a, const lrm_secondary_dev &out, uint64_t *n_sec,
                         void *stream);
void lrm_sec_scratch_free(lrm_workspace *ws);
