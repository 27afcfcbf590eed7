// lrm_internal.h -- device image layout + internal declarations of liblrm_accel.so (the extension stage's: extend_stage.h)
//
// Device image ("blob"), designed for gfx950 gathers rather than copied from the
// reference's in-memory arrays:
//
//   [BlobHeader 256 B]
//   [occ blocks]   one 64-byte block per 64 BWT rows: for each symbol A,C,G,T a 16-byte pair
//                    u64 cnt    # of the symbol in bwt[0 .. 64*blk)       ('$' not counted)
//                    u64 mask   bit r set <=> bwt[64*blk + r] is the symbol
//                  -> one rank query == ONE aligned 16-B gather + one 64-bit popcount (the
//                     reference layout, fmidx.c:277-293, needs an 8-B o[] read plus a <=32-B
//                     byte-compare scan of bwt[] in a different array).  The '$' row sets no
//                     mask bit, so it needs no special case.
//   [lc table]     4^hlen entries of 8 bytes, k | (l-k+1) << 40 (0 = absent), indexed by the
//                  LSB-first 2-bit code of the hlen-mer (base i at bits 2i..2i+1) so the kernel
//                  extracts the index as one bit field of the packed read.  Half the footprint of
//                  the reference's {u64 k, u64 l} pairs (lchash.c:12-16): 128 MiB for hlen 12, which
//                  stays resident in the 256 MiB Infinity Cache.  Intervals of >= 2^24-1 rows are
//                  marked 0xFFFFFF and resolved through a small sorted side table [lcx].
//                  (reference order: first base most significant, lchash.c:36-49; the packer permutes.)
//   [sa]           u64 per row (values of sa_access, fmidx.c:18-33); with LRM_SA_SAMPLED=r only rows i*r
//                  (csa, fmidx.c:153-163) and the kernels locate the others by LF steps (csa_access, fmidx.c:315-331)
//   [content]      the .cat text, 1 byte per base (GACT target side)
//   [mta]          {u64 offset, u64 seq_len} per sequence (accaln.h:67-71 without names)
//
// All sections are 256-byte aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/lrm_accel.h"

#define LRM_BLOB_MAGIC 0x4c524d424c4f4232ull   // "LRMBLOB2" (2: C[] folded into the occ prefixes)
#define LRM_OCC_ROWS 64

// One LF step = ONE 16-byte gather + one 64-bit popcount: per 64 BWT rows and per symbol a
// {C[sym] + rank prefix, occurrence bitmask} pair; the four symbols of a block share a 64-byte line.
struct LrmOccEntry {
    uint64_t cnt;       // C[sym] + # of this symbol in bwt[0 .. 64*blk): an LF step is cnt + popcount(mask bits 0..r)
    uint64_t mask;      // bit r set <=> bwt[64*blk + r] is this symbol ('$' sets no bit)
};
struct LrmOccBlock { LrmOccEntry sym[4]; };
static_assert(sizeof(LrmOccBlock) == 64, "occ block must be one 64-B line");

struct LrmMtaDev { uint64_t offset, seq_len; };

struct LrmBlobHeader {
    uint64_t magic, version;
    uint64_t length;        // L = bwt rows = text bytes
    uint64_t c4[4];         // C[] for A,C,G,T  (fmidx.c:101-125)
    uint64_t dollar_row;    // row whose bwt char is '$'
    uint64_t n_blocks;
    uint64_t lc_entries;    // 4^hlen
    uint64_t sa_len, con_len;
    uint64_t off_occ, off_lc, off_sa, off_content, off_mta;
    uint64_t total_bytes;
    int32_t hlen, mta_len;
    uint64_t off_lcx, n_lcx;   // side table of {code, k, l} for intervals too long for 24 bits
    uint64_t sa_ratio;         // 0/1: [sa] holds every row; r > 1: rows i*r only (the reference's csa, fmidx.c:153-163)
    uint64_t reserved[10];
};
static_assert(sizeof(LrmBlobHeader) == 256, "header is 256 B");

// What kernels receive by value.
struct LrmIndexView {
    const LrmOccBlock *occ;
    const uint64_t *lc;       // 8-byte entries
    const uint64_t *lcx;      // {code, k, l} triples, sorted by code
    uint64_t n_lcx;
    const uint64_t *sa;
    const char *content;
    const LrmMtaDev *mta;
    uint64_t length, dollar_row, sa_len, con_len;
    uint64_t c4[4];
    int32_t hlen, mta_len;
    const uint64_t *lcl;      // optional LONG table (hl-mers, hl > hlen), built on the device from lc + FM steps; null = unused
    int32_t hl;
    int32_t sa_shift;         // log2 of the SA sampling ratio (0: every row is stored)
    int32_t lcl_pair;         // long table in PAIR-LINE layout (seed_index_dev.h): the lookups of two neighbouring seeds share a 64-byte line
    int32_t lcl_kbits;        // 0: 8-byte entries (k | count << 40).  > 0: 5-BYTE entries, k in the low lcl_kbits bits, count above
                              // (all ones = look the hl-mer up in the side hash table lclx)
    const uint64_t *core;     // optional CORE table of small texts (seed_index_dev.h): one 64-byte line per 13-mer holds the entries of
                              // the 16-mers around it, so that the lookups of FOUR neighbouring read positions share a line; null = unused
    const uint64_t *lclx;     // side hash table of the 5-byte layout: {hl-mer code + 1, k | count << 40} pairs, open addressing
    uint64_t lclx_mask;       // slots - 1 (a power of two)
    // optional SEED table (seed_index_dev.h): (first row, count) of every distinct sd_len-mer of the text in 64-byte lines shared
    // by the seeds of sd_f neighbouring read positions; null = unused
    const uint64_t *sd;
    const uint64_t *sdx;      // its side hash table {code + 1, k | count << 40}: entries of crowded lines, counts beyond the slot's bits
    uint64_t sdx_mask;
    int32_t sd_len;           // seed length it holds
    int32_t sd_f;             // read positions per line: 4 or 2
    int32_t sd_bits;          // log2 lines
    int32_t sd_kbits;         // bits of k in a slot
    int32_t sd_slot;          // slot bytes: 8 (eight per line, overflow flag in slot 0) or 6 (ten per line, entry count in the last 4 bytes)
    int32_t sd_cbits;         // count bits of a slot (all ones: the side table has the count)
    // optional presence bitmap of the seed table's lines (index_tables.hip, sd_filter_build): bit (line >> sd_filt_shift) is set iff
    // any of the 2^sd_filt_shift lines it covers holds a non-zero word; null = unused (seed_search then fetches every line)
    const uint32_t *sd_filt;
    int32_t sd_filt_shift;
};
// The seed table's usual form (E. coli- to chr1-sized texts): four positions per line, 8-byte slots, tags of at most 32 bits
// (the tag's bits as sd_key_of counts them: role 2, outside bases 6, residue = core bits - line bits).  seed_search has an
// instantiation of its own for it (SD48), and only this form gets a presence bitmap.
static inline bool lrm_sd48_form(const LrmIndexView &v) {
    return v.sd && v.sd_f == 4 && v.sd_slot == 8 && 8 + 2 * (v.sd_len - 3) - v.sd_bits <= 32;
}
// The table ends in one more line, LRM_SD_TAIL bytes of zeros (sd_build): the line that seed_search fetches for a quad whose
// bitmap bit is clear.  While the table AND that line lie below 2^32 bytes -- (2^sd_bits + 1) * 64 <= 2^32, so at most 2^25
// lines, a table of 2 GiB -- a line is addressed as the table's base plus a 32-bit byte offset (seed_search's OFF32 form);
// a longer table keeps 64-bit line addresses.
#define LRM_SD_TAIL 64
static inline bool lrm_sd_off32(const LrmIndexView &v) { return v.sd_bits <= 25; }

// ---- resolved choices of a handle ------------------------------------------------------------------------------
// Options come from the caller (lrm_index_options / lrm_map_options); LRM_* environment variables are tuning
// OVERRIDES, read ONCE when a handle is created (LrmEnv) and never per call or per launch.
struct LrmEnv {                     // the LRM_* variables as they stood when the handle was created
    static constexpr int MAXV = 32;
    const char *name[MAXV];
    long long val[MAXV];
    int n;
    bool get(const char *key, long long *out) const;
};
void lrm_env_snapshot(LrmEnv *e);
// Largest presence bitmap of the seed table's lines, KiB (LRM_SD_FILTER_KB overrides; 0: none).  Measured on the bench text
// (2^25 lines), seed_search alone: 4 MiB (one bit per line, 23.5 % set) 5.40 ms, 2 MiB (one per two lines, 41.4 %) 5.57,
// 1 MiB (65.7 %: not kept), none 6.24 - 6.44; the bench 66.6 - 66.9 / 65.7 - 66.0 / - / 62.8 - 63.7 Gbp/s (profiles/r19).
// The default goes by those times: the L2 miss counter falls by 15 % at 4 MiB and by 25 % at 2 MiB (section 1 there).
#define LRM_SD_FILTER_KB_DEFAULT 4096
struct LrmIndexTune {
    int sa_ratio;                   // 1: full SA; 2..64: sampled
    int lc_long, lc_long_max, lc_pair, lc_entry_bytes, lc_count_bits, lc_core;
    int sd, sd_len, sd_f, sd_bits, sd_cbits;      // seed table: -1 / 0 / 1, seed length, positions per line (0 automatic), tests: lines, count bits
    int sd_filter_kb;               // largest presence bitmap of the seed table's lines, KiB (LRM_SD_FILTER_KB; 0: none)
    uint64_t lcx_threshold;
};
struct LrmMapTune {
    int dense, gact_impl, seed_rounds, cigar_text, keep_reads, anchored;
    uint32_t anchor_min_len;        // 0: LRM_ANCHOR_MIN_DEFAULT
    uint32_t clip, clip_penalty, clip_end_bonus;     // end clipping of the anchored mode; 0: LRM_CLIP_*_DEFAULT
    uint32_t split, split_min_len;                   // split reads (second pass over the clipped ends); 0: LRM_SPLIT_MIN_DEFAULT
    uint32_t slice_reads, sub_batches, group_subs, bs_waves, copy_threads;
    uint32_t ss_items, ss_lds_pad, vote_vg, vote_t1, vote_u, vote_load, vote_fast;      // kernel tuning (environment only; measured defaults)
    uint32_t t3_limit, t3_slots;                                 // lrm_debug_set_vote_limits (tests)
    int ext_streams, seed_streams, verbose;
};
void lrm_resolve_index_tune(const lrm_index_options *opt, const LrmEnv &env, LrmIndexTune *out);
void lrm_resolve_map_tune(const lrm_map_options *opt, const LrmEnv &env, LrmMapTune *out);
// a caller's options struct over the defaults in *o: as many bytes as the caller's struct_size says it has (0: all)
template <typename T>
static inline void lrm_options_over_defaults(T *o, const T *opt) {
    if (opt) memcpy(o, opt, opt->struct_size && opt->struct_size < sizeof(T) ? opt->struct_size : sizeof(T));
}
// the bytes [from, to) of a caller's options struct into *o, if the caller's struct_size says it holds all of them
// (here 0 means: it holds nothing -- the rule of lrm_accaln_opt, which takes a few fields and leaves the rest)
template <typename T>
static inline void lrm_options_take_fields(T *o, const T *opt, size_t from, size_t to) {
    if (opt && opt->struct_size >= to) memcpy((char *) o + from, (const char *) opt + from, to - from);
}

struct LrmHostCtx;            // host_pipeline.h: per-handle state of the host-buffer entry points
struct lrm_index;
// the LrmMapTune of a call on a handle: the caller's options (null: the built-in defaults) under the handle's LRM_*
// overrides, then the debug vote limits (lrm_debug_set_vote_limits)
void lrm_call_map_tune(const lrm_index *ix, const lrm_map_options *opt, LrmMapTune *out);
struct lrm_index {
    void *d_blob;
    uint64_t blob_bytes;
    int owns_blob;
    int device;
    LrmBlobHeader hdr;
    LrmIndexView view;
    uint64_t *d_lcl;          // long lc table (owned; may be null)
    uint64_t *d_lclx;         // its side hash table in the 5-byte layout (owned; may be null)
    uint64_t *d_core;         // core table (owned; may be null)
    uint64_t *d_sd, *d_sdx;   // seed table and its side hash table (owned; may be null)
    uint64_t sd_side_entries; // entries of the side table (stats)
    uint32_t *d_sd_filt;      // presence bitmap of the seed table's lines (owned; may be null)
    uint64_t *d_cpl;          // planar 2-bit copy of the text for the bit-sliced GACT kernel (owned; may be null)
    int cpl_ok;               // text is pure ACGT (otherwise the byte kernels are used)
    uint64_t *d_sas;          // sampled-SA locate mode (csa_access, fmidx.c:315-331): SA rows i*sa_ratio (owned; may be null)
    LrmHostCtx *host;         // workspace, device mirrors, pinned staging and streams of the host-buffer calls (owned, lazy)
    // multi-GPU group (lrm_index_upload_multi): replica r lives on its own device; peers[0] == this.  A batch call
    // on the group handle partitions the reads by bases and runs one host thread per replica.
    int n_peers;
    lrm_index **peers;
    LrmEnv env;               // LRM_* overrides as read at creation
    LrmIndexTune itune;
    LrmMapTune mtune;         // default options of the batch calls on this handle (lrm_index_set_map_options)
    uint32_t dbg_t3_limit, dbg_t3_slots;   // lrm_debug_set_vote_limits (0 = default)
    uint32_t dbg_mapq_slots;               // lrm_debug_set_mapq_slots (0 = LRM_MAPQ_SLOTS)
};

// Per-(read,phase) vote result written by the vote kernels.
struct LrmPhaseRes {
    uint64_t key1, val1, bucket1;
    uint64_t key2, val2, bucket2;
};

// Device counters block (one per workspace).
struct LrmDevCounters {
    unsigned long long bs_queue;              // work queue of the bit-sliced GACT kernel
    unsigned long long vote_ticket[2];        // per seeding round: ticket of the exact vote kernel
    unsigned long long seed_traffic[3];       // counting build of seed_search: seeds evaluated, table lookups, rank requests
    unsigned long long reserved[2];
    unsigned long long decided_phase0;
    unsigned long long gact_tiles;
    unsigned long long pad[2];
    unsigned long long vote_fast_ticket[2];   // per seeding round: ticket of vote_fast_kernel,
    unsigned long long vote_redo_n[2];        //   items it left to the exact kernel
    unsigned long long vote_big_n[2];         //   items it left to its workgroup form, and that kernel's ticket
    unsigned long long vote_big_ticket[2];
    unsigned long long bs_count[7];           // counting build of gact_bs_kernel, LRM_BSC_*
};
// bs_count: wave-tiles (rounds of the outer loop), pass-1 step pairs whose even step was masked / plain, pass-2 blocks
// recomputed full-width / on the 32-point window / left out because no lane of the wavefront still walked, refill rounds
enum { LRM_BSC_WAVE_TILES = 0, LRM_BSC_P1_MASKED, LRM_BSC_P1_PLAIN, LRM_BSC_P2_FULL, LRM_BSC_P2_WINDOWED, LRM_BSC_P2_SKIPPED,
       LRM_BSC_REFILLS, LRM_BSC_N };
static_assert(offsetof(LrmDevCounters, decided_phase0) == 64 && sizeof(LrmDevCounters) == 216, "counters are addressed by the device as laid out here");
// Error word of a workspace: ONE dword of host-coherent pinned memory that kernels set with a plain store (bit 0:
// vote table overflow in the multi-pass tier).  It is never cleared by a launch, so an error raised by any
// sub-batch survives until the host reads it: lrm_workspace_stats and every *_dev entry point check it (the
// next call after the faulty batch fails), the host-buffer entry points check it per sub-batch.
#define LRM_ERR_VOTE_OVERFLOW 1u
// vote tiers (vote_kernels.hip): hits per (read, phase) item up to which one wavefront / one workgroup pass suffices
#define LRM_VOTE_T1_LIMIT 192
#ifndef LRM_VOTE_T3_SLOTS
#define LRM_VOTE_T3_SLOTS 1024
#endif
#define LRM_VOTE_T3_LIMIT (LRM_VOTE_T3_SLOTS * 3 / 4)
#define LRM_VOTE_GRID 1536        // resident workgroups of the vote kernel (6 per CU)
#ifndef LRM_VOTE_FAST_GRID
#define LRM_VOTE_FAST_GRID 1792   // ... of the fast vote kernel (7 per CU: its 22.6 KB of LDS per workgroup allow no more)
#endif
#define LRM_VOTE_KC_CAP 16384     // hits per workgroup whose keys the multi-pass items keep between passes (12 B each)

enum LrmKernelId { LRM_K_PACK2BIT = 0, LRM_K_SEED_SEARCH, LRM_K_VOTE, LRM_K_DECIDE,
                   LRM_K_LOCUS, LRM_K_REVCOMP, LRM_K_GACT, LRM_K_PACK_PLANAR, LRM_K_GACT_BS,
                   LRM_K_COUNT };
#define LRM_MAX_TIMED 4096

struct LrmBsScratch {                      // device scratch of the bit-sliced kernel for a number of jobs (extend_stage.h;
                                           // here because a workspace holds one by value)
    uint64_t *qpl; uint64_t wpr;           // planar reads, wpr words per read
    uint32_t *rflags;                      // per read: holds a byte other than ACGT
    uint32_t *ckpt;                        // checkpoint scratch, lrm_bs_ckpt_words(jobs) words
    uint64_t *codes; uint64_t cw;          // 2-bit CIGAR codes, cw words per read (expanded to bytes by bs_expand_kernel)
    int32_t *ncodes;                       // codes per read (the rest of n_ops is the 'I' tail)
};

#define LRM_WS_SEED 1
#define LRM_WS_EXTEND 2
struct lrm_workspace {
    lrm_index *idx;
    int parts;               // LRM_WS_SEED | LRM_WS_EXTEND: which scratch this workspace owns
    // optional per-kernel timing (HIP events recorded on the launch stream)
    int timing;
    int counting;            // seed_search and gact_bs run their counting builds (lrm_workspace_set_counting)
    int n_timed;
    void *ev_start[LRM_MAX_TIMED], *ev_stop[LRM_MAX_TIMED];
    int ev_kernel[LRM_MAX_TIMED];
    int device;
    uint64_t n_max;
    uint64_t n_last;         // reads in the last seed call (for stats)
    uint32_t max_len, seed_len, thres;
    uint32_t P;              // seed_len + 1 phases
    uint32_t cap_q;          // seeds per phase capacity
    uint64_t words_per_read; // u64 words of the 2-bit packed read (+1 guard)
    uint64_t bytes;
    // device buffers
    uint64_t *d_reads2;      // packed reads
    uint64_t *d_rec;         // survivor records k | rr << 40, compact per (read, phase): n_max * P * cap_q capacity
    uint32_t *d_recq;        // seed ordinal q of every survivor record
    uint32_t *d_cnt;         // survivors per (read, phase)
    // whose lists those are: lrm_launch_seed, the one writer of d_rec / d_recq / d_cnt / d_mq_phase, clears the stamp when it
    // starts and sets it when every launch is queued.  lrm_launch_mapq and lrm_launch_rival walk the lists only for the
    // best[] and n of the stamp, and only when that call wrote the deciding phases to d_mq_phase (lrm_seed_stamp_is)
    const lrm_entry *seeded_best;
    uint64_t seeded_n;
    int seeded_phase;
    uint64_t *d_kc_key;      // vote kernel: per-workgroup scratch of the keys of multi-pass items (LRM_VOTE_GRID x LRM_VOTE_KC_CAP)
    uint32_t *d_kc_ord;      //              ... and their order keys
    uint64_t *d_redo;        // items the fast vote kernels left to the exact one (n_max * P)
    uint64_t *d_big;         // items the wavefront form left to the workgroup form (n_max * P)
    uint64_t *d_gtab;        // pool of global-memory vote tables for items beyond the key scratch: g_slices x {key[g_slots], cf[g_slots]}
    uint32_t *d_glock;       // one lock word per slice
    uint32_t g_slices, g_slots;
    LrmPhaseRes *d_phase;    // n_max * P
    uint8_t *d_decided;      // n_max
    uint32_t *d_hcount;      // SA hits (sum of rr) per (read, phase): routes an item to its vote-table tier
    LrmDevCounters *d_counters;
    uint64_t hist_n;         // reads of the last seed launch (with the phase-0 decision count at h_err + 2: round policy)
    volatile uint32_t *h_err;   // error word (pinned host memory, 64 B block) and its device alias
    uint32_t *d_err;
    LrmBsScratch bs;         // bit-sliced GACT over up to n_max reads of up to max_len bases (LRM_WS_EXTEND)
    struct LrmAnchorScratch *an;   // anchored mode (anchor_kernels.hip): allocated by its first call on this workspace
    struct LrmCompactScratch *sp;  // split stage (split_kernels.hip, compact_rows.h): allocated by its first call with this workspace as ws_seg
    uint8_t *d_mq_phase;           // mapping quality (mapq_kernels.hip): deciding phase per read, allocated by the first mapq call
    struct LrmSecScratch *sec;     // secondary alignments (secondary_kernels.hip): allocated by the first lrm_secondary_batch_dev
};

int lrm_lcl_prepare_index(lrm_index *idx);       // index_tables.hip: the long lc table, the core table, the seed table

void lrm_set_error(const char *fmt, ...);
// internal functions that cross files without joining the library's exported symbols
#define LRM_LOCAL __attribute__((visibility("hidden")))

// THE code of a base: upper-case A, C, G, T -> 0..3, every other byte (lower case too) -> -1
static inline int base_code(char c) {
    switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}

// THE complement of a base on the host, as the device's comp_base has it (_rev_comp_in_place, alnmain.c:29-52): ACGT of
// either case -> the upper-case complement, anything else -> 'N'.  A table: the SAM formatter's hot loop looks it up per base
struct LrmCompTable {
    char t[256];
    constexpr LrmCompTable() : t() { for (int c = 0; c < 256; ++c) t[c] = 'N'; t['A'] = t['a'] = 'T'; t['C'] = t['c'] = 'G'; t['G'] = t['g'] = 'C'; t['T'] = t['t'] = 'A'; }
};
inline constexpr LrmCompTable lrm_comp_table;

// THE accessors of a suffix-array slot.  lrm_ui40 is {u32 low; u8 high} in 8 bytes (sa_use.h:17-20), 5 bytes low-first on
// disk.  This library writes a slot as one little-endian u64: the value is < 2^40, so the three padding bytes are zero and
// the slot read as a u64 is the value (HostIndex.sa() is such a view).
static_assert(sizeof(lrm_ui40) == 8, "ui40 is 8 bytes in RAM (sa_use.h:17-20)");
static inline uint64_t ui40_get(const lrm_ui40 &v) { return ((uint64_t) v.high << 32) | v.low; }
static inline void ui40_put(lrm_ui40 *slot, uint64_t v) { *reinterpret_cast<uint64_t *>(slot) = v; }

// malloc (zero: calloc) of n elements into p; false + "out of memory (what, bytes)" if there is none
template <typename T>
static inline bool lrm_alloc(T *&p, uint64_t n, const char *what, bool zero = false) {
    const size_t bytes = (size_t) (n ? n : 1) * sizeof(T);
    p = (T *) (zero ? calloc(1, bytes) : malloc(bytes));
    if (!p) lrm_set_error("out of memory (%s, %llu bytes)", what, (unsigned long long) bytes);
    return p != nullptr;
}
// OpenMP team size for the library's host loops: omp_get_max_threads() capped by the CPUs this process may really use
// (affinity mask, cgroup CPU quota) -- a GPU box hands a job 16 of its 256 hardware threads, and a team of 256 on a
// quota of 16 is throttled to a crawl.  OMP_NUM_THREADS still lowers it.
int lrm_host_threads(void);
// left / right clip of every alignment of a batch (lrm_clip_of_cigar; zeros for a read that is fenced or has score -1);
// score null: the scores in cig
LRM_LOCAL void lrm_clips_of_batch(const lrm_cigar *cig, const int *meta_r, const int *score, int is_text, uint64_t n, lrm_clip *out);
int lrm_require_device(int device);                 // hipSetDevice + "no CPU fallback" error
int lrm_workspace_create_parts(lrm_workspace **out, lrm_index *idx, uint64_t n_max, uint32_t max_len, uint32_t seed_len,
                               uint32_t thres, int parts);
int lrm_ws_take_error(lrm_workspace *ws);        // -2 + message if a kernel raised the workspace's sticky error word
void lrm_host_ctx_free(lrm_index *idx);          // host_pipeline.hip
void lrm_time_begin(lrm_workspace *ws, int kernel, void *stream);
void lrm_time_end(lrm_workspace *ws, void *stream);

// index_image.hip: a handle over an image in device memory (owns: the handle frees it); the replicas of a group are made
// with it too (index_group.hip)
int lrm_index_make_handle(lrm_index **out, void *d_blob, uint64_t bytes, int device, int owns, const LrmBlobHeader &h,
                          const lrm_index_options *opt);
// ... and pack + streamed upload of the reference's arrays to one device
int lrm_index_upload_one(lrm_index **out, const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa, const char *content,
                         uint64_t con_len, const lrm_mta_entry *mta, int mta_len, int device, const lrm_index_options *opt);

// launchers implemented in the .hip files (all asynchronous on `stream`)
// the dense result image of a unit of the host pipeline (result_pack_kernels.hip): rows of d_len[i] bytes (up to row_cap)
// to d_dense + d_off[i]; the run-length CIGAR text of every row (d_dense null: only its length, into d_tlen)
int lrm_launch_pack_rows(const uint8_t *d_src, uint64_t pitch, uint64_t row_cap, const uint32_t *d_len, const uint64_t *d_off,
                         uint8_t *d_dense, uint64_t rows, void *stream);
int lrm_launch_cigar_text(const uint8_t *d_store, uint64_t pitch, const int32_t *d_n_ops, const int32_t *d_score, const int32_t *d_meta_r,
                          uint32_t *d_tlen, const uint64_t *d_off, uint8_t *d_dense, uint64_t rows, void *stream);
// the alignment summary records (aln_summary_kernels.hip; docs/GACT_SPEC.md, "Alignment summary and PAF") of rows whose op
// bytes start at store + row * pitch (LrmOpRows, op_rows.h): behind the extension that wrote them, on its stream
struct LrmOpRows;
int lrm_launch_aln_summary(const LrmOpRows &b, lrm_aln_summary *d_out, void *stream);
// the difference events (aln_diff_kernels.hip; docs/GACT_SPEC.md, "Difference events and MD:Z") of the same rows: d_off holds
// rows + 1 exclusive prefix sums of n_x + n_del (lrm_launch_aln_diff_offsets makes them from the summary records), row i's
// events go to d_events + d_off[i]; a row whose events end behind cap writes nothing
int lrm_launch_aln_diff(const LrmOpRows &b, const char *d_content, uint64_t con_len, const uint64_t *d_off, uint64_t cap, uint32_t *d_events,
                        void *stream);
int lrm_launch_aln_diff_offsets(const lrm_aln_summary *d_sum, uint64_t rows, uint64_t *d_off, void *stream);
// the pileup (pileup_kernels.hip; docs/GACT_SPEC.md, "Pileup").  An accumulator: the counter planes of pileup_step.h over
// the window [lo, hi) (W = hi - lo positions) with LRM_PILEUP_GUARD_WORDS guard words behind them, and two words per tile
// of read-back scratch (the tiles' sums of the difference plane, then their exclusive prefix sums).  d_call: two more
// words per tile for the call stage (the tiles' site counts, then their exclusive prefix sums), allocated by the first
// lrm_pileup_sites_dev and booked into `bytes` then.
#define LRM_PILEUP_GUARD_WORDS 16u
#define LRM_PILEUP_GUARD 0xC5C5C5C5u
struct lrm_pileup {
    lrm_index *idx;
    int device;
    uint64_t lo, hi, W, n_tiles, bytes;
    uint32_t *d_planes, *d_tiles, *d_call;
    // the insertion planes of pileup_ins_step.h (lrm_pileup_create_ins): 4 * ins_cols * W words and the guard words, an
    // allocation of their own; null with ins_cols == 0
    uint32_t *d_ins, ins_cols;
    // the staging buffer of a merge from another device (lrm_pileup_merge_dev): LRM_PILEUP_MERGE_CHUNK words, allocated by the
    // first staged merge and booked into `bytes` then
    uint32_t *d_stage;
    // two more words per tile for the variant stage (the tiles' deleted-run summaries, then the run lengths that continue
    // behind each tile), allocated by the first lrm_pileup_variants_dev and booked into `bytes` then
    uint32_t *d_var;
};
#define LRM_PILEUP_MERGE_CHUNK (4ull << 20)              // words of the staging buffer (16 MiB): a multiple of 4
// the same rows as the summary and the events, plus the read rows (d_reads + row * stride, d_lens) the extension left; a
// row without an alignment, or with d_mapq[row].mapq < min_mapq (d_mapq null: no filter), adds nothing
int lrm_launch_pileup_add(const lrm_pileup *pl, const uint8_t *d_reads, uint64_t stride, const uint32_t *d_lens, const LrmOpRows &b,
                          const lrm_mapq *d_mapq, uint32_t min_mapq, void *stream);
// dst[0 .. words) += src[0 .. words), 32-bit and wrapping (pileup_merge_kernel): one launch; words == 0: nothing
int lrm_launch_pileup_merge(uint32_t *d_dst, const uint32_t *d_src, uint64_t words, void *stream);
// the records of window positions [first, first + count), count > 0: tile sums, their scan, the records
int lrm_launch_pileup_read(const lrm_pileup *pl, uint64_t first, uint64_t count, lrm_pileup_col *d_out, void *stream);
// the call stage over the same positions (docs/GACT_SPEC.md, "Pileup calls"), 0 < count < 2^32, pl->d_call allocated: tile
// sums and their scan as the read-back makes them, the tiles' site counts [and the cons bytes], their scan, the site table
struct PileCallRule;
int lrm_launch_pileup_sites(const lrm_pileup *pl, const PileCallRule &rule, uint64_t first, uint64_t count, lrm_pileup_site *d_sites,
                            uint64_t cap, uint64_t *d_n_sites, uint8_t *d_cons, void *stream);
// the insertion side (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus"): the insertion words of window
// positions [first, first + count), count > 0, position-major; the polished sequence of the same positions (0 < count,
// count * (ins_cols + 1) < 2^32, pl->d_call allocated: tile sums and their scan, the tiles' byte counts, their scan, the
// bytes); the inserted allele of every record of a site table
int lrm_launch_pileup_ins_read(const lrm_pileup *pl, uint64_t first, uint64_t count, uint32_t *d_out, void *stream);
int lrm_launch_pileup_polish(const lrm_pileup *pl, const PileCallRule &rule, uint64_t first, uint64_t count, uint8_t *d_seq, uint64_t cap,
                             uint64_t *d_len, void *stream);
int lrm_launch_pileup_site_alleles(const lrm_pileup *pl, const PileCallRule &rule, const lrm_pileup_site *d_sites, uint64_t n,
                                   lrm_pileup_ins_allele *d_out, void *stream);
// the variant stage (docs/GACT_SPEC.md, "Pileup variants and VCF"), 0 < count, 3 * count < 2^32, pl->d_call and pl->d_var
// allocated: tile sums and their scan, the tiles' record counts and run summaries, the two scans, the table
struct PileVarRule;
int lrm_launch_pileup_variants(const lrm_pileup *pl, const PileVarRule &rule, uint64_t first, uint64_t count, lrm_pileup_variant *d_vars,
                               uint64_t cap, uint64_t *d_n_vars, void *stream);
int lrm_launch_seed(lrm_index *idx, lrm_workspace *ws, const char *d_reads, uint64_t stride,
                    const uint32_t *d_lens, uint64_t n, uint32_t seed_len,
                    uint32_t thres, lrm_entry *d_best, const LrmMapTune &mt, void *stream, uint8_t *d_phase_out = nullptr);
// the vote of one seeding round over the survivor lists of the workspace (vote_kernels.hip): the fast pair plus the exact
// kernel, or the exact kernel alone
struct LrmVoteLaunch {
    const uint8_t *decided;                // reads to skip (round 1 of two); null: none
    uint64_t n; uint32_t seed_len; int phase_lo, phase_hi;
    uint32_t tbits;                        // bits of the SA offset in the order key (q << tbits) | t
    int round;                             // which ticket / list counters of LrmDevCounters
    const LrmMapTune *mt;
};
int lrm_launch_vote(lrm_index *idx, lrm_workspace *ws, const LrmVoteLaunch &v, void *stream);
// mapping quality (mapq_kernels.hip; docs/GACT_SPEC.md, "Mapping quality"): lrm_mapq_phase_buf before lrm_launch_seed (the
// deciding phase per read is that call's d_phase_out; the first call on a workspace allocates the n_max bytes),
// lrm_launch_mapq right behind it on the same stream -- the survivor lists of the workspace are still those of the batch,
// which the stamp of the workspace says: any other d_best or n, or a seed call without the phase output, is refused (-1)
uint8_t *lrm_mapq_phase_buf(lrm_workspace *ws);
// the lists and the deciding phases in ws are those lrm_launch_seed made for best[0 .. n)
static inline bool lrm_seed_stamp_is(const lrm_workspace *ws, const lrm_entry *d_best, uint64_t n) {
    return ws->seeded_phase && ws->seeded_best == d_best && ws->seeded_n == n;
}
int lrm_launch_mapq(lrm_index *idx, lrm_workspace *ws, const uint32_t *d_lens, uint64_t n, uint32_t seed_len, uint32_t thres,
                    const lrm_entry *d_best, lrm_mapq *d_mapq, void *stream);
int lrm_wait_event(void *ev);                              // host_pipeline.hip: the sleep-poll every host wait of this library uses
int lrm_launch_debug_seed(lrm_index *idx, const char *d_read, uint32_t len, uint32_t seed_len,
                          uint64_t *d_reads2, uint64_t words, int32_t *d_j, uint64_t *d_rr,
                          uint64_t *d_k, uint64_t *d_l, uint64_t cap, void *stream);
