/*
 * lrm_accel.h -- C-ABI of liblrm_accel.so, the MI355X (gfx950) implementation
 * of the seed-and-extend hot path of lisanhu/LongReadMapper (accaln).
 *
 * Everything here is extern "C", plain pointers and sizes.  The entry points
 * are what a maintainer of the reference binds in alnmain.c instead of the
 * per-read CPU loops (see INTEGRATION.md for the patch):
 *
 *   reference (file:line, relative to the reference tree)      replaced by
 *   ---------------------------------------------------------  ------------------
 *   init(): index arrays resident in host RAM                   lrm_index_upload
 *     alnmain.c:179-256, fmidx.h:16-28, lchash.h:16-20
 *   PART 1 seed + vote loop, alnmain.c:333-405                  lrm_seed_batch
 *     lc_aln lchash.h:25-27, fmi_aln fmidx.h:37-38,
 *     sa_access fmidx.h:30, histo_* histo.h:32-37
 *   PART 2 locus resolve + rev-comp + extension,                lrm_extend_batch
 *     alnmain.c:408-451, cigar_align mutils.h:57-58
 *   PART 1 + PART 2 in one device pass (one upload per batch)   lrm_map_batch
 *   the batch loop with its planned copy clauses,                lrm_map_batch_submit / lrm_map_batch_wait
 *     alnmain.c:302-330, 420-424 (batches overlap on the device)
 *   params (run-time options), alnmain.h:10-13,                  lrm_index_options / lrm_map_options
 *     alnmain.c:574-588
 *   PART 3 result flags, alnmain.c:458-477                      lrm_result_flags (lrm_result_flags_mapq: a real MAPQ)
 *   (no counterpart: the reference prints neither NM nor MD)     lrm_aln_summary_dev, lrm_aln_diff_dev (lrm_md_format: MD:Z)
 *   (no counterpart: the reference has no per-position output)   lrm_pileup_create, lrm_pileup_add_dev, lrm_pileup_read_dev,
 *                                                                  lrm_pileup_sites_dev, lrm_pileup_create_ins, lrm_pileup_polish_dev;
 *                                                                  on host buffers lrm_map_batch_submit_ex3 (lrm_batch_pileup), one
 *                                                                  accumulator per replica, lrm_pileup_merge_dev
 *   context_destroy(), accaln.c:7-43                            lrm_index_free
 *   host batch loop over devices, alnmain.c:302-330             lrm_index_upload_multi (+ the same batch calls)
 *   pair_end(), alnmain.c:554-557 (unimplemented, returns -1)   lrm_pair_end
 *
 * Struct mirrors keep the reference's field order so the reference's own
 * objects can be passed by pointer cast (dna_fmi*, lc_hash*, entry*, params).
 *
 * There is NO CPU fallback: every batch call fails (negative return,
 * lrm_last_error()) when no gfx950 device / code object is available.
 *
 * Return convention: 0 = ok, <0 = error (message via lrm_last_error()).
 * Data-level conventions of the reference are preserved: 0 seed hits, score
 * -1 = alignment failure, meta_r 0 = locus outside every sequence.
 */
#ifndef LRM_ACCEL_H
#define LRM_ACCEL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRM_ABI_VERSION 3

/* histo/histo.h:21-23 `entry` */
typedef struct lrm_entry { uint64_t key, val, bucket; } lrm_entry;

/* alnmain.h:10-13 `params` */
typedef struct lrm_params { uint64_t batch_size; uint32_t seed_len, thres; } lrm_params;

/* fmidx/fmidx.h:16-21 `dna_fmi` (identical field order) */
typedef struct lrm_dna_fmi {
    uint64_t length, o_len, csa_len;
    uint64_t *c, *o, *csa;
    int o_ratio, csa_ratio;
    char *bwt;
} lrm_dna_fmi;

/* lchash/lchash.h:16-20 `lc_hash` */
typedef struct lrm_lc_hash { uint64_t *lc; uint64_t len; int hlen; } lrm_lc_hash;

/* psascan/sa_use.h:17-20 `ui40_t` as it sits in RAM (8 bytes with padding) and
 * fmidx/fmidx.h:23-26 `sa_mem` */
typedef struct lrm_ui40 { uint32_t low; uint8_t high; } lrm_ui40;
typedef struct lrm_sa_mem { uint64_t start, len; lrm_ui40 *mem; } lrm_sa_mem;

/* accaln.h:67-71 `mta_entry` flattened: {mstring seq_name{l,s,own}; offset; seq_len} */
typedef struct lrm_mta_entry {
    uint64_t name_len; char *name; int name_own;
    uint64_t offset; size_t seq_len;
} lrm_mta_entry;

/* alnmain.c:143-148 `seq_meta`; g_name is returned as the index of the mta entry */
typedef struct lrm_seq_meta { uint64_t loc, off; int32_t seq_id; uint8_t strand; } lrm_seq_meta;

/* gact `cigar` as used at mutils.c:97-103 / alnmain.c:314-325: one op byte per
 * alignment column ('=' 'X' 'I' 'D'; 'S' at the two ends only with lrm_map_options.clip) in a caller-owned buffer */
typedef struct lrm_cigar { uint8_t *cigar; int n_cigar_op; int score; } lrm_cigar;

/* GACT tile / overlap / band (docs/GACT_SPEC.md); {0,0,0} selects the defaults */
typedef struct lrm_gact_params { int T, O, W; } lrm_gact_params;
#define LRM_GACT_T_DEFAULT 320
#define LRM_GACT_O_DEFAULT 120
#define LRM_GACT_W_DEFAULT 128

typedef struct lrm_index lrm_index;       /* opaque: device-resident index */

/* ---------------------------------------------------------------------------
 * Run-time options (the reference's run-time surface is `params`, alnmain.h:10-13, filled from argv at
 * alnmain.c:574-588; what is a choice of THIS implementation lives in the two structs below).
 * Initialise with lrm_*_options_init (sets struct_size and the automatic choices), change fields, pass by pointer;
 * NULL means "all automatic".  LRM_* environment variables remain as OVERRIDES for tuning sessions only: they are
 * read once, when a handle is created, never per call.
 * ------------------------------------------------------------------------- */
typedef struct lrm_index_options {
    uint32_t struct_size;      /* sizeof(lrm_index_options) of the caller's header */
    int32_t sa_sampled;        /* 0 / 1: the full suffix array (sa_access, fmidx.c:18-33); r = 2..64, a power of two: only
                                  rows i*r stay on the device -- r = 4 is the reference's csa table, fmidx.c:153-163 -- and the
                                  kernels locate the other rows by LF steps (csa_access, fmidx.c:315-331): GRCh38 49.6 -> 12.4 GB */
    int32_t lc_long;           /* k-mer length of the long seed table derived on the device: -1 automatic (the longest that
                                  leaves room in HBM), 0 none (lchash alone, lchash.c:89-104), 13..17 */
    int32_t lc_long_max;       /* cap on the automatic choice (0: none): the 64 GiB 16-mer table costs 0.7-2 s at upload, a
                                  caller that knows its run is short says 15 */
    int32_t lc_pair;           /* layout of the long table: -1 automatic (pair-line), 0 plain, 1 pair-line */
    uint32_t lcx_threshold;    /* 0: default (2^24 - 1); lchash intervals of at least this many rows go through the side
                                  table (tests) */
    uint32_t lc_entry_bytes;   /* entries of the long table: 0 automatic, 8, or 5 (pair-line layout only: 40 bytes per
                                  (k-1)-mer instead of 64 -- pair-line 17-mers of a GRCh38-sized text in 160 GiB; counts that
                                  do not fit the 40 - ceil(log2(rows)) count bits go through a side hash table) */
    int32_t lc_core;           /* core table (texts of up to 2^25 rows, next to pair-line 16-mers): one 64-byte line per 13-mer holds
                                  the entries of the 16-mers around it, the lookups of FOUR neighbouring read positions share it
                                  (4 GiB): -1 automatic, 0 off, 1 on */
    uint32_t lc_count_bits;    /* tests: count bits of the 5-byte entries (0: 40 - ceil(log2(rows))); a small value sends
                                  ordinary repeats through the side hash table */
    int32_t seed_table;        /* SEED table: a hash table of the text's seed_table_len-mers -- (first row, count) of every distinct one,
                                  the exact result of lc_aln + fmi_aln (lchash.c:89-104, fmidx.c:295-313) for it -- in 64-byte lines
                                  that the seeds of 4 (or 2) neighbouring read positions share: a seed of that length costs a quarter
                                  (half) of a memory line and no backward step; a 20-mer that occurs once carries its text position
                                  (sa_access of its row, fmidx.c:18-33), so the vote stage gathers nothing for it.  -1 automatic (pure ACGT texts, when HBM allows: 2 GiB
                                  for an E. coli-sized text, 64 GiB chr1-sized, 128 GiB GRCh38-sized), 0 off, 1 on.  Seeds of any
                                  other length go through the tables above. */
    uint32_t seed_table_len;   /* seed length the table is built for: 0 = 20, the reference's default (alnmain.c:577-580); 16..24 */
    uint32_t seed_table_share; /* read positions per line: 0 automatic, 4 (8-byte slots, eight per line) or 2 (6-byte slots, ten) */
    uint32_t seed_table_bits;  /* tests: log2 of the number of lines (0: automatic) -- few lines force the overflow paths */
    uint32_t seed_table_count_bits; /* tests: count bits of a slot (0: all that are left) -- few send repeats to the side table */
    uint32_t reserved[2];
} lrm_index_options;
void lrm_index_options_init(lrm_index_options *o);

typedef struct lrm_map_options {
    uint32_t struct_size;      /* sizeof(lrm_map_options) of the caller's header */
    int32_t dense_results;     /* 0: cig_out[i].cigar = store_mem + i*store_stride (alnmain.c:322-325).
                                  1: DENSE -- cig_out[i].cigar = store_mem + off[i], the used op bytes of consecutive reads
                                  packed back to back (16-byte aligned) inside the region of store_mem their rows would
                                  occupy.  The convention of mutils.c:97-103 is kept (caller-owned buffer, callee-set
                                  pointer); with store_mem pinned the device image of the op bytes is DMA'd straight into
                                  it and the library spends no host CPU on the results.  Needs store_stride % 16 == 0. */
    int32_t gact_impl;         /* extension kernel: 0 automatic, 1 one read per wavefront, 3 two reads per wavefront,
                                  4 bit-sliced lane per read whenever it applies */
    int32_t seed_rounds;       /* 0 automatic (phase 0 first unless the previous batch decided < 2 % there), 1, 2 */
    int32_t vote_exact_only;   /* 1: every (read, phase) item goes through the exact vote kernel (the fast kernel in front of it
                                  is skipped); results are identical either way -- tests and A/B timing */
    uint32_t slice_reads;      /* host pipeline shape, 0 = automatic: reads per device pass, */
    uint32_t sub_batches;      /*   seed sub-batches per pass, */
    uint32_t group_subs;       /*   sub-batches per extension group */
    uint32_t bs_waves;         /* tests: cap on the resident wavefronts of the bit-sliced kernel (forces lane refills) */
    uint32_t cigar_text;       /* 1 (implies dense_results): cig_out[i].cigar points to the NUL-terminated run-length CIGAR TEXT
                                  parse_cigar would print from the op bytes (alnmain.c:497-498; '=' and 'X' columns as M, "*"
                                  for a read without an alignment) instead of the op bytes themselves -- the run-length pass runs
                                  on the device and ~0.45 instead of 1.1 bytes per read base cross the link.  n_cigar_op stays
                                  the number of alignment columns. */
    uint32_t copy_threads;     /* memcpy team of the PAGEABLE paths (upload staging, result placement): 0 automatic (the host's CPU
                                  share / replicas, at most 8 -- what 24 Gbp/s through pageable buffers needs), else 1..16; a caller
                                  whose own threads need the cores (lrm_accaln's parser and formatter) says 1 or 2 */
    uint32_t keep_reads;       /* 1: reads_buf is left exactly as the caller gave it -- the reverse-complemented copies of the
                                  reverse-strand reads (alnmain.c:437 does that in place, before the extension) stay on the device,
                                  0.5 bytes per read base less cross the link and nothing is placed on the host.  A caller that
                                  prints such a read (SAM SEQ) applies meta_out[i].strand itself: the read was reverse-complemented
                                  iff meta_r[i] != 0 && meta_out[i].strand == 1 (lrm_accaln's formatter does).  Host-buffer
                                  batch calls only. */
    uint32_t anchored;         /* 1: ANCHORED extension (docs/GACT_SPEC.md, "Anchored extension"): the longest exact match of the
                                  read within LRM_ANCHOR_DIAGS diagonals of the voted locus becomes the anchor, the read is extended
                                  to the right and to the left of it, and meta_out[i].loc / .off move to the alignment's first text
                                  base (SAM POS).  Needs store_stride >= 2*max_len + max_len/8 + 2.  0: every read is aligned
                                  against the window at the voted locus (alnmain.c:440-446) */
    uint32_t anchor_min_len;   /* shortest exact match that anchors a read: 0 = 20 (the default seed length), else 12..64 */
    uint32_t clip;             /* 1 (needs anchored): END CLIPPING (docs/GACT_SPEC.md, "End clipping"): each of the two jobs of an
                                  anchored read keeps the best-scoring prefix of its columns, counted outward from the anchor
                                  ('=' +1, 'X' / 'I' / 'D' -clip_penalty; the smallest such prefix), when that gains more than
                                  clip_end_bonus over keeping the whole job; the query bases of the columns that go become 'S'
                                  columns at the ends of the ops, score counts the aligned columns only and meta_out[i].loc / .off
                                  is the first ALIGNED text base.  Unanchored reads are left as the anchored mode leaves them.
                                  0: both jobs are global in the read */
    uint32_t clip_penalty;     /* P: 0 = 2, else 1..15 */
    uint32_t clip_end_bonus;   /* B: 0 = 6, else 1..255 */
    uint32_t split;            /* 1 (needs clip): SPLIT READS (docs/GACT_SPEC.md, "Split reads"): a soft-clipped end of at least
                                  split_min_len bases is mapped as a read of its own -- lrm_split_batch / lrm_split_batch_dev are the
                                  second pass, lrm_accaln_opt prints its results as supplementary records with SA:Z.  The batch
                                  calls themselves ignore the field: with it or without it they return the same bytes */
    uint32_t split_min_len;    /* M: 0 = 200, else 50..2^20 */
} lrm_map_options;
void lrm_map_options_init(lrm_map_options *o);

const char *lrm_last_error(void);
/* releases what an entry point documents as "free with lrm_free" (malloc'd text, the .cat of lrm_cat_from_seqs) */
void lrm_free(void *p);
int lrm_abi_version(void);
/* number of visible HIP devices (<=0: none). Does not fail loudly: probing only. */
int lrm_device_count(void);

/* ---------------------------------------------------------------------------
 * Index: host arrays in the reference's in-memory layout -> device image
 * ------------------------------------------------------------------------- */

/* Size in bytes of the device image ("blob") for an index of these dimensions. */
uint64_t lrm_index_blob_bytes(uint64_t length, int hlen, int mta_len);

/* Serialise the reference-layout arrays into the device image, in host memory
 * (blob must hold lrm_index_blob_bytes()).  Pure CPU; usable without a GPU.
 * sa: sa_len elements of ui40 in RAM (8-byte stride), as filled by ui40_fread. */
int lrm_index_pack_blob(const lrm_dna_fmi *fmi, const lrm_lc_hash *lch,
                        const lrm_sa_mem *sa, const char *content, uint64_t con_len,
                        const lrm_mta_entry *mta, int mta_len, void *blob, uint64_t blob_bytes);

/* One-call upload used behind alnmain.c:init(): the image is packed piece by piece into pinned chunks whose
 * DMA overlaps the packing of the next piece -- no host copy of the image. */
int lrm_index_upload(lrm_index **out, const lrm_dna_fmi *fmi, const lrm_lc_hash *lch,
                     const lrm_sa_mem *sa, const char *content, uint64_t con_len,
                     const lrm_mta_entry *mta, int mta_len, int device);

/* pack straight into device memory the caller owns (blob_bytes >= lrm_index_blob_bytes()): no host copy of the
 * image; the buffer can then be broadcast and adopted (lrm_index_adopt_device) on every rank. */
int lrm_index_pack_device(const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                          const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len,
                          void *d_blob, uint64_t blob_bytes, int device);

/* Multi-GPU group: the image is packed once, uploaded to devices[0] and replicated to the other devices over
 * xGMI (one RCCL broadcast; hipMemcpyPeer if librccl cannot be loaded).  devices == NULL means 0..ngpus-1.  The
 * returned handle is used with the same batch calls: lrm_seed_batch / lrm_extend_batch / lrm_map_batch split
 * the batch into ngpus contiguous slices balanced by bases and run one host thread per device, every device
 * writing its slice of the caller's arrays in place (results do not depend on ngpus).  A device may be listed
 * more than once (logical replicas on one GPU).  The *_dev entry points address one replica:
 * lrm_index_replica(). */
int lrm_index_upload_multi(lrm_index **out, const lrm_dna_fmi *fmi, const lrm_lc_hash *lch,
                           const lrm_sa_mem *sa, const char *content, uint64_t con_len,
                           const lrm_mta_entry *mta, int mta_len, const int *devices, int ngpus);
int lrm_index_replicas(const lrm_index *idx);
lrm_index *lrm_index_replica(lrm_index *idx, int r);     /* borrowed; replica 0 is the handle itself */

/* The same entry points with options (NULL = automatic).  lrm_index_upload_opt covers one device (ngpus == 1,
 * devices[0]; devices == NULL means device 0..ngpus-1) and the multi-GPU group. */
uint64_t lrm_index_blob_bytes_opt(uint64_t length, int hlen, int mta_len, const lrm_index_options *opt);
int lrm_index_pack_blob_opt(const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa, const char *content,
                            uint64_t con_len, const lrm_mta_entry *mta, int mta_len, void *blob, uint64_t blob_bytes,
                            const lrm_index_options *opt);
int lrm_index_pack_device_opt(const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa, const char *content,
                              uint64_t con_len, const lrm_mta_entry *mta, int mta_len, void *d_blob, uint64_t blob_bytes,
                              int device, const lrm_index_options *opt);
int lrm_index_upload_opt(lrm_index **out, const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                         const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len,
                         const int *devices, int ngpus, const lrm_index_options *opt);
int lrm_index_adopt_device_opt(lrm_index **out, void *d_blob, uint64_t blob_bytes, int device, const lrm_index_options *opt);
int lrm_index_upload_blob_opt(lrm_index **out, const void *blob, uint64_t blob_bytes, int device, const lrm_index_options *opt);

/* Default options of the batch calls on this handle (every replica of a group): lrm_seed_batch, lrm_extend_batch,
 * lrm_map_batch and the *_dev calls use them; lrm_map_batch_submit takes its own.  NULL restores the automatic choices. */
int lrm_index_set_map_options(lrm_index *idx, const lrm_map_options *opt);

/* Which derived seed tables a handle (replica 0 of a group) ended up with -- the automatic choices depend on the text
 * and on the HBM that was free at upload.  Results never depend on them. */
typedef struct lrm_index_tables {
    int32_t lc_long;             /* k-mer length of the long table (0: none) */
    int32_t lc_pair;             /* pair-line layout */
    int32_t lc_entry_bytes;      /* 8 or 5 */
    int32_t lc_core;             /* core table present */
    int32_t seed_table_len;      /* seed length of the seed table (0: none) */
    int32_t seed_table_share;    /* read positions per line: 4 or 2 */
    int32_t seed_table_bits;     /* log2 of its lines (64 bytes each) */
    int32_t seed_table_slot_bytes;
    int32_t seed_table_count_bits;
    int32_t reserved0;
    uint64_t seed_table_side_entries;   /* entries of crowded lines / counts beyond the slot's bits, in the side hash table */
    uint64_t derived_bytes;      /* HBM held by all derived tables (long table, core table, seed table, side tables) */
    uint64_t reserved[4];
} lrm_index_tables;
int lrm_index_get_tables(const lrm_index *idx, lrm_index_tables *out);

/* Adopt a blob that already sits in device memory (e.g. the destination of an
 * RCCL broadcast).  The blob is borrowed: it must outlive the handle. */
int lrm_index_adopt_device(lrm_index **out, void *d_blob, uint64_t blob_bytes, int device);

/* Upload a host blob (copy). */
int lrm_index_upload_blob(lrm_index **out, const void *blob, uint64_t blob_bytes, int device);

void lrm_index_free(lrm_index *idx);

/* ---------------------------------------------------------------------------
 * Batch entry points with HOST buffers (the drop-in boundary)
 * ------------------------------------------------------------------------- */

/* PART 1.  reads_buf: dense buffer, read i at reads_buf + i*stride, lens[i]
 * bases, upper-case ACGT (alnmain.c:87-103 layout, stride = max_read_len+1).
 * best_out[i] = the candidate entry the reference leaves in best[chunk_i]. */
int lrm_seed_batch(lrm_index *idx, const char *reads_buf, uint64_t stride,
                   const uint32_t *lens, uint64_t n, lrm_params p, lrm_entry *best_out);

/* PART 2.  Reads whose locus resolves to the reverse strand are reverse-
 * complemented IN PLACE in reads_buf (alnmain.c:433-438).  cig_out[i].cigar is
 * set to store_mem + i*store_stride (store_stride >= 2*lens[i]);
 * score_out[i] = cig_out[i].score (the value the reference writes to limit[]). */
int lrm_extend_batch(lrm_index *idx, char *reads_buf, uint64_t stride,
                     const uint32_t *lens, uint64_t n, const lrm_entry *best,
                     lrm_gact_params gp, lrm_cigar *cig_out, uint8_t *store_mem,
                     uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                     int *meta_r_out);

/* PART 1 + PART 2 for one batch in a single device pass: the reads cross the link once, best[] stays on the
 * device between the two parts.  Same outputs as lrm_seed_batch followed by lrm_extend_batch. */
int lrm_map_batch(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                  lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                  uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                  int *meta_r_out);

/* The same, asynchronous: lrm_map_batch_submit queues the batch and returns; lrm_map_batch_wait blocks until its
 * results are in the caller's arrays, returns the batch's status and frees the ticket.  Up to TWO batches per device
 * are in flight on the device at once -- the upload and the seeds of batch k+1 run under the extension tail and the
 * result download of batch k, which is the chain that bounds a single call (alnmain.c:302-330 with the copy clauses
 * planned at :420-424) -- further submissions queue.  Every argument array must stay valid, and untouched by the
 * caller, until the wait returns; batches complete in submission order.  lrm_map_batch == submit + wait.
 * opt == NULL: the handle's default options. */
typedef struct lrm_ticket lrm_ticket;
int lrm_map_batch_submit(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                         lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                         uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                         int *meta_r_out, const lrm_map_options *opt, lrm_ticket **ticket_out);
int lrm_map_batch_wait(lrm_ticket *ticket);

/* Pinned host memory for the batch buffers (reads_buf, store_mem): the DMA engines then read / write the
 * caller's memory directly; pageable buffers work too and are staged through pinned chunks.
 * lrm_host_register pins memory the caller already owns (what alnmain.c:297-320 mallocs). */
void *lrm_host_alloc(uint64_t bytes);
void lrm_host_free(void *p);
int lrm_host_register(void *p, uint64_t bytes);
int lrm_host_unregister(void *p);

/* alnmain.c:554-557 `pair_end`: declared, unimplemented ("todo") and returning -1 in the reference; kept so
 * that the call surface is complete. */
int lrm_pair_end(int argc, const char *argv[]);

/* PART 3 flag/mapq/valid assembly (alnmain.c:460-474); pure host arithmetic. */
void lrm_result_flags(const int *score, const int *meta_r, const lrm_seq_meta *meta,
                      uint64_t n, int *flag_out, int *mapq_out, int *valid_out);

/* MAPPING QUALITY (docs/GACT_SPEC.md, "Mapping quality").  The reference prints MAPQ 255 for every mapped read
 * (alnmain.c:460-474); this is a choice of THIS implementation, and it is asked for per CALL -- the entry points that take an
 * lrm_mapq array compute the records when they are given one, every other output is the same with it or without it --
 * not through lrm_map_options: that struct has no spare words left and keeps its 76 bytes.  Per read: n1 = the seed hits (phases up to the
 * deciding one) within `radius` diagonals of the chosen locus, n2 = the most hits any other place of width <= radius
 * collected, mapq = 60 * (n1 - min(n2, n1)) * min(n1, 10) / (10 * n1).  A read without a locus (best.val == 0): all zeros. */
#define LRM_MAPQ_SLOTS 4096            /* distinct (histogram, bucket) pairs of rival hits one read can hold */
#define LRM_MAPQ_OVERFLOW 1u           /* lrm_mapq.flags: more distinct rival places than slots -- a repeat read: n2 = n1, mapq 0 */
typedef struct lrm_mapq { uint32_t n1, n2, radius; uint8_t mapq, phase, flags, pad; } lrm_mapq;   /* 16 bytes; phase: the deciding one */
/* lrm_result_flags with the records: mapq_out[i] = mq[i].mapq for a mapped read, 0 for an unmapped one.  mq == NULL:
 * lrm_result_flags. */
void lrm_result_flags_mapq(const int *score, const int *meta_r, const lrm_seq_meta *meta, const lrm_mapq *mq, uint64_t n,
                           int *flag_out, int *mapq_out, int *valid_out);
/* lrm_map_batch_submit plus the records of the batch (mapq_out: n entries, filled when the wait returns; group handles write
 * every share in place).  mapq_out == NULL: lrm_map_batch_submit. */
int lrm_map_batch_submit_mapq(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                              lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                              uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                              int *meta_r_out, const lrm_map_options *opt, lrm_mapq *mapq_out, lrm_ticket **ticket_out);

/* ALIGNMENT SUMMARY (docs/GACT_SPEC.md, "Alignment summary and PAF").  With lrm_map_options.cigar_text only the run-length
 * text of an alignment crosses the link, and it prints '=' and 'X' both as M: what the alignment consists of is counted on
 * the device, over the op bytes while they are still in HBM, into one fixed-size record per read.  A read without an
 * alignment (n_cigar_op <= 0, meta_r == 0 or score == -1: the reads whose CIGAR prints as "*"): all zeros.  A row made only
 * of 'S': clip_left = n_cigar_op, clip_right = 0.  A byte outside "=XIDS" is counted nowhere (it still ends a run, and it
 * is a column that is not 'S').  An 'I' run right behind a 'D' run, or the reverse, is a run of its own; the classic mode's
 * 'I' tail ("target exhausted") is insertion columns and one run.  From a record:
 *   NM            = n_x + n_ins + n_del        (the score of the spec: the edit distance of the ops)
 *   target span   = n_eq + n_x + n_del
 *   block length  = n_eq + n_x + n_ins + n_del
 *   aligned query = [clip_left, len - clip_right) in the orientation of the ops
 * Like the mapping quality it is asked for per CALL, not through lrm_map_options. */
typedef struct lrm_aln_summary {          /* 32 bytes, all columns counted over the read's n_cigar_op op bytes */
    uint32_t n_eq, n_x, n_ins, n_del;     /* '=' , 'X', 'I', 'D' columns */
    uint32_t ins_runs, del_runs;          /* maximal runs of 'I' / of 'D' columns (gap opens) */
    uint32_t clip_left, clip_right;       /* 'S' columns before the first / after the last column that is not 'S' */
} lrm_aln_summary;
/* The rule on the host, for callers that hold op bytes: pure arithmetic, usable without a GPU.  n_ops <= 0: zeros. */
void lrm_aln_summary_host(const uint8_t *ops, int n_ops, lrm_aln_summary *out);

/* Per-call extras of the host-buffer path: output arrays of n entries each that a batch fills on top of the arguments of
 * lrm_map_batch_submit (NULL: that output is not computed, nothing runs or is allocated for it).  struct_size:
 * sizeof(lrm_batch_extras) of the caller's header (0: all of it). */
typedef struct lrm_batch_extras {
    uint32_t struct_size, reserved;
    lrm_mapq *mapq_out;                   /* the mapping-quality records (lrm_map_batch_submit_mapq) */
    lrm_aln_summary *summary_out;         /* the alignment summary records: the stage runs per extension group, behind the group's
                                             extension (clip and stitch included), and the records come down with the small arrays */
} lrm_batch_extras;
/* lrm_map_batch_submit plus the extras (ex == NULL or both arrays NULL: lrm_map_batch_submit).  Filled when the wait
 * returns; group handles write every share in place; every other output is the same bytes with the extras or without. */
int lrm_map_batch_submit_ex(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                            lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                            uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                            int *meta_r_out, const lrm_map_options *opt, const lrm_batch_extras *ex, lrm_ticket **ticket_out);

/* The DIFFERENCE EVENTS of a host-buffer batch (above; docs/GACT_SPEC.md, "Difference events and MD:Z").  Read i's events are
 * events_out[off_out[i] .. off_out[i] + cnt_out[i]).  The stage runs per extension group (every share of a group handle
 * too), and a group takes its place in events_out when it is collected: the offsets of different groups come in any order.
 * A group whose events do not fit below cap gives its reads off_out = UINT64_MAX with their true counts; *needed_out is the
 * batch's total in any case and the wait still returns 0 -- the caller compares needed with cap.  The request runs the
 * summary stage whether lrm_batch_extras.summary_out is given or not.  struct_size: sizeof(lrm_batch_diff) of the caller's header. */
typedef struct lrm_batch_diff {
    uint32_t struct_size, reserved;
    uint64_t *off_out;                    /* n entries */
    uint32_t *cnt_out;                    /* n entries: n_x + n_del of every read */
    uint32_t *events_out;                 /* cap events (may be NULL when cap == 0: counting only) */
    uint64_t cap;
    uint64_t *needed_out;                 /* one entry, written when the wait returns */
} lrm_batch_diff;
/* lrm_map_batch_submit_ex plus the events (diff == NULL: exactly lrm_map_batch_submit_ex).  Every other output is the same
 * bytes with them or without. */
int lrm_map_batch_submit_ex2(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                             lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                             uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                             int *meta_r_out, const lrm_map_options *opt, const lrm_batch_extras *ex,
                             const lrm_batch_diff *diff, lrm_ticket **ticket_out);

/* ---------------------------------------------------------------------------
 * Batch entry points with DEVICE buffers (inputs/outputs resident in HBM;
 * asynchronous on `stream`, a hipStream_t passed as void*, may be NULL).
 * ------------------------------------------------------------------------- */

typedef struct lrm_workspace lrm_workspace;   /* opaque: device scratch for a batch shape */

/* Scratch for batches of up to n_max reads of up to max_len bases.
 * Preconditions of the *_dev calls (not checked on the device): d_lens[i] <= max_len <= stride, and
 * store_stride >= 2*max_len.  A kernel-side error of a batch (vote table overflow) is sticky: the NEXT *_dev
 * call on the workspace, or lrm_workspace_stats, returns -2 and clears it.
 *
 * Read extents.  stride == max_len is supported: rows may abut, and the last row may end on the buffer's last byte.  The
 * result of every call is a function of d_reads[i*stride .. i*stride + d_lens[i]) and d_lens alone: whatever lies between,
 * in front of and behind the reads -- zeros, bases, the next read -- is never compared, packed or copied.  A kernel may
 * LOAD the aligned 16-byte lines that hold a read's first and last base, so up to 15 bytes in front of the first read and
 * behind the last one: d_reads need not be aligned, but those two lines must lie in memory the device can read (any
 * allocation does: its granularity is coarser).  Rows >= n of any array are neither read nor written.
 *
 * Written extents.  The extension calls turn the d_lens[i] bases of a reverse-strand read round in place and write no
 * other byte of d_reads.  Of every output array they write the rows < n only.  Of op row i (d_store + i*store_stride) no
 * byte at or behind n_ops[i] rounded up to 4 (lrm_extend_batch_dev) or to 16 (the anchored and the clipped call, which move
 * 16-byte groups) is written; a read without a locus (meta_r == 0) gets no op byte at all.  One exception: a read of
 * lrm_extend_batch_dev with a locus whose alignment is abandoned (score == -1, n_ops == 0) may leave the columns walked so
 * far, at most 2*d_lens[i] bytes.  (Today's kernels end on byte n_ops[i]; the rounding is granted on purpose, so that a
 * kernel may come to store whole groups without breaking a caller that packs something of its own behind a row.)
 * The per-segment and per-candidate stores of the split and secondary stages follow the clipped call's rule; their rows
 * arrays are written to the next multiple of 16 behind a segment (split) or to row_stride (secondary), zeros behind the
 * bases. */
int lrm_workspace_create(lrm_workspace **out, lrm_index *idx, uint64_t n_max,
                         uint32_t max_len, uint32_t seed_len, uint32_t thres);
void lrm_workspace_free(lrm_workspace *ws);
uint64_t lrm_workspace_bytes(const lrm_workspace *ws);

int lrm_seed_batch_dev(lrm_index *idx, lrm_workspace *ws, const char *d_reads,
                       uint64_t stride, const uint32_t *d_lens, uint64_t n,
                       uint32_t max_len, lrm_params p, lrm_entry *d_best, void *stream);

/* lrm_seed_batch_dev plus the mapping-quality records (d_mapq: n entries in device memory; NULL: lrm_seed_batch_dev).  The
 * stage runs right behind the seed stage on the same stream, over the survivor lists that stage left in the workspace.  The
 * first such call on a workspace allocates one byte per read (the deciding phase); lrm_workspace_bytes grows by it. */
int lrm_seed_batch_mapq_dev(lrm_index *idx, lrm_workspace *ws, const char *d_reads, uint64_t stride,
                            const uint32_t *d_lens, uint64_t n, uint32_t max_len, lrm_params p,
                            lrm_entry *d_best, lrm_mapq *d_mapq, void *stream);

int lrm_extend_batch_dev(lrm_index *idx, lrm_workspace *ws, char *d_reads, uint64_t stride,
                         const uint32_t *d_lens, uint64_t n, uint32_t max_len,
                         const lrm_entry *d_best, lrm_gact_params gp, uint8_t *d_store,
                         uint64_t store_stride, int32_t *d_n_ops, int32_t *d_score,
                         lrm_seq_meta *d_meta, int32_t *d_meta_r, void *stream);

/* ANCHORED extension (lrm_map_options.anchored; docs/GACT_SPEC.md): the arguments of lrm_extend_batch_dev plus the anchor
 * records (d_anchor: n entries in device memory, may be NULL) and the shortest anchor (min_len: 0 = 20, else 12..64).
 * The precondition on the store becomes store_stride >= 2*max_len + max_len/8 + 2 (checked).  The first call on a
 * workspace allocates the scratch of the mode (job table, job rows, their op bytes); lrm_workspace_bytes grows by it. */
#define LRM_ANCHOR_DIAGS 64            /* diagonals L + delta, delta in [-32, 32), searched around the voted locus L */
#define LRM_ANCHOR_ANCHORED 1u         /* lrm_anchor.flags: an anchor was found, the read was extended both ways from it */
#define LRM_ANCHOR_FALLBACK 2u         /*   no exact match of min_len bases: extended from the voted locus as without the mode */
#define LRM_ANCHOR_NO_LEFT 4u          /*   the anchor starts at the read's first base: no left job */
#define LRM_ANCHOR_LEFT_CLIPPED 8u     /*   the left job's target window ends at the start of the sequence */
#define LRM_ANCHOR_RIGHT_CLIPPED 16u   /*   the right job's target window ends at the end of the sequence */
#define LRM_ANCHOR_SOFT_LEFT 32u       /*   end clipping: the ops begin with 'S' columns */
#define LRM_ANCHOR_SOFT_RIGHT 64u      /*   end clipping: the ops end with 'S' columns */
typedef struct lrm_anchor {
    uint64_t text_pos;                 /* text position of read[read_pos] (forward half of the sequence) */
    uint32_t read_pos, len;            /* the exact match read[read_pos .. read_pos + len) */
    int32_t delta;                     /* its diagonal relative to the voted locus */
    uint32_t left_ops;                 /* alignment columns of the left job (the first left_ops op bytes of the read; with end
                                          clipping: its 'S' columns and the columns it kept) */
    uint32_t flags;                    /* LRM_ANCHOR_*; 0 for a read without a locus (meta_r == 0) */
} lrm_anchor;
int lrm_extend_batch_anchored_dev(lrm_index *idx, lrm_workspace *ws, char *d_reads, uint64_t stride,
                                  const uint32_t *d_lens, uint64_t n, uint32_t max_len,
                                  const lrm_entry *d_best, lrm_gact_params gp, uint8_t *d_store,
                                  uint64_t store_stride, int32_t *d_n_ops, int32_t *d_score,
                                  lrm_seq_meta *d_meta, int32_t *d_meta_r, lrm_anchor *d_anchor, uint32_t min_len,
                                  void *stream);

/* The anchored extension with END CLIPPING (lrm_map_options.clip; docs/GACT_SPEC.md, "End clipping"): the arguments of
 * lrm_extend_batch_anchored_dev (which never clips, whatever the handle's options say), the penalty P (clip_penalty: 0 = 2,
 * else 1..15), the end bonus B (clip_end_bonus: 0 = 6, else 1..255) and the soft-clipped bases per read (d_clip: n entries
 * in device memory, may be NULL; zeros for a read the step leaves alone: unanchored or without a locus).  The first
 * clipping call on a workspace allocates 16 bytes per job on top of the mode's scratch. */
typedef struct lrm_clip { uint32_t left, right; } lrm_clip;     /* 'S' columns at the start / at the end of the ops */
int lrm_extend_batch_clipped_dev(lrm_index *idx, lrm_workspace *ws, char *d_reads, uint64_t stride,
                                 const uint32_t *d_lens, uint64_t n, uint32_t max_len,
                                 const lrm_entry *d_best, lrm_gact_params gp, uint8_t *d_store,
                                 uint64_t store_stride, int32_t *d_n_ops, int32_t *d_score,
                                 lrm_seq_meta *d_meta, int32_t *d_meta_r, lrm_anchor *d_anchor, uint32_t min_len,
                                 uint32_t clip_penalty, uint32_t clip_end_bonus, lrm_clip *d_clip, void *stream);

/* The ALIGNMENT SUMMARY records (lrm_aln_summary above) of a batch whose op bytes sit in device memory: call it behind any
 * of the three extension calls on the same stream, with that call's d_store, store_stride, d_n_ops, d_score, d_meta_r.
 * d_out: n records in device memory, 16-byte aligned.  One streaming kernel, one byte read per column; no workspace. */
int lrm_aln_summary_dev(lrm_index *idx, const uint8_t *d_store, uint64_t store_stride,
                        const int32_t *d_n_ops, const int32_t *d_score, const int32_t *d_meta_r,
                        uint64_t n, lrm_aln_summary *d_out, void *stream);

/* DIFFERENCE EVENTS (docs/GACT_SPEC.md, "Difference events and MD:Z"): what MD:Z needs and the run-length text has lost --
 * one 32-bit word per 'X' or 'D' column of an alignment, in column order:
 *   bits 0-7    the reference base of the column, content[meta.loc + t] as stored (0 for a position at or behind the end of the text)
 *   bits 8-9    the kind: LRM_DIFF_X, LRM_DIFF_D_OPEN (a 'D' whose previous column is not 'D'), LRM_DIFF_D_MORE
 *   bits 10-31  the '=' columns before it
 * A read has n_x + n_del events of its summary record; a read without an alignment has none.  The events of a batch are
 * packed per read at exclusive prefix sums of those counts.  store_stride <= 2^22 (checked): the '=' count fits its bits. */
#define LRM_DIFF_X 0u
#define LRM_DIFF_D_OPEN 1u
#define LRM_DIFF_D_MORE 2u
#define LRM_DIFF_BASE(w) ((uint32_t) (w) & 0xFFu)
#define LRM_DIFF_KIND(w) (((uint32_t) (w) >> 8) & 3u)
#define LRM_DIFF_EQ_BEFORE(w) ((uint32_t) (w) >> 10)
/* d_off[0 .. n]: exclusive prefix sums of n_x + n_del over the n summary records in device memory (d_off[n]: the batch's
 * total).  One small scan kernel on `stream`. */
int lrm_aln_diff_offsets_dev(const lrm_aln_summary *d_summary, uint64_t n, uint64_t *d_off, void *stream);
/* The events of a batch whose op bytes sit in device memory: call it behind any of the three extension calls and the summary
 * (and lrm_aln_diff_offsets_dev) on the same stream, with the extension's d_store, store_stride, d_n_ops, d_score, d_meta_r,
 * d_meta.  Read i's events go to d_events[d_off[i] .. d_off[i + 1]); a read with d_off[i + 1] > cap writes nothing (cap: the
 * room of d_events, in events).  One streaming kernel: a byte of ops and a byte of text read per column; no workspace. */
int lrm_aln_diff_dev(lrm_index *idx, const uint8_t *d_store, uint64_t store_stride, const int32_t *d_n_ops,
                     const int32_t *d_score, const int32_t *d_meta_r, const lrm_seq_meta *d_meta, uint64_t n,
                     const uint64_t *d_off, uint64_t cap, uint32_t *d_events, void *stream);
/* The rule on the host, for callers that hold op bytes and the text they were aligned against: target[0] is the first
 * aligned target base (content + meta.loc), target_len what is left of the text from there.  events_out: room for every
 * 'X' and 'D' column of ops (NULL: count only).  Returns the number of events; n_ops <= 0: 0.  Usable without a GPU. */
int64_t lrm_aln_diff_host(const uint8_t *ops, int n_ops, const uint8_t *target, uint64_t target_len, uint32_t *events_out);
/* MD:Z text of one read from its events and the n_eq of its summary record, NUL-terminated ("10A0C5", "5^AC0T").  Returns
 * the text length, < 0 when buf (buflen bytes, the NUL included) is too small. */
int lrm_md_format(const uint32_t *events, uint64_t count, uint32_t n_eq, char *buf, int buflen);

/* PILEUP (docs/GACT_SPEC.md, "Pileup"): per text position of a window [lo, hi) of content[] -- the coordinate of
 * lrm_seq_meta.loc -- how many alignments cover it, which read bases their 'X' columns show there, how many 'D' columns
 * fall on it and how many 'I' runs open behind it.  A reduction over all reads of all batches that stays in device memory:
 * an accumulator is created once, every batch is added behind its extension, and the records come down when the caller
 * asks, 32 bytes per position.  Asked for per CALL like the summary and the events: nothing runs or is allocated unless a
 * caller creates an accumulator, and every other output is the same bytes with it or without it.
 *   depth   the alignments that cover the position, 'D' columns included
 *   n_eq    depth - (every 'X' count, the class `other` included) - n_del
 *   x_a, x_c, x_g, x_t   'X' columns whose read byte is A/a, C/c, G/g, T/t; any other read byte counts in `other`, which is
 *           depth - n_eq - x_a - x_c - x_g - x_t - n_del
 *   n_del   'D' columns
 *   n_ins   'I' runs that open right behind this position
 * All counters are 32-bit and wrap. */
typedef struct lrm_pileup_col { uint32_t depth, n_eq, x_a, x_c, x_g, x_t, n_del, n_ins; } lrm_pileup_col;   /* 32 bytes */
#define LRM_PILEUP_TILE 2048           /* positions per workgroup of the read-back: the depth is a prefix sum, scanned by tiles */
typedef struct lrm_pileup lrm_pileup;  /* opaque: the accumulator of one window on one device */
/* lo < hi <= con_len of the handle's text (checked; a group handle is refused: its replicas would each hold a part).  The
 * accumulator is 32 * (hi - lo) + 4 bytes of counters, zeroed, with 64 guard bytes behind them, and 8 bytes per tile of
 * read-back scratch; lrm_pileup_bytes: all of it. */
int lrm_pileup_create(lrm_pileup **out, lrm_index *idx, uint64_t lo, uint64_t hi);
void lrm_pileup_free(lrm_pileup *pl);
uint64_t lrm_pileup_bytes(const lrm_pileup *pl);
int lrm_pileup_reset(lrm_pileup *pl, void *stream);      /* all counters back to zero, asynchronous on `stream` */
/* Adds a batch whose op bytes sit in device memory: call it behind any of the three extension calls on the same stream, with
 * that call's d_reads, stride, d_lens (the reads as the extension left them: reverse-strand reads reverse-complemented in
 * place), d_store, store_stride, d_n_ops, d_score, d_meta_r, d_meta.  d_mapq (n lrm_mapq records in device memory, may be
 * NULL): a read with mapq < min_mapq adds nothing.  store_stride <= 2^31 (checked: the column counts of a row are 32-bit).
 * One streaming kernel: a byte of ops read per column, 16 read bytes per lane that holds an 'X'; one atomic add per 'X',
 * 'D' and opening 'I' column inside the window, and two per read for the depth. */
int lrm_pileup_add_dev(lrm_pileup *pl, const char *d_reads, uint64_t stride, const uint32_t *d_lens, const uint8_t *d_store,
                       uint64_t store_stride, const int32_t *d_n_ops, const int32_t *d_score, const int32_t *d_meta_r,
                       const lrm_seq_meta *d_meta, uint64_t n, const lrm_mapq *d_mapq, uint32_t min_mapq, void *stream);
/* The records of the positions lo + first .. lo + first + count - 1 into d_out (count records in device memory, 16-byte
 * aligned); first + count <= hi - lo (checked).  Three small kernels on `stream`; the counters are not modified, so more
 * batches can be added afterwards and read back again. */
int lrm_pileup_read_dev(lrm_pileup *pl, uint64_t first, uint64_t count, lrm_pileup_col *d_out, void *stream);
/* The rule on the host, usable without a GPU.  planes: 8 * (hi - lo) + 1 words, zeroed by the caller before the first read
 * (the device accumulator's own layout: the depth as a difference plane of hi - lo + 1 words, then seven event planes).
 * One ALIGNED read: its op bytes, its bases in the orientation of the ops, meta.loc.  n_ops <= 0: nothing. */
void lrm_pileup_add_host(const uint8_t *ops, int n_ops, const uint8_t *read, uint32_t read_len, uint64_t loc, uint64_t lo,
                         uint64_t hi, uint32_t *planes);
/* ... and the records of lo + first .. lo + first + count - 1 from such planes.  0 ok, -1 bad range. */
int lrm_pileup_cols_host(const uint32_t *planes, uint64_t lo, uint64_t hi, uint64_t first, uint64_t count, lrm_pileup_col *out);
/* Tab-separated text of count positions of sequence seq from its base seq_pos (0-based) on, one line each, no header:
 * name, 1-based position, reference base, depth, n_eq, x_a, x_c, x_g, x_t, other, n_del, n_ins.  cols[k]: the record of
 * text position mta[seq].offset + seq_pos + k; content: the text (host memory).  Returns the text length (NUL-terminated,
 * the NUL not counted), < 0 when buf (buflen bytes) is too small or an argument is bad. */
int64_t lrm_pileup_format(const lrm_mta_entry *mta, int mta_len, int seq, uint64_t seq_pos, uint64_t count, const char *content,
                          const lrm_pileup_col *cols, char *buf, int64_t buflen);
/* PILEUP CALLS (docs/GACT_SPEC.md, "Pileup calls"): the read side of the accumulator for a caller who wants the few
 * positions where the reads disagree with the text, and one consensus letter per position, instead of 32 bytes per
 * position.  With c the record of a position, b = content[pos] its text byte, rc the class of b (A, C, G, T or other, case
 * folded) and allele[k] = x_k + (k == rc ? n_eq : 0) for k in A, C, G, T:
 *   passes(n)  depth >= min_depth && n >= min_count && 100 * n >= min_pct * depth        (64-bit products)
 *   kinds      LRM_CALL_SNV: some k != rc has passes(allele[k]); LRM_CALL_DEL: passes(n_del); LRM_CALL_INS: passes(n_ins).
 *              A position is a SITE iff kinds != 0.
 *   alt, n_alt the k != rc with the largest allele[k] (a tie: the earlier of A, C, G, T) and its count; '.' when that is 0
 *   cons       'N' when depth < min_depth or allele[A..T] and n_del are all 0; otherwise the largest of the five, ties to
 *              the reference class first, then A, C, G, T, then the deletion ('-').  Insertions do not enter it: one
 *              byte per position.  Their bases are the polished sequence's (lrm_pileup_create_ins, below).
 * Options: a zero field means its default (8, 4, 25); min_pct > 100 or reserved != 0 is refused. */
#define LRM_CALL_SNV 1u
#define LRM_CALL_DEL 2u
#define LRM_CALL_INS 4u
typedef struct lrm_pileup_call_options { uint32_t min_depth, min_count, min_pct, reserved; } lrm_pileup_call_options;
typedef struct lrm_pileup_site {       /* 32 bytes */
    uint64_t pos;                      /* the text position */
    uint32_t depth, n_ref, n_alt, n_del, n_ins;        /* n_ref = n_eq */
    uint8_t ref, alt, cons, kinds;     /* ref: the text byte as stored */
} lrm_pileup_site;
/* The sites of window positions [first, first + count), first + count <= hi - lo (checked; count < 2^32), in ascending
 * position into d_sites (cap records in device memory, 16-byte aligned; may be NULL with cap == 0).  *d_n_sites (device
 * memory, 8-byte aligned) gets the number of sites in the range whether or not they fit; sites from index cap on are not
 * written.  d_cons, when not NULL, gets count bytes: d_cons[k] = cons of position first + k.  opt NULL: the defaults.
 * Everything is asynchronous on `stream`: no host wait.  The counters are not modified: add more batches, call again.  The
 * first call allocates 8 bytes per tile of scratch, which lrm_pileup_bytes counts from then on. */
int lrm_pileup_sites_dev(lrm_pileup *pl, const lrm_pileup_call_options *opt, uint64_t first, uint64_t count,
                         lrm_pileup_site *d_sites, uint64_t cap, uint64_t *d_n_sites, uint8_t *d_cons, void *stream);
/* The same rule on records the caller holds, usable without a GPU: cols[k] and content[k] are the record and the text byte
 * of text position pos0 + k.  out: cap records (may be NULL with cap == 0); cons: count bytes or NULL.  Returns the number
 * of sites whether or not they fit, < 0 for refused options or a null argument. */
int64_t lrm_pileup_sites_host(const lrm_pileup_col *cols, const char *content, uint64_t pos0, uint64_t count,
                              const lrm_pileup_call_options *opt, lrm_pileup_site *out, uint64_t cap, uint8_t *cons);
/* Tab-separated text of count sites, one line each, no header: sequence name, 1-based position in it, ref, alt, the kinds
 * as a subset of the letters SDI, depth, n_ref, n_alt, n_del, n_ins, cons.  The sequence is the entry of mta that holds
 * pos.  Returns the text length (NUL-terminated, the NUL not counted), < 0 when buf (buflen bytes) is too small or an
 * argument is bad (a pos in no sequence among them). */
int64_t lrm_pileup_sites_format(const lrm_mta_entry *mta, int mta_len, const lrm_pileup_site *sites, uint64_t count,
                                char *buf, int64_t buflen);
/* Test-only: the first `words` words of the accumulator's allocation (the 8 * (hi - lo) + 1 counter words, then 16 guard
 * words of 0xC5C5C5C5) into host memory; waits for `stream`. */
int lrm_debug_pileup_raw(lrm_pileup *pl, uint32_t *out, uint64_t words, void *stream);
/* PILEUP INSERTIONS AND THE POLISHED CONSENSUS (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus"): an
 * accumulator may carry K insertion columns, 1 <= K <= LRM_PILEUP_INS_COLS_MAX: 4 * K more planes of hi - lo words in an
 * allocation of their own, plane 4 * j + k for insertion column j < K and base class k in A, C, G, T.  An 'I' column that is
 * the j-th of its run (j counted from 0), j < K, behind at least one target column, whose read byte is a base (case folded),
 * adds 1 to plane (j, class) at the position of the target column before the run, when that lies in the window.  A read
 * byte that is no base, or at or behind the read's length, is counted nowhere.  With s[j][k] a position's insertion words,
 * sup[j] their 32-bit sum over k (it wraps like the counters), depth and n_ins the position's record:
 *   len      the number of leading j < K with 2 * sup[j] > n_ins (64-bit products): the majority of the reads that insert here
 *   bases[j] for j < len the class with the largest s[j][k], a tie to the earlier of A, C, G, T; 0 from len on
 *   flags    LRM_INS_ENTERS: depth >= min_depth && 2 * n_ins > depth; LRM_INS_FULL: len == K (the run may be longer)
 *   n_col0   sup[0]
 * The polished sequence of a range, position by position in ascending order: the cons letter of the call rule, nothing for
 * '-' ('N' stays), then, when LRM_INS_ENTERS, the len bases of the allele. */
#define LRM_PILEUP_INS_COLS_MAX 8
#define LRM_INS_ENTERS 1u
#define LRM_INS_FULL 2u
typedef struct lrm_pileup_ins_allele { uint32_t n_col0; uint8_t len, flags, pad[2]; uint8_t bases[8]; } lrm_pileup_ins_allele;   /* 16 bytes */
/* lrm_pileup_create with ins_cols insertion columns.  ins_cols == 0 is lrm_pileup_create exactly; ins_cols > 8 is refused.
 * The insertion planes are 16 * ins_cols * (hi - lo) bytes, zeroed, with 64 guard bytes behind them; lrm_pileup_bytes
 * counts them, lrm_pileup_reset clears them.  On such an accumulator the one launch of lrm_pileup_add_dev also counts the
 * insertion columns: about one more atomic add per 'I' column of a run's first ins_cols. */
int lrm_pileup_create_ins(lrm_pileup **out, lrm_index *idx, uint64_t lo, uint64_t hi, uint32_t ins_cols);
uint32_t lrm_pileup_ins_cols(const lrm_pileup *pl);
/* The insertion words of window positions [first, first + count), position-major: d_out[(g - first) * 4K + 4j + k] (device
 * memory, 16-byte aligned).  Refused on an accumulator without insertion planes.  Asynchronous; the counters are not modified. */
int lrm_pileup_ins_read_dev(lrm_pileup *pl, uint64_t first, uint64_t count, uint32_t *d_out, void *stream);
/* The polished sequence of window positions [first, first + count) into d_seq[0 .. cap) (device memory; may be NULL with
 * cap == 0).  *d_len (device memory, 8-byte aligned) gets its length whether or not it fits; bytes from index cap on are not
 * written and nothing outside d_seq[0 .. cap) is touched.  count * (K + 1) < 2^32 (checked).  On an accumulator without
 * insertion planes: the cons letters without '-'.  opt as for lrm_pileup_sites_dev; asynchronous on `stream`, the counters
 * are not modified; the scratch is that of lrm_pileup_sites_dev (allocated by the first call of either). */
int lrm_pileup_polish_dev(lrm_pileup *pl, const lrm_pileup_call_options *opt, uint64_t first, uint64_t count, uint8_t *d_seq,
                          uint64_t cap, uint64_t *d_len, void *stream);
/* The inserted allele of every record of a site table of this accumulator (n records in device memory, as
 * lrm_pileup_sites_dev wrote them: depth and n_ins are the record's) into d_out (n records, 16-byte aligned), zero-padded.
 * A pos outside the window gives an all-zero record.  Refused on an accumulator without insertion planes. */
int lrm_pileup_site_alleles_dev(lrm_pileup *pl, const lrm_pileup_call_options *opt, const lrm_pileup_site *d_sites, uint64_t n,
                                lrm_pileup_ins_allele *d_out, void *stream);
/* The rules on the host, usable without a GPU.  ins_planes: 4 * ins_cols * (hi - lo) words in the device's layout, zeroed by
 * the caller; one ALIGNED read as for lrm_pileup_add_host (which counts everything else).  Bad arguments: nothing. */
void lrm_pileup_ins_add_host(const uint8_t *ops, int n_ops, const uint8_t *read, uint32_t read_len, uint64_t loc, uint64_t lo,
                             uint64_t hi, uint32_t ins_cols, uint32_t *ins_planes);
/* cols[k], content[k], ins_words + 4 * ins_cols * k: the record, the text byte and the position-major insertion words of
 * position k (ins_cols == 0: ins_words is not read).  out: cap bytes (may be NULL with cap == 0).  Returns the polished
 * length whether or not it fits, < 0 for refused options or arguments. */
int64_t lrm_pileup_polish_host(const lrm_pileup_col *cols, const uint32_t *ins_words, uint32_t ins_cols, const char *content,
                               uint64_t count, const lrm_pileup_call_options *opt, uint8_t *out, uint64_t cap);
/* The allele of one position from its 4 * ins_cols insertion words.  0 ok, < 0 refused. */
int lrm_pileup_ins_allele_host(uint32_t depth, uint32_t n_ins, const uint32_t *ins_words, uint32_t ins_cols,
                               const lrm_pileup_call_options *opt, lrm_pileup_ins_allele *out);
/* Test-only: the first `words` words of the insertion planes' allocation (4 * ins_cols * (hi - lo) words, then 16 guard
 * words of 0xC5C5C5C5) into host memory; waits for `stream`. */
int lrm_debug_pileup_ins_raw(lrm_pileup *pl, uint32_t *out, uint64_t words, void *stream);
/* PILEUP ON THE HOST-BUFFER PATH AND ACROSS REPLICAS (docs/GACT_SPEC.md, section of that name).  A host-buffer batch may name
 * one accumulator per replica of its handle; every extension group of the batch is then added to its replica's accumulator
 * behind the group's extension, on the group's stream, from the device mirrors of the batch (the one launch of
 * lrm_pileup_add_dev; nothing is downloaded, no device memory is allocated for it).  The accumulators of the replicas are
 * combined afterwards with lrm_pileup_merge_dev: all counters are integer sums.
 * lrm_pileup_create_replica: lrm_pileup_create_ins on replica r of a handle (0 <= r < lrm_index_replicas(idx), checked) -- the
 * way to an accumulator on replica 0 of a group handle, which is the group handle itself and which lrm_pileup_create refuses. */
int lrm_pileup_create_replica(lrm_pileup **out, lrm_index *idx, int r, uint64_t lo, uint64_t hi, uint32_t ins_cols);
/* The request of a batch.  pileups[r]: the accumulator of replica r, created on that replica (lrm_pileup_create_replica, or
 * lrm_pileup_create[_ins] on a handle of one device); n_pileups == lrm_index_replicas(idx).  min_mapq: a read whose lrm_mapq
 * record says less adds nothing; it needs lrm_batch_extras.mapq_out (the filter reads the records of that stage on the device).
 * Refused with nothing queued: another n_pileups, an entry that is NULL or of another replica, reserved != 0, min_mapq != 0
 * without mapq_out, store_stride above 2^31.  Contract:
 *   - when lrm_map_batch_wait returns 0, all counts of the batch are in the accumulators: any later read-side call, on any
 *     stream, sees them;
 *   - several batches in flight may add to one accumulator (the adds are atomic, the sums integer); the slices of a replica's
 *     share of one batch do;
 *   - the accumulators must outlive the ticket; lrm_pileup_reset with a batch in flight is the caller's error;
 *   - a batch that fails may have added part of its reads;
 *   - lrm_split_batch and lrm_secondary_batch add nothing. */
typedef struct lrm_batch_pileup {
    uint32_t struct_size, min_mapq;
    lrm_pileup **pileups;
    uint32_t n_pileups, reserved;
} lrm_batch_pileup;
/* lrm_map_batch_submit_ex2 plus the request (pile == NULL: exactly lrm_map_batch_submit_ex2).  Every other output is the same
 * bytes with it or without. */
int lrm_map_batch_submit_ex3(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                             lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                             uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                             int *meta_r_out, const lrm_map_options *opt, const lrm_batch_extras *ex,
                             const lrm_batch_diff *diff, const lrm_batch_pileup *pile, lrm_ticket **ticket_out);
/* dst += src.  Both must have the same lo, hi and ins_cols and be different objects (refused otherwise).  Every one of the
 * 8 * (hi - lo) + 1 counter words of dst -- the difference plane of the depth included -- gets src's word added, in 32 bits
 * and wrapping like the counters; with insertion planes every one of their 16 * ins_cols * (hi - lo) / 4 words likewise.  The
 * guard words are not touched and src is not modified (a caller who wants it empty resets it).  Asynchronous on `stream`, a
 * stream of dst's device; the batches that add to src must have been waited for, and the caller orders other writers of dst
 * (the kernel uses no atomics).  src on dst's device: one streaming kernel per allocation reads src's planes directly.  src
 * on another device: a staging buffer on dst's device (allocated by the first such merge, counted by lrm_pileup_bytes(dst)
 * from then on, freed with dst) receives src's words chunk by chunk through hipMemcpyPeerAsync on `stream`, and the kernel
 * adds each chunk; the next copy follows the add by stream order. */
int lrm_pileup_merge_dev(lrm_pileup *dst, const lrm_pileup *src, void *stream);
/* Test-only: the staged route with chunks of chunk_words words (a multiple of 4, at least 4: checked) on any pair of devices. */
int lrm_debug_pileup_merge_staged(lrm_pileup *dst, const lrm_pileup *src, uint64_t chunk_words, void *stream);
/* lrm_pileup_sites_format with one more column at the end of every line: the inserted bases of the site, alleles[k].bases[0 ..
 * alleles[k].len), '.' when len == 0 (alleles: what lrm_pileup_site_alleles_dev wrote for the same table).  alleles == NULL:
 * exactly lrm_pileup_sites_format. */
int64_t lrm_pileup_sites_format_ins(const lrm_mta_entry *mta, int mta_len, const lrm_pileup_site *sites,
                                    const lrm_pileup_ins_allele *alleles, uint64_t count, char *buf, int64_t buflen);
/* PILEUP VARIANTS AND VCF (docs/GACT_SPEC.md, section of that name): the sites of a range as variant records -- adjacent
 * deleted positions merged into one run, the inserted allele inside the record, a genotype on every record.  Over the window
 * positions [first, first + count), with kinds, alt, n_alt of the call rule, position g in ascending order gives up to three
 * records, in this order:
 *   DEL  when kinds has LRM_CALL_DEL and g == first or position g - 1 has no LRM_CALL_DEL.  len: the consecutive positions
 *        from g on, inside the range, that have LRM_CALL_DEL -- runs are cut at both ends of the range and nowhere else.
 *        n_alt = n_del, n_ref = n_eq and depth are those of g, the run's FIRST position; alt = 0.
 *   SNV  when kinds has LRM_CALL_SNV.  len = 1; alt, n_alt as in the call rule; n_ref = n_eq.
 *   INS  when kinds has LRM_CALL_INS.  n_alt = n_ins, n_ref = n_eq; on an accumulator with insertion planes len, bases, n_col0
 *        and ins_flags are the inserted allele of the position (lrm_pileup_ins_allele_host), otherwise 0.
 *   gt   2 when 100 * n_alt >= hom_pct * depth (64-bit products), else 1.
 * Options: hom_pct == 0 means 70; hom_pct > 100, a nonzero reserved word or refused call options are refused. */
typedef struct lrm_pileup_variant_options { lrm_pileup_call_options call; uint32_t hom_pct, reserved[3]; } lrm_pileup_variant_options;
typedef struct lrm_pileup_variant {    /* 48 bytes, 16-byte aligned */
    uint64_t pos;                      /* the text position (DEL: of the run's first deleted base) */
    uint32_t len, depth;
    uint32_t n_ref, n_alt, n_col0;
    uint8_t kind, ref, alt, gt;        /* kind: exactly one of LRM_CALL_SNV / _DEL / _INS; ref: the text byte at pos as stored */
    uint8_t bases[8];
    uint8_t ins_flags, pad[7];         /* LRM_INS_ENTERS, LRM_INS_FULL; the padding is zero */
} lrm_pileup_variant;
/* The records of window positions [first, first + count), first + count <= hi - lo and 3 * count < 2^32 (checked: ranks are
 * 32-bit), into d_vars (cap records in device memory, 16-byte aligned; may be NULL with cap == 0).  *d_n_vars (device
 * memory, 8-byte aligned) gets the total whether or not the table fits; records from index cap on are not written and
 * nothing outside d_vars[0 .. cap) is touched.  opt NULL: the defaults.  Works on plain accumulators and on accumulators with
 * insertion planes.  Everything is asynchronous on `stream`: no host wait; the counters are not modified.  The scratch is
 * that of lrm_pileup_sites_dev (allocated by the first call of any of the three) plus 8 more bytes per tile, which the
 * first call allocates and lrm_pileup_bytes counts from then on. */
int lrm_pileup_variants_dev(lrm_pileup *pl, const lrm_pileup_variant_options *opt, uint64_t first, uint64_t count,
                            lrm_pileup_variant *d_vars, uint64_t cap, uint64_t *d_n_vars, void *stream);
/* The same rule on records the caller holds, usable without a GPU; cols, ins_words, ins_cols and content as for
 * lrm_pileup_polish_host, position k of the range is text position pos0 + k.  out: cap records (may be NULL with cap == 0).
 * Returns the total whether or not it fits, < 0 for refused options or arguments. */
int64_t lrm_pileup_variants_host(const lrm_pileup_col *cols, const uint32_t *ins_words, uint32_t ins_cols, const char *content,
                                 uint64_t pos0, uint64_t count, const lrm_pileup_variant_options *opt, lrm_pileup_variant *out, uint64_t cap);
/* VCF 4.2 text.  lrm_vcf_header: ##fileformat, one ##contig=<ID=,length=> per sequence, the INFO and FORMAT lines used below,
 * the column line with `sample` (NULL: SAMPLE).  lrm_pileup_variants_format_vcf: one line per record,
 *   name  POS  .  REF  ALT  .  .  DP=<depth>  GT:AD  <0/1|1/1>:<n_ref>,<n_alt>
 * SNV: POS is pos (1-based), REF the text byte, ALT alt.  DEL: POS is that of the base before the run, REF that base plus the
 * len deleted text bytes, ALT that base; a run on a sequence's first base: POS 1, REF the deleted bytes plus the base behind
 * them, ALT that base.  INS: POS is pos, REF the text byte, ALT the text byte plus bases[0 .. len), <INS> when len == 0;
 * ;INSFULL behind DP when LRM_INS_FULL is set.  Text bytes print in upper case.  The sequence of a record is the entry of mta
 * that holds pos; content: the text (host memory).  Both return the text length (NUL-terminated, the NUL not counted), < 0
 * when buf (buflen bytes) is too small or an argument is bad (a pos in no sequence, a run that leaves its sequence). */
int64_t lrm_pileup_variants_format_vcf(const lrm_mta_entry *mta, int mta_len, const char *content, const lrm_pileup_variant *vars,
                                       uint64_t count, char *buf, int64_t buflen);
int64_t lrm_vcf_header(const lrm_mta_entry *mta, int mta_len, const char *sample, char *buf, int64_t buflen);

/* SPLIT READS (lrm_map_options.split; docs/GACT_SPEC.md, "Split reads"): the soft-clipped ends of a batch that went through
 * the anchored extension with end clipping, mapped as reads of their own.  For read i with n = lens[i] bases, R the read as
 * the extension left it and (cl, cr) its lrm_clip: the left segment R[0 .. cl) if cl >= M, then the right segment
 * R[n - cr .. n) if cr >= M; reads ascending, left before right, M = split_min_len (0 = 200, else 50..2^20). */
#define LRM_SPLIT_MIN_DEFAULT 200
#define LRM_SEG_RIGHT 1u               /* lrm_segment.flags: the segment is the read's right end */
#define LRM_SEG_ALIGNED 2u             /*   REPORTED: it has a locus (meta_r != 0) and was extended from an anchor of its own */
typedef struct lrm_segment { uint32_t read, start, len, flags; } lrm_segment;   /* start: in R's coordinates */

/* The segment table from clip counts: pure host arithmetic, usable without a GPU.  seg_out holds up to cap records (may be
 * NULL when cap == 0); *n_seg is the number of segments in any case.  0 ok, -3 more than cap segments (nothing written),
 * -1 bad argument (split_min_len outside its range). */
int lrm_split_plan(const uint32_t *lens, const lrm_clip *clip, uint64_t n, uint32_t split_min_len, lrm_segment *seg_out,
                   uint64_t cap, uint64_t *n_seg);
/* The 'S' run at either end of one alignment: of its op bytes (is_text == 0) or of its run-length text (is_text != 0:
 * cig->cigar is NUL-terminated, lrm_map_options.cigar_text).  The host-buffer batch calls return no lrm_clip records;
 * this recovers them.  No alignment (n_cigar_op <= 0, "*"): 0, 0. */
int lrm_clip_of_cigar(const lrm_cigar *cig, int is_text, uint32_t *left, uint32_t *right);

/* Device buffers of the second pass, owned by the caller, for up to cap segments: the segment table, the segment batch
 * (row s at rows + s*row_stride, 16-byte aligned, row_stride a multiple of 16 and > the longest segment) and, per segment,
 * everything lrm_seed_batch_dev + lrm_extend_batch_clipped_dev return for a batch made of those rows (store_stride >=
 * 2*L + L/8 + 2 for the longest segment L, a multiple of 4; checked). */
typedef struct lrm_split_dev {
    uint64_t cap;
    lrm_segment *seg;
    char *rows; uint64_t row_stride;
    uint32_t *lens;
    lrm_entry *best;
    uint8_t *store; uint64_t store_stride;
    int32_t *n_ops, *score;
    lrm_seq_meta *meta; int32_t *meta_r;
    lrm_anchor *anchor;
    lrm_clip *clip;
} lrm_split_dev;
/* Call after lrm_extend_batch_clipped_dev on the same stream: d_reads, d_lens, d_clip are that call's.  p, gp, anchor_min_len,
 * clip_penalty, clip_end_bonus: as the primary pass had them.  The stage marks and counts the segments on the device, and
 * THE COUNT CROSSES TO THE HOST (8 bytes into pinned memory; the call sleeps on an event until they are there): this is the
 * one place a *_dev call waits for the device, everything before it on the stream included.  Then it gathers the segment
 * rows and runs the seed stage and the clipped anchored extension over them on ws_seg, in chunks of ws_seg's n_max rows
 * when there are more segments than that; these launches are asynchronous like those of the other *_dev calls.
 * *n_seg = the number of segments.  More than out->cap: -3, *n_seg says how many, no result array is written.
 * ws_seg: a workspace from lrm_workspace_create for (rows per chunk, longest segment, p.seed_len, p.thres).  The workspace
 * of the primary pass MAY be passed: its scratch is idle once the primary's extension has been issued on the same stream,
 * it holds reads at least as long as any segment, and a batch with more segments than its n_max goes through it in chunks
 * (its counters and its timing record then describe the two passes together). */
int lrm_split_batch_dev(lrm_index *idx, lrm_workspace *ws_seg, const char *d_reads, uint64_t stride, const uint32_t *d_lens,
                        uint64_t n, const lrm_clip *d_clip, lrm_params p, lrm_gact_params gp, uint32_t anchor_min_len,
                        uint32_t clip_penalty, uint32_t clip_end_bonus, uint32_t split_min_len, const lrm_split_dev *out,
                        uint64_t *n_seg, void *stream);

/* The second pass with HOST buffers, over a batch the caller has just got back from lrm_map_batch / lrm_map_batch_wait with
 * lrm_map_options.clip: reads_buf, lens, cig, meta, meta_r as returned.  It takes the clip counts from cig (rows, dense or
 * cigar_text layout, as opt says), plans the segments, gathers their bases on the host (with opt->keep_reads the caller's
 * copy of a reverse-strand read was not reverse-complemented: meta_r != 0 && strand == 1 -- the gather does it) and sends
 * that batch through lrm_map_batch_submit / _wait with opt (split and keep_reads themselves ignored: the segment rows come
 * back as the extension left them).  Only the clipped bases cross the link a second time.  Same segment table and same
 * per-segment bytes as lrm_split_batch_dev; group handles work.  out->cig[s] is in opt's layout inside out->store.
 * opt == NULL: the handle's default options.  -3: more than out->cap segments (out->n_seg says how many). */
typedef struct lrm_split_out {
    uint64_t cap, n_seg;               /* n_seg: set by the call */
    lrm_segment *seg;
    char *rows; uint64_t row_stride;   /* may be pinned (lrm_host_alloc); row_stride a multiple of 16 and > the longest segment */
    uint32_t *lens;
    lrm_entry *best;
    lrm_cigar *cig;
    uint8_t *store; uint64_t store_stride;
    int *score;
    lrm_seq_meta *meta; int *meta_r;
    lrm_anchor *anchor;
    lrm_clip *clip;
} lrm_split_out;
int lrm_split_batch(lrm_index *idx, const char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                    const lrm_cigar *cig, const lrm_seq_meta *meta, const int *meta_r, lrm_params p, lrm_gact_params gp,
                    const lrm_map_options *opt, lrm_split_out *out);

/* SECONDARY ALIGNMENTS (docs/GACT_SPEC.md, "Secondary alignments"): the mapping-quality stage counts the seed hits of the
 * best OTHER place (lrm_mapq.n2); this stage finds where that place is and extends the read there.  Asked for per CALL, like
 * the mapping quality: nothing runs or is allocated unless one of the entry points below is called, and every other output
 * is the same bytes with it or without.  A read is a CANDIDATE iff it has a locus, its record has no LRM_MAPQ_OVERFLOW,
 * n2 >= H and 100 * n2 >= pct * n1 (H = min_hits: 0 = 8, else 1..65535; pct = ratio_pct: 0 = 50, else 1..100).  Its RIVAL
 * entry: of the fullest (histogram, bucket) pair of the rival vote (ties: the smallest bucket, histogram 0 first) the fullest
 * sub-bucket of 2^s diagonals (s = max(4, log2(radius) - 10); ties: the smallest) -- key = its smallest hit, val = its hits,
 * bucket = key >> 4.  A read that is not a candidate has an all-zero entry.  One secondary per read; secondaries of split
 * segments are out of scope. */
#define LRM_SEC_ALIGNED 1u             /* lrm_secondary.flags: REPORTED -- resolved, extended (in the anchored modes: from an
                                          anchor of its own) and not a duplicate */
#define LRM_SEC_DUPLICATE 2u           /*   resolved to the primary's sequence and strand, less than len/2 bases from it: the
                                          tail of the primary's own cluster */
typedef struct lrm_secondary { uint32_t read, hits, flags, pad; } lrm_secondary;     /* 16 bytes; hits: the rival entry's val */
typedef struct lrm_secondary_options {
    uint32_t struct_size;      /* sizeof(lrm_secondary_options) of the caller's header (0: all of it) */
    uint32_t min_hits;         /* H */
    uint32_t ratio_pct;        /* pct */
    uint32_t anchored;         /* the extension the candidates go through: 0 classic, 1 anchored (clip implies it) */
    uint32_t anchor_min_len;   /*   as lrm_map_options.anchor_min_len */
    uint32_t clip;             /*   1: anchored with end clipping */
    uint32_t clip_penalty;     /*   P */
    uint32_t clip_end_bonus;   /*   B */
} lrm_secondary_options;

/* The rival entries of a batch (d_rival: n lrm_entry in device memory): call it behind lrm_seed_batch_mapq_dev on the same
 * workspace and stream, with that call's d_lens, n, p, d_best and d_mapq, BEFORE any other seed stage runs on that workspace
 * -- it walks the survivor lists that call left there.  (The split stage, handed the primary's workspace as ws_seg, is such a
 * stage: lrm_rival_dev / lrm_secondary_batch_dev first, then lrm_split_batch_dev.)  Refused otherwise: every seed stage
 * stamps the workspace with the d_best and n it ran for and with whether it wrote the deciding phases (a plain
 * lrm_seed_batch_dev does not), and this call, lrm_secondary_batch_dev and the mapping-quality stage return -1 ("the
 * workspace did not run the seed stage of this batch with the phase output") before any launch unless d_best and n are the
 * stamp's.  One kernel, asynchronous; it checks what the mapping-quality stage checks. */
int lrm_rival_dev(lrm_index *idx, lrm_workspace *ws, const uint32_t *d_lens, uint64_t n, lrm_params p,
                  const lrm_entry *d_best, const lrm_mapq *d_mapq, uint32_t min_hits, uint32_t ratio_pct,
                  lrm_entry *d_rival, void *stream);
/* The rule on the host over the hits of ONE read (keys: SA[row] - j of every survivor of the evidence phases, 64-bit wrap
 * kept), usable without a GPU: *out = the rival entry (zeros for a read that is not a candidate).  slots: 0 = LRM_MAPQ_SLOTS.
 * Returns 1 for a candidate, 0 otherwise, -1 for a bad argument. */
int lrm_rival_host(const uint64_t *keys, uint64_t n_keys, const lrm_entry *best, uint32_t len, uint32_t min_hits,
                   uint32_t ratio_pct, uint32_t slots, lrm_entry *out);
/* The candidate table from the records: reads ascending, hits = 0 (the rival's val is known only behind the rival kernel),
 * flags = 0.  Pure host arithmetic.  table holds up to cap records (may be NULL when cap == 0); *n_sec is the number of
 * candidates in any case.  0 ok, -3 more than cap candidates (nothing written), -1 bad argument. */
int lrm_secondary_plan(const lrm_mapq *mapq, uint64_t n, uint32_t min_hits, uint32_t ratio_pct, lrm_secondary *table,
                       uint64_t cap, uint64_t *n_sec);

/* Device buffers of the stage, owned by the caller, for up to cap candidates: the table, the candidate batch (row s = read
 * table[s].read AS SEQUENCED at rows + s*row_stride, 16-byte aligned, row_stride a multiple of 16 and > the longest
 * candidate; every byte of a row behind the read's end is 0), their lengths, their rival entries and, per candidate,
 * everything the extension call of the chosen mode returns for a batch made of those rows with best = the rival entries
 * (store_stride as that call wants it for the longest candidate, a multiple of 4; anchor / clip may be NULL in the modes
 * that do not write them). */
typedef struct lrm_secondary_dev {
    uint64_t cap;
    lrm_secondary *table;
    char *rows; uint64_t row_stride;
    uint32_t *lens;
    lrm_entry *rival;
    uint8_t *store; uint64_t store_stride;
    int32_t *n_ops, *score;
    lrm_seq_meta *meta; int32_t *meta_r;
    lrm_anchor *anchor;
    lrm_clip *clip;
} lrm_secondary_dev;
/* Call behind the primary's seed stage WITH mapping quality and its extension, on the same workspace and stream: d_reads
 * (as the extension left them: a read with d_meta_r != 0 && d_meta.strand == 1 was reverse-complemented in place, the gather
 * undoes that), d_lens, d_best, d_mapq, d_meta, d_meta_r are those calls'.  d_meta == NULL (then d_meta_r too): the reads are
 * as sequenced, and no candidate is tested for LRM_SEC_DUPLICATE.  The stage runs the rival kernel, counts the candidates on
 * the device, and THE COUNT CROSSES TO THE HOST (8 bytes; the call sleeps on an event, as lrm_split_batch_dev does); then it
 * marks the table, gathers the rows, runs the unchanged extension stage so names over them on ws with gp, and sets the flags.
 * *n_sec = the number of candidates.  More than out->cap: -3, *n_sec says how many, no result array is written.  The first
 * call on a workspace allocates 24 bytes per read of its n_max, 8 bytes per 256 reads and 8 bytes; lrm_workspace_bytes grows
 * by it.  "As sequenced" holds for reads of upper-case A, C, G, T and N: the gather undoes the reverse complement with the
 * extension's own base map, which folds case and turns every other byte into N.
 * so == NULL: the defaults, classic extension. */
int lrm_secondary_batch_dev(lrm_index *idx, lrm_workspace *ws, const char *d_reads, uint64_t stride, const uint32_t *d_lens,
                            uint64_t n, const lrm_entry *d_best, const lrm_mapq *d_mapq, const lrm_seq_meta *d_meta,
                            const int32_t *d_meta_r, lrm_params p, lrm_gact_params gp, const lrm_secondary_options *so,
                            const lrm_secondary_dev *out, uint64_t *n_sec, void *stream);

/* The results of the stage in HOST memory, for the callers that print them (lrm_sam_format_secondary): what a caller
 * downloads from an lrm_secondary_dev, with cig[s] = {the op bytes of candidate s inside store (or its run-length text),
 * n_ops, score}.  n_sec: the number of candidates the arrays hold. */
typedef struct lrm_secondary_out {
    uint64_t cap, n_sec;
    lrm_secondary *table;
    char *rows; uint64_t row_stride;
    uint32_t *lens;
    lrm_entry *rival;
    lrm_cigar *cig;
    uint8_t *store; uint64_t store_stride;
    int *score;
    lrm_seq_meta *meta; int *meta_r;
    lrm_anchor *anchor;
    lrm_clip *clip;
} lrm_secondary_out;
/* The stage with HOST buffers, over a batch the caller has just got back from lrm_map_batch_submit_mapq / _wait: reads_buf,
 * lens, mapq, meta, meta_r as returned (meta == NULL, then meta_r too: the reads are as sequenced, no duplicate test).  It plans
 * the candidates from the records (lrm_secondary_plan), gathers them on the host as sequenced (without opt->keep_reads the
 * caller's copy of a read with meta_r != 0 && strand == 1 was reverse-complemented in place: the gather undoes that, A/C/G/T of
 * either case to the upper-case complement, any other byte to N, as the device does), uploads only those rows and runs seed +
 * mapping quality + rival + the extension `so` names for them in ONE synchronous device pass on a workspace of its own, then
 * downloads.  The host pipeline is not touched.  A read's records do not depend on its batch, so the table and the
 * per-candidate results equal lrm_secondary_batch_dev's.  out->cig[s] is in opt's layout inside out->store (rows; dense_results:
 * the used op bytes back to back in 16-byte units; cigar_text: the NUL-terminated run-length text, likewise); row_stride a
 * multiple of 16 above the longest candidate, store_stride a multiple of 16 and what the extension mode needs.  On a group
 * handle the first device does the pass.  opt == NULL: the handle's default options.  -3: more than out->cap candidates
 * (out->n_sec says how many, nothing else is written). */
int lrm_secondary_batch(lrm_index *idx, const char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                        const lrm_mapq *mapq, const lrm_seq_meta *meta, const int *meta_r, lrm_params p, lrm_gact_params gp,
                        const lrm_map_options *opt, const lrm_secondary_options *so, lrm_secondary_out *out);

/* Counters of the last *_dev call on this workspace (device->host copy, syncs
 * the stream): vote items per table tier, reads decided in
 * phase 0, GACT tiles.  For tests / bench bookkeeping only. */
typedef struct lrm_stats {
    uint64_t vote_tier2_items;      /* (read,phase) items voted by a whole workgroup in one pass (192 < hits <= 1152) */
    uint64_t vote_tier3_items;      /* ... in several passes over the workgroup table (hits > 1152) */
    uint64_t reads_decided_phase0;  /* reads whose vote passed 0.6 in phase 0 */
    uint64_t gact_tiles;
    /* with lrm_workspace_set_counting(ws, 1): the memory requests the DEVICE layout made in the last seed call */
    uint64_t seeds_evaluated;       /* seed positions searched */
    uint64_t seed_table_lookups;    /* 8-byte entries of the seed tables (lchash image or long table) read */
    uint64_t seed_rank_requests;    /* 16-byte {prefix, mask} pairs of the occ blocks read (1 or 2 per backward step) */
    uint64_t vote_redo_items;       /* (read, phase) items the fast vote kernel left to the exact one */
    /* with lrm_workspace_set_counting(ws, 1): the paths the bit-sliced extension kernel took, added up over its launches
     * since the last seed call (or since the workspace was made) */
    uint64_t bs_wave_tiles;         /* rounds of a wavefront's tile loop (64 lanes, one tile each) */
    uint64_t bs_pass1_pairs_masked; /* pass-1 pairs of anti-diagonals whose even step ran the masked (free-exit) form */
    uint64_t bs_pass1_pairs_plain;  /* ... the plain form */
    uint64_t bs_blocks_full;        /* traceback blocks recomputed in full width with the masked step */
    uint64_t bs_blocks_windowed;    /* ... on the 32-point window */
    uint64_t bs_blocks_skipped;     /* ... left out: no lane of the wavefront was still walking */
    uint64_t bs_refill_rounds;      /* rounds of the read queue (one atomic each) */
} lrm_stats;
/* Counting builds of the seed kernel and of the bit-sliced extension kernel for the NEXT calls on this workspace
 * (bench bookkeeping: slower, never timed). */
int lrm_workspace_set_counting(lrm_workspace *ws, int enable);
int lrm_workspace_stats(lrm_workspace *ws, lrm_stats *out, void *stream);

/* Per-kernel timing with HIP events recorded on the launch stream (bench bookkeeping).
 * Kernel order: pack2bit, seed_search, vote, decide, locus_resolve, revcomp, gact (byte kernels),
 * bs_pack_reads, gact_bs (bit-sliced kernel + expansion).  The anchored mode adds its anchor scan to the
 * locus_resolve slot, its job builder to the revcomp slot, its end clipping and its stitch to the slot of the extension
 * kernel.  The split stage (lrm_split_batch_dev) books its own kernels -- compact_count / compact_scan / compact_mark,
 * compact_gather, split_flag -- into the revcomp slot of ws_seg, next to the seed and extension kernels of the segment batch.
 * lrm_workspace_timing synchronises the stream, ADDS the elapsed milliseconds and launch counts
 * of everything recorded since the last call into ms[LRM_N_KERNELS] / launches[LRM_N_KERNELS], and
 * resets the record. */
#define LRM_N_KERNELS 9
int lrm_workspace_set_timing(lrm_workspace *ws, int enable);
int lrm_workspace_timing(lrm_workspace *ws, double *ms, uint64_t *launches, void *stream);
const char *lrm_kernel_name(int kernel);

/* Debug/parity taps (tests only): per-seed search results of one read as the
 * seed kernel produced them, in (phase, ordinal) order: j, rr, k, l. */
int lrm_debug_seed_search(lrm_index *idx, const char *read, uint32_t len, uint32_t seed_len,
                          uint32_t thres, int32_t *j_out, uint64_t *rr_out, uint64_t *k_out,
                          uint64_t *l_out, uint64_t cap, uint64_t *n_out);

/* Debug/parity tap (tests only): what the vote kernels left for the first n reads of the last seed call on this
 * workspace -- six words {key1, val1, bucket1, key2, val2, bucket2} per (read, phase), read-major, seed_len + 1 phases per
 * read.  Only the phases the call evaluated are meaningful (phase 0 always is). */
int lrm_debug_vote_results(lrm_workspace *ws, uint64_t n, uint64_t *out, void *stream);

/* Test-only: force the multi-pass vote tier of this handle's batches into overflow (a pass limit above the table size
 * and a small table); 0, 0 restores the defaults. */
int lrm_debug_set_vote_limits(lrm_index *idx, uint32_t t3_limit, uint32_t t3_slots);

/* Test-only: the mapping-quality stage of this handle's batches (every replica) uses a rival table of `slots` slots: 0 =
 * LRM_MAPQ_SLOTS, else a power of two 16..LRM_MAPQ_SLOTS -- a small table forces LRM_MAPQ_OVERFLOW. */
int lrm_debug_set_mapq_slots(lrm_index *idx, uint32_t slots);

/* Tuning sessions only (tools/): re-read the LRM_* overrides for the batch calls of this handle (normally they are
 * read once, when the handle is created). */
int lrm_debug_reload_env(lrm_index *idx);

/* RCCL self-test (tests only): dlopen + ncclCommInitAll + a 1-rank grouped ncclBroadcast of `bytes` bytes on
 * `device`.  0 ok, 1 librccl not loadable (lrm_index_upload_multi then uses hipMemcpyPeer), <0 error. */
int lrm_debug_rccl_selftest(int device, uint64_t bytes);

/* Anchor tap (tests only): the anchor of ONE read (oriented like the forward strand) at ONE voted locus `loc`, a text
 * position on the forward half of a sequence; out->left_ops is 0 (nothing is extended). */
int lrm_debug_anchor(lrm_index *idx, const char *read, uint32_t len, uint64_t loc, uint32_t min_len, lrm_anchor *out);

/* Direct kernel tap (tests only): simple_gact on one (q, d) pair. */
int lrm_debug_gact(const char *q, int n, const char *d, int m, lrm_gact_params gp,
                   uint8_t *ops, int *n_ops, int *score, int device);
/* ... with the kernel chosen by the caller (lrm_map_options.gact_impl values) */
int lrm_debug_gact_impl(const char *q, int n, const char *d, int m, lrm_gact_params gp, int impl,
                        uint8_t *ops, int *n_ops, int *score, int device);

/* Job-table tap (tests only): n (read, target) pairs as ONE job table through the extension's own plan and launch, target
 * lengths set.  Job k is read row k (reads + k * stride, lens[k] bases) against text[toffs[k], toffs[k] + tlens[k]): the
 * caller lays the targets out, so it decides the locus residue and what follows a target.  meta_r: null, or per job 0 =
 * fenced.  store (n rows of store_stride >= lens[k] + tlens[k] bytes), n_ops and score go to the device as they are and
 * come back as the kernels left them.  counters: null, or 8 words: gact_tiles, then the counters of the bit-sliced
 * kernel's counting build in the order of lrm_stats (bs_wave_tiles .. bs_refill_rounds; all 0 unless `count`). */
typedef struct lrm_debug_gact_table {
    uint64_t n;
    const char *reads; uint64_t stride; const uint32_t *lens;
    const char *text; uint64_t text_len; const uint64_t *toffs; const uint32_t *tlens;
    const int32_t *meta_r;
    uint8_t *store; uint64_t store_stride; int32_t *n_ops; int32_t *score;
    uint64_t *counters;
} lrm_debug_gact_table;
/* impl, bs_waves: as lrm_map_options.gact_impl / bs_waves; count: the counting build of the bit-sliced kernel */
int lrm_debug_gact_jobs(const lrm_debug_gact_table *t, lrm_gact_params gp, int impl, uint32_t bs_waves, int count, int device);

#ifdef __cplusplus
}
#endif
#endif /* LRM_ACCEL_H */
