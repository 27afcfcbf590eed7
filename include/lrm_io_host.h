/*
 * lrm_io_host.h -- the steps either side of the hot path, host C++ in
 * liblrm_accel.so: FASTA/FASTQ batch loader, SAM header / records, run-length CIGAR text, and the
 * whole `accaln ref.fa reads.fq` flow on the GPU path.
 *
 *   reads_load + refactor_reads_seq   accaln.c:45-58, alnmain.c:87-103   -> lrm_reader_*
 *   gen_sam_header                    alnmain.c:62-75                    -> lrm_sam_header
 *   SAM record printing               alnmain.c:485-527                  -> lrm_sam_format (_split, _mapq, _md)
 *   parse_cigar (gact submodule, source absent; PARITY UNPINNED)         -> lrm_parse_cigar
 *   single_end                        alnmain.c:277-551                  -> lrm_accaln
 *   (no counterpart: the reference prints SAM only)                      -> lrm_paf_format, lrm_accaln_paf, lrm_accaln_pileup[_vcf]
 */
#ifndef LRM_IO_HOST_H
#define LRM_IO_HOST_H

#include "lrm_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One batch in the layout refactor_reads_seq builds: read i at seqs + i*stride, NUL padded,
 * stride = max_len + 1.  quals[i] is NULL for FASTA records. */
typedef struct lrm_read_batch {
    uint64_t n, stride;
    uint32_t max_len;
    char *seqs;
    uint32_t *lens;
    char **names;
    char **quals;
    /* storage behind names[] / quals[] (one block each), and whether seqs is the caller's buffer
     * (lrm_reader_next_into); lrm_read_batch_free looks at them */
    char *name_arena, *qual_arena;
    int seqs_borrowed;
} lrm_read_batch;

typedef struct lrm_reader lrm_reader;

/* FASTA / FASTQ, plain or gzip (zlib), multi-line records, name = header up to the first blank. */
int lrm_reader_open(lrm_reader **out, const char *path);
/* Loads up to batch_size records; returns the number loaded (0 at end of file), <0 on error
 * (-2: quality string of a different length, like kseq). */
int64_t lrm_reader_next(lrm_reader *r, uint64_t batch_size, lrm_read_batch *out);
/* The same with the sequences written into a buffer of the caller (e.g. pinned memory from lrm_host_alloc, so that the
 * batch can be handed to lrm_map_batch_submit without a staging copy) when n * (max_len + 1) <= seq_cap; otherwise the
 * library allocates as lrm_reader_next does.  out->seqs_borrowed tells which. */
int64_t lrm_reader_next_into(lrm_reader *r, uint64_t batch_size, lrm_read_batch *out, void *seq_buf, uint64_t seq_cap);
void lrm_read_batch_free(lrm_read_batch *b);
void lrm_reader_close(lrm_reader *r);

/* Run-length SAM CIGAR from op bytes ('=' and 'X' print as M); "*" for an empty alignment.
 * Returns the text length, <0 if buf is too small. */
int lrm_parse_cigar(const uint8_t *ops, int n_ops, char *buf, int buflen);

/* @SQ per sequence, @RG with ID accaln<rg_id> (the reference uses time(NULL)), @PG.
 * Returns malloc'd text (free with lrm_free). */
char *lrm_sam_header(const lrm_mta_entry *mta, int mta_len, long rg_id, uint64_t *len_out);

/* One SAM line per read, alnmain.c:500-525 field for field.  Unmapped reads (meta_r == 0 or
 * score == -1; the reference prints an uninitialised struct there) print RNAME "*", POS 0, CIGAR "*".
 * Returns malloc'd text (free with lrm_free). */
char *lrm_sam_format(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len,
                     const lrm_cigar *cig, const int *score, const lrm_seq_meta *meta,
                     const int *meta_r, uint64_t n, uint64_t *len_out);
/* The same with SPLIT READS (docs/GACT_SPEC.md, "Split reads"): `split` is what lrm_split_batch returned for this batch
 * (NULL or no segment: exactly the lines of lrm_sam_format).  Right behind a read's primary line comes one supplementary line
 * (FLAG 2048, + 16 when its strand relative to the read as sequenced is reverse) per REPORTED segment: SEQ the segment row,
 * QUAL the matching slice of the read's qualities, CIGAR <hl>H + the segment's own run-length CIGAR + <hr>H.  The primary and
 * its supplementary lines name each other in SA:Z (rname,pos,strand,<c5>S<q>M<d>D|I<c3>S,255,ED;).
 * cigar_is_text: cig[i].cigar and split->cig[s].cigar are run-length text (lrm_map_options.cigar_text), not op bytes;
 * revcomp_here: the batch ran with keep_reads -- reverse-strand reads are reverse-complemented while they are printed. */
char *lrm_sam_format_split(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                           const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                           int revcomp_here, const lrm_split_out *split, uint64_t *len_out);
/* The same with MAPPING QUALITY (docs/GACT_SPEC.md, "Mapping quality"): mq is what lrm_map_batch_submit_mapq returned for this
 * batch (NULL: exactly the lines of lrm_sam_format_split).  Column 5 of a mapped read is mq[i].mapq instead of 255, every
 * read's line gains v1:i:<n1>\tv2:i:<n2> behind ED:I, and the primary's entry inside the SA:Z of its supplementary lines
 * carries the primary's MAPQ.  The split segments have no records: their lines and their own SA:Z entries keep 255. */
char *lrm_sam_format_mapq(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                          const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                          int revcomp_here, const lrm_split_out *split, const lrm_mapq *mq, uint64_t *len_out);
/* The same with NM:i and MD:Z (docs/GACT_SPEC.md, "Difference events and MD:Z"): sum, diff_off, diff_cnt and events are what
 * lrm_map_batch_submit_ex2 returned for this batch -- the summary records, and read i's events at events[diff_off[i] ..
 * diff_off[i] + diff_cnt[i]) (events == NULL: exactly the lines of lrm_sam_format_mapq).  A mapped read's primary line gains
 * NM:i:<n_x + n_ins + n_del>\tMD:Z:<lrm_md_format's text> behind ED:I (behind v1:i / v2:i with mq); a read without an
 * alignment, or one whose events found no room (diff_off[i] == UINT64_MAX), gains nothing.  Supplementary lines gain nothing:
 * the segment batch of lrm_split_out has no records. */
char *lrm_sam_format_md(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                        const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                        int revcomp_here, const lrm_split_out *split, const lrm_mapq *mq, const lrm_aln_summary *sum,
                        const uint64_t *diff_off, const uint32_t *diff_cnt, const uint32_t *events, uint64_t *len_out);
/* The same with SECONDARY ALIGNMENTS (docs/GACT_SPEC.md, "Secondary alignments"): sec holds the results of the secondary
 * stage for this batch (NULL or no candidate: exactly the text of lrm_sam_format_md).  Behind a read's primary and supplementary
 * lines comes one line per REPORTED secondary (LRM_SEC_ALIGNED): FLAG 256 (+ 16 when it is on the reverse strand of the read as
 * sequenced), its own RNAME and POS = off + 1, MAPQ 0, its own run-length CIGAR with soft clips as S, SEQ * and QUAL *,
 * ED:I:<score>\ttp:A:S.  Every other line is unchanged. */
char *lrm_sam_format_secondary(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                               const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                               int revcomp_here, const lrm_split_out *split, const lrm_mapq *mq, const lrm_aln_summary *sum,
                               const uint64_t *diff_off, const uint32_t *diff_cnt, const uint32_t *events,
                               const lrm_secondary_out *sec, uint64_t *len_out);

/* PAF (docs/GACT_SPEC.md, "Alignment summary and PAF"): one line per MAPPED read -- an unmapped one (meta_r == 0 or score == -1)
 * prints nothing --, every number of it taken from the read's alignment summary record (sum: required, what
 * lrm_map_batch_submit_ex or lrm_aln_summary_dev returned for this batch).  Tab-separated, with cl / cr the record's clips:
 *   qname  qlen  qstart  qend  strand  tname  tlen  tstart  tend  matches  block  mapq  tags
 * qstart, qend: on the read as sequenced -- cl, qlen - cr on the forward strand; cr, qlen - cl on the reverse strand
 * (meta.strand == 1).  tstart = meta.off, tend = meta.off + target span, matches = n_eq, block = the block length, mapq =
 * mq[i].mapq (255 without mq).  Tags: NM:i  ED:i:<score>  tp:A:P  de:f:<%.4f of (n_x + ins_runs + del_runs) / (n_eq + n_x +
 * ins_runs + del_runs), 0.0000 for a zero denominator>  cg:Z:<the run-length CIGAR as lrm_parse_cigar prints it>, and with
 * mq v1:i:<n1>  v2:i:<n2>.  cigar_is_text: cig[i].cigar is run-length text (lrm_map_options.cigar_text), not op bytes.
 * Returns malloc'd text (free with lrm_free); NULL on a bad argument. */
char *lrm_paf_format(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                     const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                     const lrm_aln_summary *sum, const lrm_mapq *mq, uint64_t *len_out);

/* `accaln genome reads [batch seed_len thres]` on the GPU path: loads the index files next to
 * `genome`, maps `reads_path` batch by batch, writes SAM to `sam_path`.  total/valid are the
 * reference's "Sensitivity: valid/total" counters (alnmain.c:541). */
int lrm_accaln(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
               lrm_gact_params gp, int device, long rg_id, uint64_t *total, uint64_t *valid);
/* ... with options (NULL: lrm_accaln).  Taken from opt: anchored, anchor_min_len -- SAM POS is then the alignment's first
 * text base (meta.off + 1 of the moved meta) --, clip and its two parameters, split and split_min_len (needs clip: after a
 * batch's wait its clipped ends go through lrm_split_batch and come out as supplementary records, lrm_sam_format_split;
 * total / valid keep counting reads); the other fields are this flow's own choice. */
int lrm_accaln_opt(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                   lrm_gact_params gp, int device, long rg_id, uint64_t *total, uint64_t *valid,
                   const lrm_map_options *opt);
/* ... with MAPPING QUALITY (docs/GACT_SPEC.md, "Mapping quality"; mapq == 0: lrm_accaln_opt): every batch goes through
 * lrm_map_batch_submit_mapq and is printed by lrm_sam_format_mapq -- column 5 is the record's MAPQ instead of 255, v1:i / v2:i
 * follow ED:I.  The flag travels next to the options, not inside them: lrm_map_options keeps its size. */
int lrm_accaln_mapq(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                    lrm_gact_params gp, int device, long rg_id, uint64_t *total, uint64_t *valid,
                    const lrm_map_options *opt, int mapq);
/* ... with NM:i and MD:Z (md == 0: lrm_accaln_mapq): every batch goes through lrm_map_batch_submit_ex2 and is printed by
 * lrm_sam_format_md.  The event buffer of a batch has room for the bound, the sum of its store strides (a read has no more
 * events than columns; pages the events never touch cost nothing); more events than that is an error of the flow. */
int lrm_accaln_md(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                  lrm_gact_params gp, int device, long rg_id, uint64_t *total, uint64_t *valid,
                  const lrm_map_options *opt, int mapq, int md);
/* ... with SECONDARY ALIGNMENTS (docs/GACT_SPEC.md, "Secondary alignments"; so == NULL: lrm_accaln_mapq with its mode on): the
 * flow of lrm_accaln_mapq, and after a batch's wait its candidates go through lrm_secondary_batch with `so` (thresholds and the
 * extension mode of the candidates) and the batch is printed by lrm_sam_format_secondary: one FLAG 256 line behind the lines
 * of every read with a reported secondary, every other line as lrm_accaln_mapq prints it. */
int lrm_accaln_secondary(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                         lrm_gact_params gp, int device, long rg_id, uint64_t *total, uint64_t *valid,
                         const lrm_map_options *opt, const lrm_secondary_options *so);
/* The flow of lrm_accaln_mapq with PAF output: every batch goes through lrm_map_batch_submit_ex with summary_out (and
 * mapq_out when mapq != 0) and is printed by lrm_paf_format; the file has no header.  total / valid count as in the SAM flow.
 * opt->split != 0 is refused (-1): PAF lines for split segments need summary records of the segment batch, which the
 * fixed-size lrm_split_out cannot carry. */
int lrm_accaln_paf(const char *genome, const char *reads_path, const char *paf_path, lrm_params p, lrm_gact_params gp,
                   int device, uint64_t *total, uint64_t *valid, const lrm_map_options *opt, int mapq);

/* The flow of lrm_accaln_mapq with a PILEUP (docs/GACT_SPEC.md, "Pileup on the host-buffer path and across replicas"; po ==
 * NULL: lrm_accaln_mapq): every batch goes through lrm_map_batch_submit_ex3 onto one accumulator, created behind the index
 * upload with lrm_pileup_create_ins over the window of `seq` -- one sequence of the index, or with -1 everything from the first
 * sequence's first base to the last one's last (32 + 16 * ins_cols bytes of device memory per position: the creation error is
 * the flow's error).  Behind the last wait the flow writes, for each selected sequence in index order from its slice of the window:
 *   sites_path  the lines of lrm_pileup_sites_format for the sites of lrm_pileup_sites_dev with `call`; with ins_cols > 0 every
 *               line ends on the inserted-bases column (lrm_pileup_sites_format_ins)
 *   fasta_path  >name, then the bytes of lrm_pileup_polish_dev, 60 columns a line (ins_cols == 0: the consensus without '-')
 * Either path may be NULL.  sam_path may be NULL here: the reads are mapped and downloaded, nothing is formatted or written;
 * total / valid count as before.  Refused (-1) before any output file is created: min_mapq != 0 with mapq == 0, seq outside
 * [-1, the number of sequences), a nonzero reserved field, ins_cols > 8, call.min_pct > 100. */
typedef struct lrm_accaln_pileup_options {
    uint32_t struct_size, ins_cols, min_mapq, reserved;
    lrm_pileup_call_options call;
    int32_t seq; uint32_t reserved2;
    const char *sites_path, *fasta_path;
} lrm_accaln_pileup_options;
int lrm_accaln_pileup(const char *genome, const char *reads_path, const char *sam_path, lrm_params p, lrm_gact_params gp, int device,
                      long rg_id, uint64_t *total, uint64_t *valid, const lrm_map_options *opt, int mapq,
                      const lrm_accaln_pileup_options *po);
/* lrm_accaln_pileup plus a VCF file (docs/GACT_SPEC.md, "Pileup variants and VCF"; vo == NULL: exactly lrm_accaln_pileup).
 * Behind the last wait the flow also writes vcf_path: lrm_vcf_header with `sample` (NULL: SAMPLE), then for each selected
 * sequence in index order the lines of lrm_pileup_variants_format_vcf for the records of lrm_pileup_variants_dev with po->call
 * and hom_pct over that sequence's slice of the window -- a deleted run therefore never crosses a sequence end.  Refused (-1)
 * before any output file is created: what lrm_accaln_pileup refuses, po == NULL, a struct_size below the struct's, hom_pct >
 * 100, vcf_path == NULL, reserved != 0. */
typedef struct lrm_accaln_vcf_options {
    uint32_t struct_size, hom_pct;
    const char *vcf_path, *sample;
    uint64_t reserved;
} lrm_accaln_vcf_options;
int lrm_accaln_pileup_vcf(const char *genome, const char *reads_path, const char *sam_path, lrm_params p, lrm_gact_params gp, int device,
                          long rg_id, uint64_t *total, uint64_t *valid, const lrm_map_options *opt, int mapq,
                          const lrm_accaln_pileup_options *po, const lrm_accaln_vcf_options *vo);

#ifdef __cplusplus
}
#endif
#endif
