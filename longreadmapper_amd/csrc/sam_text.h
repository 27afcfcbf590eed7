// sam_text.h -- what the accaln flow (accaln_flow.cpp) takes from the SAM formatter (sam_text.cpp): a batch as the
// formatter reads it, the parallel formatting of it, and where the parts of its text go
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/lrm_io_host.h"

// One batch of results on its way into SAM text; built once by whoever has the results, read-only from there on.
struct SamBatch {
    const lrm_read_batch *reads;
    const lrm_mta_entry *mta; int mta_len;
    const lrm_cigar *cig; const int *score; const lrm_seq_meta *meta; const int *meta_r;
    uint64_t n;
    bool cigar_is_text;            // cig[i].cigar (and split->cig[s].cigar) is the NUL-terminated run-length text already (lrm_map_options.cigar_text)
    bool revcomp_here;             // the batch ran with keep_reads: reverse-strand reads are reverse-complemented while they are printed
    const lrm_split_out *split;    // null or no segment: no supplementary lines
    const lrm_mapq *mq;            // null: column 5 is 255, no v1:i / v2:i
    // the difference events of the batch (docs/GACT_SPEC.md, "Difference events and MD:Z"); events null: no NM:i / MD:Z
    const lrm_aln_summary *sum; const uint64_t *diff_off; const uint32_t *diff_cnt; const uint32_t *events;
    const lrm_secondary_out *sec;  // null or no candidate: no FLAG 256 lines (docs/GACT_SPEC.md, "Secondary alignments")
};

// ---- the writers every field goes through (sam_text.cpp, paf_text.cpp) ----
static inline int put_uint(char *dst, uint64_t v) {           // decimal text of v, returns its length (<= 20)
    char tmp[24];
    int n = 0;
    do { tmp[n++] = (char) ('0' + v % 10); v /= 10; } while (v);
    for (int i = 0; i < n; ++i) dst[i] = tmp[n - 1 - i];
    return n;
}
static inline void put_num(std::string &s, uint64_t v) { char num[24]; s.append(num, (size_t) put_uint(num, v)); }
static inline void put_int(std::string &s, int64_t v) { if (v < 0) { s += '-'; put_num(s, (uint64_t) -v); } else put_num(s, (uint64_t) v); }
// MD:Z text of one read from its events and its n_eq, appended to s (lrm_md_format)
void sam_append_md(std::string &s, const uint32_t *events, uint64_t count, uint32_t n_eq);
// the CIGAR column of one alignment as lrm_parse_cigar prints it: the text as it is, or the run-length text of the op bytes
void sam_append_cigar(std::string &s, const lrm_cigar &c, bool is_text);

// Up to nt threads format a contiguous range of reads each into a buffer of their own: the text is parts[0] + parts[1] + ...
void sam_format_parts(const SamBatch &b, int nt, std::vector<std::string> &parts);
// at[k]: where parts[k] begins in a text that begins at `base`; at[parts.size()]: where the text ends
std::vector<uint64_t> sam_part_offsets(const std::vector<std::string> &parts, uint64_t base);
