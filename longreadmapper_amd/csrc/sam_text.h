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
};

// Up to nt threads format a contiguous range of reads each into a buffer of their own: the text is parts[0] + parts[1] + ...
void sam_format_parts(const SamBatch &b, int nt, std::vector<std::string> &parts);
// at[k]: where parts[k] begins in a text that begins at `base`; at[parts.size()]: where the text ends
std::vector<uint64_t> sam_part_offsets(const std::vector<std::string> &parts, uint64_t base);
