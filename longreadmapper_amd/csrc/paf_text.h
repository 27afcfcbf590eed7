// paf_text.h -- what the accaln flow (accaln_flow.cpp) takes from the PAF formatter (paf_text.cpp): a batch as the
// formatter reads it and the parallel formatting of it.  The parts are placed like SAM text (sam_part_offsets, sam_text.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/lrm_io_host.h"

// One batch of results on its way into PAF text (docs/GACT_SPEC.md, "Alignment summary and PAF"); read-only.
struct PafBatch {
    const lrm_read_batch *reads;
    const lrm_mta_entry *mta; int mta_len;
    const lrm_cigar *cig; const int *score; const lrm_seq_meta *meta; const int *meta_r;
    uint64_t n;
    bool cigar_is_text;            // cig[i].cigar is the NUL-terminated run-length text already (lrm_map_options.cigar_text)
    const lrm_aln_summary *sum;    // the records of the batch: every number of a line but the names and lengths comes from them
    const lrm_mapq *mq;            // null: column 12 is 255, no v1:i / v2:i
};

// Up to nt threads format a contiguous range of reads each into a buffer of their own: the text is parts[0] + parts[1] + ...
void paf_format_parts(const PafBatch &b, int nt, std::vector<std::string> &parts);
