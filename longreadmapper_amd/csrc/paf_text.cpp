// paf_text.cpp -- PAF records from the alignment summary records (lrm_paf_format, include/lrm_io_host.h; docs/GACT_SPEC.md,
// "Alignment summary and PAF").  Host-side C++; every field goes through the writers of sam_text.h.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "paf_text.h"
#include "sam_text.h"
#include "lrm_internal.h"

// PAF lines of reads [lo, hi) written to s: one per mapped read, nothing for an unmapped one
static void paf_format_range(const PafBatch &b, uint64_t lo, uint64_t hi, std::string &s) {
    const lrm_read_batch *reads = b.reads;
    uint64_t est = 0;
    for (uint64_t i = lo; i < hi; ++i) est += 2ull * (b.cig[i].n_cigar_op > 0 ? (uint64_t) b.cig[i].n_cigar_op : 0) + 256;
    s.clear();
    s.reserve(est);
    for (uint64_t i = lo; i < hi; ++i) {
        if (b.meta_r[i] == 0 || b.score[i] == -1) continue;           // alnmain.c:466-469: unmapped
        const lrm_seq_meta &m = b.meta[i];
        const lrm_aln_summary &a = b.sum[i];
        const uint64_t qlen = reads->lens[i], cl = a.clip_left, cr = a.clip_right;
        const bool rev = m.strand == 1;                               // the ops run along the reverse complement of the read
        const uint64_t span = (uint64_t) a.n_eq + a.n_x + a.n_del, block = span + a.n_ins;
        const bool named = m.seq_id >= 0 && m.seq_id < b.mta_len;
        s += reads->names[i];
        s += '\t'; put_num(s, qlen);
        s += '\t'; put_num(s, rev ? cr : cl);
        s += '\t'; put_num(s, qlen - (rev ? cl : cr));
        s += '\t'; s += rev ? '-' : '+';
        s += '\t';
        if (named) s.append(b.mta[m.seq_id].name, b.mta[m.seq_id].name_len); else s += '*';
        s += '\t'; put_num(s, named ? (uint64_t) b.mta[m.seq_id].seq_len : 0ull);
        s += '\t'; put_num(s, m.off);
        s += '\t'; put_num(s, m.off + span);
        s += '\t'; put_num(s, a.n_eq);
        s += '\t'; put_num(s, block);
        s += '\t'; put_num(s, b.mq ? b.mq[i].mapq : 255u);
        s += "\tNM:i:"; put_num(s, (uint64_t) a.n_x + a.n_ins + a.n_del);
        s += "\tED:i:"; put_int(s, b.score[i]);
        s += "\ttp:A:P";
        // gap-compressed divergence: every gap counts once, however long
        const uint64_t ev = (uint64_t) a.n_x + a.ins_runs + a.del_runs, den = ev + a.n_eq;
        char de[32];
        snprintf(de, sizeof(de), "%.4f", den ? (double) ev / (double) den : 0.0);
        s += "\tde:f:"; s += de;
        s += "\tcg:Z:"; sam_append_cigar(s, b.cig[i], b.cigar_is_text);
        if (b.mq) {
            s += "\tv1:i:"; put_num(s, b.mq[i].n1);
            s += "\tv2:i:"; put_num(s, b.mq[i].n2);
        }
        s += '\n';
    }
}

void paf_format_parts(const PafBatch &b, int nt, std::vector<std::string> &parts) {
    if (nt < 1) nt = 1;
    if ((uint64_t) nt > b.n) nt = b.n ? (int) b.n : 1;
    parts.resize((size_t) nt);
    const uint64_t n = b.n, T = (uint64_t) nt;
#pragma omp parallel for schedule(static, 1) num_threads(nt)
    for (int t = 0; t < nt; ++t) paf_format_range(b, n * (uint64_t) t / T, n * (uint64_t) (t + 1) / T, parts[(size_t) t]);
}

extern "C" char *lrm_paf_format(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                                const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                                const lrm_aln_summary *sum, const lrm_mapq *mq, uint64_t *len_out) {
    if (!sum || (n && (!reads || !cig || !score || !meta || !meta_r))) { lrm_set_error("null argument"); return nullptr; }
    const PafBatch b = {reads, mta, mta_len, cig, score, meta, meta_r, n, cigar_is_text != 0, sum, mq};
    std::vector<std::string> parts;
    paf_format_parts(b, lrm_host_threads(), parts);
    const std::vector<uint64_t> at = sam_part_offsets(parts, 0);
    const uint64_t total = at[parts.size()];
    char *out = (char *) malloc(total + 1);
    if (!out) { lrm_set_error("out of memory"); return nullptr; }
#pragma omp parallel for schedule(static, 1) num_threads((int) parts.size())
    for (size_t k = 0; k < parts.size(); ++k) memcpy(out + at[k], parts[k].data(), parts[k].size());
    out[total] = 0;
    if (len_out) *len_out = total;
    return out;
}
