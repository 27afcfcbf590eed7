// sam_text.cpp -- run-length CIGAR text, SAM header, SAM records and the split reads' supplementary records with SA:Z
// (lrm_parse_cigar, lrm_sam_header, lrm_sam_format*, include/lrm_io_host.h).  Host-side C++.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "sam_text.h"
#include "lrm_internal.h"

// (the writers every field goes through -- put_uint, put_num, put_int -- are in sam_text.h: the PAF formatter uses them too)

// class of an op byte for the run-length CIGAR: '=' and 'X' print as M, every other byte as itself
static inline char op_class(uint8_t o) { return (o == '=' || o == 'X') ? 'M' : (char) o; }

// run-length text of n_ops op bytes written at dst; returns its length.  One pass, one compare per column, the decimal
// digits of a run written back to front into place.
// CHECKED == false: room for 11 bytes per run must be there (callers reserve 2 * n_ops + 16 -- a run of one column prints
//   as two bytes, a longer one as fewer per column); nothing is checked per run, this is the formatter's hot loop.
// CHECKED == true: dst has `room` bytes; -1 as soon as fewer than 13 (<= 10 digits + op + NUL) are left before a run.
// (always_inline, here and on put_cigar: left to itself the compiler keeps this loop out of the formatter's, which costs
//  lrm_sam_format 6-9 % of its rate)
template <bool CHECKED>
__attribute__((always_inline)) static inline int64_t rle_write(const uint8_t *ops, int n_ops, char *dst, int64_t room = 0) {
    size_t w = 0;
    int i = 0;
    while (i < n_ops) {
        const char cls = op_class(ops[i]);
        int j = i + 1;
        if (cls == 'M') { while (j < n_ops && (ops[j] == '=' || ops[j] == 'X')) ++j; }
        else { const uint8_t o = ops[i]; while (j < n_ops && ops[j] == o) ++j; }
        if (CHECKED && room - (int64_t) w < 13) return -1;
        uint32_t run = (uint32_t) (j - i);
        if (run < 10) { dst[w++] = (char) ('0' + run); }
        else if (run < 100) { dst[w++] = (char) ('0' + run / 10); dst[w++] = (char) ('0' + run % 10); }
        else w += (size_t) put_uint(dst + w, run);
        dst[w++] = cls;
        i = j;
    }
    return (int64_t) w;
}

extern "C" int lrm_parse_cigar(const uint8_t *ops, int n_ops, char *buf, int buflen) {
    if (n_ops <= 0) {
        if (buflen < 2) return -1;
        buf[0] = '*'; buf[1] = 0;
        return 1;
    }
    // room for the worst case: no checks inside the loop
    const int64_t w = buflen >= 2 * n_ops + 16 ? rle_write<false>(ops, n_ops, buf) : rle_write<true>(ops, n_ops, buf, buflen);
    if (w < 0) return -1;
    buf[w] = 0;
    return (int) w;
}

// the CIGAR column of one alignment: the text as it is, or the op bytes through rle_write; "*" without an alignment
__attribute__((always_inline)) static inline void put_cigar(std::string &s, const lrm_cigar &c, bool is_text) {
    if (c.n_cigar_op <= 0) s += '*';
    else if (is_text) s.append((const char *) c.cigar);
    else {
        const size_t at = s.size();
        s.resize(at + 2 * (size_t) c.n_cigar_op + 16);                  // alnmain.c:497: a 2 * qlen buffer there
        s.resize(at + (size_t) rle_write<false>(c.cigar, c.n_cigar_op, &s[at]));
    }
}
void sam_append_cigar(std::string &s, const lrm_cigar &c, bool is_text) { put_cigar(s, c, is_text); }

// MD:Z from a read's difference events (docs/GACT_SPEC.md, "Difference events and MD:Z"): before an 'X' and before the first
// 'D' of a run the '=' columns since the previous such event ("0" included), '^' in front of a run of deleted bases, the
// base; a 'D' that continues a run prints its base alone; at the end the '=' columns that are left
void sam_append_md(std::string &s, const uint32_t *events, uint64_t count, uint32_t n_eq) {
    uint32_t prev = 0;
    for (uint64_t k = 0; k < count; ++k) {
        const uint32_t w = events[k], kind = LRM_DIFF_KIND(w), e = LRM_DIFF_EQ_BEFORE(w);
        if (kind != LRM_DIFF_D_MORE) {
            put_num(s, e - prev);
            if (kind == LRM_DIFF_D_OPEN) s += '^';
            prev = e;
        }
        s += (char) LRM_DIFF_BASE(w);
    }
    put_num(s, n_eq - prev);
}
extern "C" int lrm_md_format(const uint32_t *events, uint64_t count, uint32_t n_eq, char *buf, int buflen) {
    if (!buf || buflen < 1 || (count && !events)) return -1;
    std::string s;
    sam_append_md(s, events, count, n_eq);
    if (s.size() + 1 > (size_t) buflen) return -1;
    memcpy(buf, s.data(), s.size());
    buf[s.size()] = 0;
    return (int) s.size();
}
// the name of reference sequence seq_id; "*" if there is none
static inline void put_rname(std::string &s, const SamBatch &b, int seq_id) {
    if (seq_id >= 0 && seq_id < b.mta_len) s.append(b.mta[seq_id].name, b.mta[seq_id].name_len); else s += '*';
}

extern "C" void lrm_free(void *p) { free(p); }

static char *dup_out(const std::string &s, uint64_t *len_out) {
    char *p = (char *) malloc(s.size() + 1);
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    if (len_out) *len_out = s.size();
    return p;
}

extern "C" char *lrm_sam_header(const lrm_mta_entry *mta, int mta_len, long rg_id, uint64_t *len_out) {
    std::string s;
    char line[1200];
    for (int i = 0; i < mta_len; ++i) {                       // alnmain.c:66-72
        snprintf(line, sizeof(line), "@SQ\tSN:%.*s\tLN:%ld\n", (int) (mta[i].name_len < 1023 ? mta[i].name_len : 1023),
                 mta[i].name ? mta[i].name : "", (long) mta[i].seq_len);
        s += line;
    }
    snprintf(line, sizeof(line), "@RG\tID:%s%ld\tSM:SM_data\n", "accaln", rg_id);   // alnmain.c:73
    s += line;
    s += "@PG\tID:accaln\tPN:accaln\n";                                                // alnmain.c:74
    return dup_out(s, len_out);
}

// ---- split reads: supplementary records and SA:Z (docs/GACT_SPEC.md, "Split reads") ----------------------------------------
struct AlnShape { uint64_t q, t, sl, sr; };        // aligned query bases, target span, 'S' columns at the start / at the end
static AlnShape aln_shape(const lrm_cigar &c, bool is_text) {
    AlnShape a = {0, 0, 0, 0};
    if (c.n_cigar_op <= 0 || !c.cigar) return a;
    bool seen = false;                             // a column other than 'S' has been seen: an 'S' run from here on is the right one
    auto add = [&](char op, uint64_t run) {
        if (op == 'S') { (seen ? a.sr : a.sl) += run; return; }
        seen = true;
        if (op == 'M' || op == '=' || op == 'X') { a.q += run; a.t += run; }
        else if (op == 'I') a.q += run;
        else if (op == 'D') a.t += run;
    };
    if (is_text) {
        uint64_t run = 0;
        for (const char *p = (const char *) c.cigar; *p; ++p) {
            if (*p >= '0' && *p <= '9') run = run * 10 + (uint64_t) (*p - '0');
            else { add(*p, run); run = 0; }
        }
    } else {
        for (int i = 0; i < c.n_cigar_op; ++i) add((char) c.cigar[i], 1);
    }
    return a;
}
// one SA:Z entry: rname,pos,strand,<c5>S<q>M<d>D|I<c3>S,<mapq>,ED;  (mapq: 255 without a record -- the split segments have none)
static void sa_entry(std::string &s, const SamBatch &b, const lrm_seq_meta &m, bool rev, uint64_t c5, const AlnShape &a, uint64_t c3,
                     int ed, unsigned mapq = 255) {
    put_rname(s, b, m.seq_id);
    s += ','; put_num(s, m.off + 1); s += ','; s += rev ? '-' : '+'; s += ',';
    if (c5) { put_num(s, c5); s += 'S'; }
    put_num(s, a.q); s += 'M';
    if (a.t > a.q) { put_num(s, a.t - a.q); s += 'D'; }
    if (a.q > a.t) { put_num(s, a.q - a.t); s += 'I'; }
    if (c3) { put_num(s, c3); s += 'S'; }
    s += ','; put_num(s, mapq); s += ','; put_int(s, ed); s += ';';
}
struct SplitCtx {                                  // a batch's segments, and where those of read i begin (first[i] .. first[i + 1])
    const lrm_split_out *sp;
    std::vector<uint64_t> first;
    SplitCtx(const lrm_split_out *o, uint64_t n) : sp(o), first((size_t) n + 1, 0) {
        const uint64_t k = o ? o->n_seg : 0;
        for (uint64_t s = 0; s < k; ++s) if (o->seg[s].read < n) ++first[(size_t) o->seg[s].read + 1];
        for (uint64_t i = 0; i < n; ++i) first[(size_t) i + 1] += first[(size_t) i];
    }
};
// the hard-clipped bases either side of segment g of a read of n bases, in the orientation of the segment's record
static inline void seg_hard(const lrm_segment &g, uint32_t n, bool ss, uint64_t *hl, uint64_t *hr) {
    const uint64_t a = g.start, b = (uint64_t) n - g.start - g.len;
    *hl = ss ? b : a; *hr = ss ? a : b;
}
// SA:Z of read i's primary (tail of its line) and its supplementary lines
static void sam_split_lines(const SamBatch &b, uint64_t i, const SplitCtx &sx, std::string &s) {
    const lrm_split_out &o = *sx.sp;
    uint64_t rep[2];
    int nrep = 0;
    for (uint64_t k = sx.first[(size_t) i]; k < sx.first[(size_t) i + 1] && nrep < 2; ++k) if (o.seg[k].flags & LRM_SEG_ALIGNED) rep[nrep++] = k;
    if (!nrep) { s += '\n'; return; }
    const uint32_t n = b.reads->lens[i];
    const bool ps = b.meta[i].strand == 1;
    const AlnShape pa = aln_shape(b.cig[i], b.cigar_is_text);
    AlnShape sa[2];
    uint64_t hl[2], hr[2];
    bool ss[2];
    for (int k = 0; k < nrep; ++k) {
        sa[k] = aln_shape(o.cig[rep[k]], b.cigar_is_text);
        ss[k] = o.meta[rep[k]].strand == 1;
        seg_hard(o.seg[rep[k]], n, ss[k], &hl[k], &hr[k]);
    }
    auto seg_entry = [&](int k) { sa_entry(s, b, o.meta[rep[k]], ps != ss[k], hl[k] + sa[k].sl, sa[k], sa[k].sr + hr[k], o.score[rep[k]]); };
    s += "\tSA:Z:";
    for (int k = 0; k < nrep; ++k) seg_entry(k);
    s += '\n';
    for (int k = 0; k < nrep; ++k) {
        const uint64_t x = rep[k];
        const lrm_segment &g = o.seg[x];
        const bool rev = ps != ss[k];
        s += b.reads->names[i];
        s += '\t'; put_num(s, 2048u + (rev ? 16u : 0u));
        s += '\t'; put_rname(s, b, o.meta[x].seq_id);
        s += '\t'; put_num(s, o.meta[x].off + 1);
        s += "\t255\t";
        if (hl[k]) { put_num(s, hl[k]); s += 'H'; }
        put_cigar(s, o.cig[x], b.cigar_is_text);
        if (hr[k]) { put_num(s, hr[k]); s += 'H'; }
        s += "\t*\t0\t0\t";
        s.append(o.rows + x * o.row_stride, g.len);                  // the segment row as the extension left it
        s += '\t';
        if (b.reads->quals[i]) {                                     // the read's qualities run as it was sequenced
            const uint64_t q0 = ps ? (uint64_t) n - g.start - g.len : g.start;
            const char *q = b.reads->quals[i] + q0;
            if (rev) { const size_t at = s.size(); s.resize(at + g.len); for (uint32_t c = 0; c < g.len; ++c) s[at + c] = q[g.len - 1 - c]; }
            else s.append(q, g.len);
        } else s += '*';
        s += "\tED:I:"; put_int(s, o.score[x]);
        s += "\tSA:Z:";
        sa_entry(s, b, b.meta[i], ps, pa.sl, pa, pa.sr, b.score[i], b.mq ? b.mq[i].mapq : 255u);
        if (nrep == 2) seg_entry(1 - k);
        s += '\n';
    }
}

// SAM lines of reads [lo, hi) written to s (alnmain.c:500-525 field for field).  No snprintf on the hot path: a 10 kbp
// ONT read has ~2000 CIGAR runs.  sx: the batch's split table, if it has segments.
// ---- secondary alignments (docs/GACT_SPEC.md, "Secondary alignments") -------------------------------------------------------
// the FLAG 256 line of candidate c of read i, if it is reported: its own locus and run-length CIGAR (soft clips as S), MAPQ 0,
// no SEQ and no QUAL (the primary line has them), tp:A:S
static void sam_secondary_line(const SamBatch &b, uint64_t i, uint64_t c, std::string &s) {
    const lrm_secondary_out &o = *b.sec;
    if (!(o.table[c].flags & LRM_SEC_ALIGNED)) return;
    s += b.reads->names[i];
    s += '\t'; put_num(s, 256u + (o.meta[c].strand == 1 ? 16u : 0u));
    s += '\t'; put_rname(s, b, o.meta[c].seq_id);
    s += '\t'; put_num(s, o.meta[c].off + 1);
    s += "\t0\t";
    put_cigar(s, o.cig[c], b.cigar_is_text);
    s += "\t*\t0\t0\t*\t*\tED:I:"; put_int(s, o.score[c]);
    s += "\ttp:A:S\n";
}
// where read i's candidate is in the table (reads ascending, one per read): sec_at[i], or UINT64_MAX
static std::vector<uint64_t> sec_index(const lrm_secondary_out *o, uint64_t n) {
    std::vector<uint64_t> at;
    if (!o || !o->n_sec) return at;
    at.assign((size_t) n, UINT64_MAX);
    for (uint64_t c = 0; c < o->n_sec; ++c) if (o->table[c].read < n) at[o->table[c].read] = c;
    return at;
}

static void sam_format_range(const SamBatch &b, uint64_t lo, uint64_t hi, std::string &s, const SplitCtx *sx,
                             const std::vector<uint64_t> &sec_at) {
    const lrm_read_batch *reads = b.reads;
    const lrm_mapq *mq = b.mq;
    uint64_t est = 0;
    for (uint64_t i = lo; i < hi; ++i) est += 2ull * reads->lens[i] + 2ull * (b.cig[i].n_cigar_op > 0 ? (uint64_t) b.cig[i].n_cigar_op : 0) + 160;
    s.clear();
    s.reserve(est);
    for (uint64_t i = lo; i < hi; ++i) {
        const uint32_t len = reads->lens[i];
        const lrm_seq_meta &m = b.meta[i];
        const bool unmapped = b.meta_r[i] == 0 || b.score[i] == -1;  // alnmain.c:466-469
        unsigned flag = 0, mapq = 255;
        if (unmapped) { flag += 0x4; mapq = 0; }
        else if (m.strand == 1) flag += 16;
        if (mq && !unmapped) mapq = mq[i].mapq;                      // mapping quality: the record's value instead of 255
        s += reads->names[i];
        s += '\t'; put_num(s, flag);
        s += '\t'; put_rname(s, b, unmapped ? -1 : m.seq_id);
        s += '\t'; put_num(s, unmapped ? 0ull : (uint64_t) (m.off + 1));       // %ld of a non-negative value
        s += '\t'; put_num(s, mapq);
        s += '\t';
        if (unmapped) s += '*'; else put_cigar(s, b.cig[i], b.cigar_is_text);
        s += "\t*\t0\t0\t";                                            // r_name "*", 0L, 0
        if (b.revcomp_here && b.meta_r[i] != 0 && m.strand == 1) {
            // lrm_map_options.keep_reads: the batch came back as it went -- _rev_comp_in_place (alnmain.c:27-60) while copying
            const size_t at = s.size();
            s.resize(at + len);
            const char *src = reads->seqs + i * reads->stride;
            char *dst = &s[at];
            for (uint32_t x = 0; x < len; ++x) dst[x] = lrm_comp_table.t[(uint8_t) src[len - 1 - x]];
        } else {
            s.append(reads->seqs + i * reads->stride, len);           // the (possibly rev-comped) read
        }
        s += '\t';
        if (reads->quals[i]) s.append(reads->quals[i], len); else s += '*';
        s += "\tED:I:"; put_int(s, b.score[i]);
        if (mq) {                                                      // the two vote counts behind the MAPQ
            s += "\tv1:i:"; put_num(s, mq[i].n1);
            s += "\tv2:i:"; put_num(s, mq[i].n2);
        }
        if (b.events && !unmapped && b.cig[i].n_cigar_op > 0 && b.diff_off[i] != UINT64_MAX) {   // (UINT64_MAX: the read's events found no room)
            const lrm_aln_summary &a = b.sum[i];
            s += "\tNM:i:"; put_num(s, (uint64_t) a.n_x + a.n_ins + a.n_del);
            s += "\tMD:Z:"; sam_append_md(s, b.events + b.diff_off[i], b.diff_cnt[i], a.n_eq);
        }
        if (sx && !unmapped) sam_split_lines(b, i, *sx, s);
        else s += '\n';
        if (!sec_at.empty() && sec_at[(size_t) i] != UINT64_MAX) sam_secondary_line(b, i, sec_at[(size_t) i], s);
    }
}

void sam_format_parts(const SamBatch &b, int nt, std::vector<std::string> &parts) {
    if (nt < 1) nt = 1;
    if ((uint64_t) nt > b.n) nt = b.n ? (int) b.n : 1;
    parts.resize((size_t) nt);
    const bool segs = b.split && b.split->n_seg;
    const SplitCtx sx(segs ? b.split : nullptr, segs ? b.n : 0);
    const std::vector<uint64_t> sec_at = sec_index(b.sec, b.n);
    const uint64_t n = b.n, T = (uint64_t) nt;
#pragma omp parallel for schedule(static, 1) num_threads(nt)
    for (int t = 0; t < nt; ++t) sam_format_range(b, n * (uint64_t) t / T, n * (uint64_t) (t + 1) / T, parts[(size_t) t], segs ? &sx : nullptr, sec_at);
}

std::vector<uint64_t> sam_part_offsets(const std::vector<std::string> &parts, uint64_t base) {
    std::vector<uint64_t> at(parts.size() + 1, base);
    for (size_t k = 0; k < parts.size(); ++k) at[k + 1] = at[k] + parts[k].size();
    return at;
}

extern "C" char *lrm_sam_format_secondary(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                                          const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                                          int revcomp_here, const lrm_split_out *split, const lrm_mapq *mq, const lrm_aln_summary *sum,
                                          const uint64_t *diff_off, const uint32_t *diff_cnt, const uint32_t *events,
                                          const lrm_secondary_out *sec, uint64_t *len_out) {
    if (events && (!sum || !diff_off || !diff_cnt)) { lrm_set_error("lrm_sam_format_md: events without summary records, offsets or counts"); return nullptr; }
    if (sec && sec->n_sec && (!sec->table || !sec->cig || !sec->score || !sec->meta)) { lrm_set_error("lrm_sam_format_secondary: null array in lrm_secondary_out"); return nullptr; }
    const SamBatch b = {reads, mta, mta_len, cig, score, meta, meta_r, n, cigar_is_text != 0, revcomp_here != 0, split, mq,
                        sum, diff_off, diff_cnt, events, sec};
    std::vector<std::string> parts;
    sam_format_parts(b, lrm_host_threads(), parts);
    const std::vector<uint64_t> at = sam_part_offsets(parts, 0);
    const uint64_t total = at[parts.size()];
    char *out = (char *) malloc(total + 1);
    if (!out) return nullptr;
#pragma omp parallel for schedule(static, 1) num_threads((int) parts.size())
    for (size_t k = 0; k < parts.size(); ++k) memcpy(out + at[k], parts[k].data(), parts[k].size());
    out[total] = 0;
    if (len_out) *len_out = total;
    return out;
}
extern "C" char *lrm_sam_format_md(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                                   const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                                   int revcomp_here, const lrm_split_out *split, const lrm_mapq *mq, const lrm_aln_summary *sum,
                                   const uint64_t *diff_off, const uint32_t *diff_cnt, const uint32_t *events, uint64_t *len_out) {
    return lrm_sam_format_secondary(reads, mta, mta_len, cig, score, meta, meta_r, n, cigar_is_text, revcomp_here, split, mq, sum, diff_off,
                                    diff_cnt, events, nullptr, len_out);
}
extern "C" char *lrm_sam_format_mapq(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                                     const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                                     int revcomp_here, const lrm_split_out *split, const lrm_mapq *mq, uint64_t *len_out) {
    return lrm_sam_format_md(reads, mta, mta_len, cig, score, meta, meta_r, n, cigar_is_text, revcomp_here, split, mq, nullptr, nullptr,
                             nullptr, nullptr, len_out);
}
extern "C" char *lrm_sam_format_split(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len, const lrm_cigar *cig,
                                      const int *score, const lrm_seq_meta *meta, const int *meta_r, uint64_t n, int cigar_is_text,
                                      int revcomp_here, const lrm_split_out *split, uint64_t *len_out) {
    return lrm_sam_format_mapq(reads, mta, mta_len, cig, score, meta, meta_r, n, cigar_is_text, revcomp_here, split, nullptr, len_out);
}
extern "C" char *lrm_sam_format(const lrm_read_batch *reads, const lrm_mta_entry *mta, int mta_len,
                                const lrm_cigar *cig, const int *score, const lrm_seq_meta *meta,
                                const int *meta_r, uint64_t n, uint64_t *len_out) {
    return lrm_sam_format_mapq(reads, mta, mta_len, cig, score, meta, meta_r, n, 0, 0, nullptr, nullptr, len_out);
}
