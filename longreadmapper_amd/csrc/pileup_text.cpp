// pileup_text.cpp -- pileup records as text (lrm_pileup_format, lrm_pileup_sites_format[_ins], lrm_pileup_variants_format_vcf, lrm_vcf_header, include/lrm_accel.h; docs/GACT_SPEC.md, "Pileup", "Pileup calls", "Pileup variants and VCF").  Host-side
// C++; the numbers go through put_uint of sam_text.h.
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include "pileup_text.h"
#include "sam_text.h"
#include "lrm_internal.h"

int pileup_put_line(char *dst, const char *name, uint64_t name_len, uint64_t pos1, char base, const lrm_pileup_col &c) {
    char *p = dst;
    memcpy(p, name, name_len);
    p += name_len;
    *p++ = '\t';
    p += put_uint(p, pos1);
    *p++ = '\t';
    *p++ = base;
    const uint32_t other = c.depth - c.n_eq - c.x_a - c.x_c - c.x_g - c.x_t - c.n_del;
    for (const uint32_t v : {c.depth, c.n_eq, c.x_a, c.x_c, c.x_g, c.x_t, other, c.n_del, c.n_ins}) {
        *p++ = '\t';
        p += put_uint(p, v);
    }
    *p++ = '\n';
    return (int) (p - dst);
}

extern "C" int64_t lrm_pileup_format(const lrm_mta_entry *mta, int mta_len, int seq, uint64_t seq_pos, uint64_t count, const char *content,
                                     const lrm_pileup_col *cols, char *buf, int64_t buflen) {
    if (!mta || !buf || buflen <= 0 || (count && (!content || !cols))) { lrm_set_error("null argument"); return -1; }
    if (seq < 0 || seq >= mta_len) { lrm_set_error("pileup text: sequence %d of %d", seq, mta_len); return -1; }
    const lrm_mta_entry &m = mta[seq];
    if (seq_pos > m.seq_len || count > m.seq_len - seq_pos) { lrm_set_error("pileup text: positions [%llu, +%llu) outside a sequence of %llu bases", (unsigned long long) seq_pos, (unsigned long long) count, (unsigned long long) m.seq_len); return -1; }
    const char *name = m.name ? m.name : "";
    const uint64_t name_len = m.name ? m.name_len : 0, room = pileup_line_room(name_len);
    int64_t at = 0;
    for (uint64_t k = 0; k < count; ++k) {
        if ((uint64_t) (buflen - at) < room + 1) { lrm_set_error("pileup text: buffer of %lld bytes too small", (long long) buflen); return -2; }   // (+1: the NUL)
        at += pileup_put_line(buf + at, name, name_len, seq_pos + k + 1, content[m.offset + seq_pos + k], cols[k]);
    }
    buf[at] = '\0';
    return at;
}

int pileup_put_site_line(char *dst, const char *name, uint64_t name_len, uint64_t pos1, const lrm_pileup_site &s) {
    char *p = dst;
    memcpy(p, name, name_len);
    p += name_len;
    *p++ = '\t';
    p += put_uint(p, pos1);
    *p++ = '\t';
    *p++ = (char) s.ref;
    *p++ = '\t';
    *p++ = (char) s.alt;
    *p++ = '\t';
    if (s.kinds & LRM_CALL_SNV) *p++ = 'S';
    if (s.kinds & LRM_CALL_DEL) *p++ = 'D';
    if (s.kinds & LRM_CALL_INS) *p++ = 'I';
    for (const uint32_t v : {s.depth, s.n_ref, s.n_alt, s.n_del, s.n_ins}) {
        *p++ = '\t';
        p += put_uint(p, v);
    }
    *p++ = '\t';
    *p++ = (char) s.cons;
    *p++ = '\n';
    return (int) (p - dst);
}

// alleles (may be null): one more column per line, the inserted bases of the site or '.' (lrm_pileup_sites_format_ins)
extern "C" int64_t lrm_pileup_sites_format_ins(const lrm_mta_entry *mta, int mta_len, const lrm_pileup_site *sites,
                                               const lrm_pileup_ins_allele *alleles, uint64_t count, char *buf, int64_t buflen) {
    if (!mta || mta_len <= 0 || !buf || buflen <= 0 || (count && !sites)) { lrm_set_error("null argument"); return -1; }
    int64_t at = 0;
    int seq = 0;                                                       // sites come in ascending position: start at the last sequence found
    for (uint64_t k = 0; k < count; ++k) {
        const uint64_t pos = sites[k].pos;
        int tried = 0;
        while (tried < mta_len && !(pos >= mta[seq].offset && pos - mta[seq].offset < mta[seq].seq_len)) {
            seq = seq + 1 < mta_len ? seq + 1 : 0;
            ++tried;
        }
        if (tried == mta_len) { lrm_set_error("pileup sites text: position %llu lies in no sequence", (unsigned long long) pos); return -1; }
        const lrm_mta_entry &m = mta[seq];
        const uint64_t name_len = m.name ? m.name_len : 0;
        if ((uint64_t) (buflen - at) < pileup_site_line_room(name_len) + 1 + (alleles ? 1u + LRM_PILEUP_INS_COLS_MAX : 0u)) { lrm_set_error("pileup sites text: buffer of %lld bytes too small", (long long) buflen); return -2; }   // (+1: the NUL)
        at += pileup_put_site_line(buf + at, m.name ? m.name : "", name_len, pos - m.offset + 1, sites[k]);
        if (alleles) {                                                 // the line's '\n' moves behind the new column
            const uint32_t len = alleles[k].len < LRM_PILEUP_INS_COLS_MAX ? alleles[k].len : LRM_PILEUP_INS_COLS_MAX;
            buf[at - 1] = '\t';
            if (len == 0) buf[at++] = '.';
            memcpy(buf + at, alleles[k].bases, len);
            at += len;
            buf[at++] = '\n';
        }
    }
    buf[at] = '\0';
    return at;
}
extern "C" int64_t lrm_pileup_sites_format(const lrm_mta_entry *mta, int mta_len, const lrm_pileup_site *sites, uint64_t count, char *buf,
                                           int64_t buflen) {
    return lrm_pileup_sites_format_ins(mta, mta_len, sites, nullptr, count, buf, buflen);
}

// ---- VCF (docs/GACT_SPEC.md, "Pileup variants and VCF") ----
static inline char vcf_upper(uint8_t b) { return (char) (b >= 'a' && b <= 'z' ? b - 32 : b); }
static int64_t vcf_small(int64_t buflen) { lrm_set_error("VCF text: buffer of %lld bytes too small", (long long) buflen); return -2; }

extern "C" int64_t lrm_vcf_header(const lrm_mta_entry *mta, int mta_len, const char *sample, char *buf, int64_t buflen) {
    if (!mta || mta_len <= 0 || !buf || buflen <= 0) { lrm_set_error("null argument"); return -1; }
    int64_t at = 0;
    auto put = [&](const char *t, uint64_t n) {                        // false: no room for n bytes and the NUL
        if ((uint64_t) (buflen - at) < n + 1) return false;
        memcpy(buf + at, t, n);
        at += (int64_t) n;
        return true;
    };
    auto puts_ = [&](const char *t) { return put(t, strlen(t)); };
    if (!puts_("##fileformat=VCFv4.2\n")) return vcf_small(buflen);
    for (int k = 0; k < mta_len; ++k) {
        char num[24];
        const int d = put_uint(num, mta[k].seq_len);
        if (!puts_("##contig=<ID=") || !put(mta[k].name ? mta[k].name : "", mta[k].name ? mta[k].name_len : 0) || !puts_(",length=") || !put(num, (uint64_t) d) ||
            !puts_(">\n")) return vcf_small(buflen);
    }
    if (!puts_("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Alignments that cover the position\">\n"
               "##INFO=<ID=INSFULL,Number=0,Type=Flag,Description=\"The inserted bases fill every insertion column: the insertion may be longer\">\n"
               "##ALT=<ID=INS,Description=\"Insertion without a majority base in its first column\">\n"
               "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
               "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Alignments that show the text, alignments that show the alternative\">\n"
               "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t") ||
        !puts_(sample && *sample ? sample : "SAMPLE") || !puts_("\n")) return vcf_small(buflen);
    buf[at] = '\0';
    return at;
}

extern "C" int64_t lrm_pileup_variants_format_vcf(const lrm_mta_entry *mta, int mta_len, const char *content, const lrm_pileup_variant *vars,
                                                  uint64_t count, char *buf, int64_t buflen) {
    if (!mta || mta_len <= 0 || !buf || buflen <= 0 || (count && (!vars || !content))) { lrm_set_error("null argument"); return -1; }
    int64_t at = 0;
    int seq = 0;                                                       // records come in ascending position: start at the last sequence found
    for (uint64_t k = 0; k < count; ++k) {
        const lrm_pileup_variant &v = vars[k];
        const uint64_t pos = v.pos;
        int tried = 0;
        while (tried < mta_len && !(pos >= mta[seq].offset && pos - mta[seq].offset < mta[seq].seq_len)) {
            seq = seq + 1 < mta_len ? seq + 1 : 0;
            ++tried;
        }
        if (tried == mta_len) { lrm_set_error("VCF text: position %llu lies in no sequence", (unsigned long long) pos); return -1; }
        const lrm_mta_entry &m = mta[seq];
        const uint64_t name_len = m.name ? m.name_len : 0, off = pos - m.offset;
        const bool del = v.kind == LRM_CALL_DEL, at_start = del && off == 0;
        if (v.kind != LRM_CALL_SNV && v.kind != LRM_CALL_DEL && v.kind != LRM_CALL_INS) { lrm_set_error("VCF text: record %llu has kind %u", (unsigned long long) k, v.kind); return -1; }
        if (del && (v.len == 0 || v.len > m.seq_len - off || (at_start && v.len == m.seq_len))) {
            lrm_set_error("VCF text: a deletion of %u bases at position %llu leaves its sequence", v.len, (unsigned long long) pos);
            return -1;
        }
        // the name, nine tabs and the newline, a 20-digit position, '.', REF, ALT, '.', '.', DP= and ;INSFULL, GT:AD, the
        // genotype, three 10-digit counts, ':' and ','
        const uint64_t ref_len = del ? (uint64_t) v.len + 1u : 1u;
        const uint64_t room = name_len + 10u + 20u + 1u + ref_len + (1u + LRM_PILEUP_INS_COLS_MAX + 5u) + 2u + (3u + 8u) + 5u + 3u + 3u * 10u + 2u;
        if ((uint64_t) (buflen - at) < room + 1) return vcf_small(buflen);   // (+1: the NUL)
        char *p = buf + at;
        memcpy(p, m.name ? m.name : "", name_len);
        p += name_len;
        *p++ = '\t';
        p += put_uint(p, del ? (at_start ? 1u : off) : off + 1u);       // a deletion is anchored on the base before it
        *p++ = '\t'; *p++ = '.'; *p++ = '\t';
        if (del) {
            const uint64_t from = at_start ? pos : pos - 1u;
            for (uint64_t j = 0; j < ref_len; ++j) *p++ = vcf_upper((uint8_t) content[from + j]);
            *p++ = '\t';
            *p++ = vcf_upper((uint8_t) content[at_start ? pos + v.len : pos - 1u]);
        } else if (v.kind == LRM_CALL_SNV) {
            *p++ = vcf_upper(v.ref);
            *p++ = '\t';
            *p++ = (char) v.alt;
        } else {
            const uint32_t len = v.len < LRM_PILEUP_INS_COLS_MAX ? v.len : LRM_PILEUP_INS_COLS_MAX;
            *p++ = vcf_upper(v.ref);
            *p++ = '\t';
            if (len == 0) { memcpy(p, "<INS>", 5); p += 5; }
            else { *p++ = vcf_upper(v.ref); memcpy(p, v.bases, len); p += len; }
        }
        memcpy(p, "\t.\t.\tDP=", 8); p += 8;
        p += put_uint(p, v.depth);
        if (v.kind == LRM_CALL_INS && (v.ins_flags & LRM_INS_FULL)) { memcpy(p, ";INSFULL", 8); p += 8; }
        memcpy(p, "\tGT:AD\t", 7); p += 7;
        memcpy(p, v.gt == 2 ? "1/1" : "0/1", 3); p += 3;
        *p++ = ':';
        p += put_uint(p, v.n_ref);
        *p++ = ',';
        p += put_uint(p, v.n_alt);
        *p++ = '\n';
        at = p - buf;
    }
    buf[at] = '\0';
    return at;
}
