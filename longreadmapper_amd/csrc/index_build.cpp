// index_build.cpp -- the index from its text: lrm_cat_from_seqs (.cat text + .mta table of a set of sequences) and
// lrm_host_index_build (suffix array through suffix_sort.cpp, then the C, BWT, O, CSA and lchash tables derived from it; the
// lchash in one pass over the suffix array instead of 4^hlen backward searches).  include/lrm_index_host.h
#include <algorithm>
#include "../../include/lrm_index_host.h"
#include "packed_text.h"

namespace {

inline uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// base_code that also takes lower case.  lrm_cat_from_seqs upper-cases, so its texts never need it; a text handed straight
// to lrm_host_index_build is taken as it is, and the O table and the lchash of one with lower-case bases have always
// counted those as bases.  Only these two tables of such a text (not pure: it has no 2-bit image) go through it.
inline int base_code_any_case(char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return -1; }
}

}  // namespace

extern "C" int lrm_cat_from_seqs(const char *const *names, const char *const *seqs, const uint64_t *lens, int nseq,
                                 uint64_t n_seed, char **cat_out, uint64_t *cat_len, lrm_mta_entry **mta_out) {
    if (!seqs || !lens || nseq <= 0 || !cat_out || !cat_len || !mta_out) { lrm_set_error("bad argument"); return -1; }
    uint64_t total = 1;
    for (int i = 0; i < nseq; ++i) total += 2 * lens[i];
    char *cat = (char *) malloc(total + 1);
    lrm_mta_entry *mta = (lrm_mta_entry *) calloc((size_t) nseq, sizeof(lrm_mta_entry));
    if (!cat || !mta) { free(cat); free(mta); lrm_set_error("out of memory"); return -1; }
    uint64_t off = 0, rs = n_seed;
    for (int i = 0; i < nseq; ++i) {
        const uint64_t n = lens[i];
        char nm[32];
        const char *name = names && names[i] ? names[i] : nm;
        if (!(names && names[i])) snprintf(nm, sizeof(nm), "seq%d", i);
        mta[i].name_len = strlen(name);
        mta[i].name = strdup(name);
        mta[i].name_own = 1;
        mta[i].offset = off;                          // asindex.c:89-93
        mta[i].seq_len = n;
        // N/n -> pseudo-random base (asindex.c:53-60; seeded per position here, so the result does not depend on
        // the thread count), upper-casing (asindex.c:63-68)
        uint64_t bad_pos = ~0ull;
        const uint64_t rs0 = splitmix64(rs);
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static) reduction(min : bad_pos)
        for (uint64_t p = 0; p < n; ++p) {
            char c = seqs[i][p];
            if (c == 'n' || c == 'N') { uint64_t st = rs0 ^ (p * 0x9E3779B97F4A7C15ull); c = "ACGT"[splitmix64(st) & 3]; }
            if (c > 0x60) c -= 0x20;
            if (base_code(c) < 0 && p < bad_pos) bad_pos = p;
            cat[off + p] = c;
        }
        if (bad_pos != ~0ull) {
            lrm_set_error("sequence %d offset %llu: byte 0x%02x is not a nucleotide", i, (unsigned long long) bad_pos, (unsigned) (unsigned char) seqs[i][bad_pos]);
            free(cat); lrm_mta_free(mta, nseq);
            return -1;
        }
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
        for (uint64_t p = 0; p < n; ++p) cat[off + n + p] = "TGCA"[base_code(cat[off + n - 1 - p])];   // asindex.c:70-75
        off += 2 * n;
    }
    cat[off++] = '$';                                  // asindex.c:109-110
    cat[off] = 0;
    *cat_out = cat; *cat_len = off; *mta_out = mta;
    return 0;
}

extern "C" void lrm_mta_free(lrm_mta_entry *mta, int n) {
    if (!mta) return;
    for (int i = 0; i < n; ++i) if (mta[i].name_own) free(mta[i].name);
    free(mta);
}

extern "C" void lrm_host_index_free(lrm_host_index *idx) {
    if (!idx) return;
    free(idx->fmi.c); free(idx->fmi.o); free(idx->fmi.csa); free(idx->fmi.bwt);
    free(idx->lch.lc); free(idx->sa.mem); free(idx->content);
    lrm_mta_free(idx->mta, idx->mta_len);
    memset(idx, 0, sizeof(*idx));
}

// ------------------------------------------------------------------------------------------
// The steps of lrm_host_index_build, in the order the driver below runs them.  Each allocates its table ("out of
// memory" is its only failure) and fills it with all host threads.
// ------------------------------------------------------------------------------------------
namespace {

struct BuildInput {                 // what the steps read
    const char *text; uint64_t L;   // the text, '$' at L-1
    const PackedText &pt;           // its 2-bit image, valid if pure: random accesses touch a quarter of the footprint
    bool pure;                      // upper-case ACGT only
    const lrm_ui40 *sa;             // its suffix array
    inline uint64_t sa_at(uint64_t row) const { return ui40_get(sa[row]); }
    inline char base_before(uint64_t v) const { return v == 0 ? '$' : (pure ? "ACGT"[pt.base(v - 1)] : text[v - 1]); }
};

// the text (+ NUL) and the mta table (names duplicated) into the index
bool copy_text_and_mta(const char *cat, uint64_t L, const lrm_mta_entry *mta, int mta_len, lrm_host_index *out) {
    if (!lrm_alloc(out->content, L + 1, "text") || !lrm_alloc(out->mta, (uint64_t) (mta_len > 0 ? mta_len : 1), "mta", true)) return false;
    const uint64_t piece = 1ull << 22, np = block_count(L, piece);
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
    for (uint64_t i = 0; i < np; ++i) { const BlockRange r = block_range(i, piece, L); memcpy(out->content + r.lo, cat + r.lo, r.hi - r.lo); }
    out->content[L] = 0;
    out->con_len = L;
    out->mta_len = mta_len;
    for (int i = 0; i < mta_len; ++i) {
        out->mta[i] = mta[i];
        out->mta[i].name = strdup(mta[i].name ? mta[i].name : "");
        out->mta[i].name_own = 1;
        if (!out->mta[i].name) { lrm_set_error("out of memory (mta name, %llu bytes)", (unsigned long long) mta[i].name_len + 1); return false; }
    }
    return true;
}

// C table: counts over text[0..L-2], exclusive prefix sums over all byte values (fmidx.c:101-125)
bool c_table(const BuildInput &in, lrm_dna_fmi *f) {
    if (!lrm_alloc(f->c, 256, "C table", true)) return false;
    const char *cat = in.text;
    const uint64_t L = in.L;
    uint64_t ca = 0, cc = 0, cg = 0, ct = 0, other = 0;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static) reduction(+ : ca, cc, cg, ct, other)
    for (uint64_t i = 0; i < L - 1; ++i) {
        switch (cat[i]) { case 'A': ca++; break; case 'C': cc++; break; case 'G': cg++; break; case 'T': ct++; break; default: other++; }
    }
    f->c[(unsigned char) 'A'] = ca; f->c[(unsigned char) 'C'] = cc; f->c[(unsigned char) 'G'] = cg; f->c[(unsigned char) 'T'] = ct;
    if (other) {                                       // generic bytes: the plain loop
        memset(f->c, 0, 256 * sizeof(uint64_t));
        for (uint64_t i = 0; i + 1 < L; ++i) f->c[(unsigned char) cat[i]]++;
    }
    uint64_t sum = 0;
    for (int i = 0; i < 256; ++i) { const uint64_t t = sum + f->c[i]; f->c[i] = sum; sum = t; }
    return true;
}

// BWT (fmidx.c:76-98)
bool bwt(const BuildInput &in, lrm_dna_fmi *f) {
    f->length = in.L;
    if (!lrm_alloc(f->bwt, in.L + 1, "bwt")) return false;
    char *b = f->bwt;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
    for (uint64_t i = 0; i < in.L; ++i) b[i] = in.base_before(in.sa_at(i));
    b[in.L] = 0;
    return true;
}

// c[x] += rows of bwt[lo, hi) that hold base x
inline void count4(const char *bwt, uint64_t lo, uint64_t hi, uint64_t *c) {
    for (uint64_t i = lo; i < hi; ++i) { const int code = base_code_any_case(bwt[i]); if (code >= 0) c[code]++; }
}

// O table (fmidx.c:128-150,186-190): the four counts over bwt[0, i) for every i that is a multiple of o_ratio
bool o_table(uint64_t L, int o_ratio, lrm_dna_fmi *f) {
    f->o_ratio = o_ratio;
    f->o_len = 4 * (L / (uint64_t) o_ratio + 1);
    if (!lrm_alloc(f->o, f->o_len, "O table", true)) return false;
    // segments of SEG sample intervals: counts per segment first, then every segment fills its samples
    const uint64_t R = (uint64_t) o_ratio, SEG = 1ull << 15, rows_per_seg = SEG * R, nseg = block_count(L, rows_per_seg);
    const char *b = f->bwt;
    std::vector<uint64_t> segc((nseg + 1) * 4, 0);
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
    for (uint64_t sg = 0; sg < nseg; ++sg) {
        uint64_t c[4] = {0, 0, 0, 0};
        const BlockRange r = block_range(sg, rows_per_seg, L);
        count4(b, r.lo, r.hi, c);
        memcpy(&segc[(sg + 1) * 4], c, sizeof(c));
    }
    for (uint64_t sg = 1; sg <= nseg; ++sg) for (int x = 0; x < 4; ++x) segc[sg * 4 + x] += segc[(sg - 1) * 4 + x];
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
    for (uint64_t sg = 0; sg < nseg; ++sg) {
        uint64_t run[4] = {segc[sg * 4], segc[sg * 4 + 1], segc[sg * 4 + 2], segc[sg * 4 + 3]};
        const BlockRange r = block_range(sg, rows_per_seg, L);
        for (uint64_t i = r.lo; i < r.hi; i += R) {            // a segment starts on a sample row
            memcpy(f->o + 4 * (i / R), run, sizeof(run));
            count4(b, i, i + R < r.hi ? i + R : r.hi, run);
        }
    }
    // (when L is a multiple of R the sample past the last row stays 0, as fmidx.c:135-147 leaves it)
    return true;
}

// CSA (fmidx.c:153-163,194)
bool csa(const BuildInput &in, lrm_dna_fmi *f) {
    f->csa_ratio = 4;
    f->csa_len = in.L / 4 + 1;
    if (!lrm_alloc(f->csa, f->csa_len, "csa", true)) return false;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
    for (uint64_t i = 0; i < f->csa_len; ++i) f->csa[i] = i * 4 < in.L ? in.sa_at(i * 4) : 0;
    return true;
}

// lchash (lchash.c:52-73): the SA interval of every hlen-mer.  Suffixes sharing their first
// hlen bases are contiguous in the SA, so one pass finds every interval's first/last row.
// Quirk kept: fmi_aln starts from rows [1, L-1] (lchash.c:56), i.e. without the '$' row, so
// the occurrence that ends on the very last base of the text (the suffix "P$", always the
// first row of P's interval) is never found.  That row is skipped here as well.
bool lchash(const BuildInput &in, int hlen, lrm_lc_hash *h) {
    const uint64_t L = in.L, upper = 1ull << (2 * hlen);
    h->hlen = hlen;
    h->len = 2 * upper;
    if (!lrm_alloc(h->lc, 2 * upper, "lchash", true)) return false;
    uint64_t *lc = h->lc;
    auto code_at = [&](uint64_t row, uint64_t &code) -> bool {
        const uint64_t pos = in.sa_at(row);
        if (pos + (uint64_t) hlen >= L - 1) return false;         // runs into '$', or is the "P$" row (see above)
        if (in.pure) { code = in.pt.window(pos) >> (64 - 2 * hlen); return true; }   // first base most significant (lchash.c:36-49)
        uint64_t c = 0;
        for (int i = 0; i < hlen; ++i) c = (c << 2) | (uint64_t) base_code_any_case(in.text[pos + i]);
        code = c;
        return true;
    };
    // one text access per row: the codes of a block of rows first, then the interval boundaries inside it
    const uint64_t RB = 1ull << 16, nrb = block_count(L, RB);
#pragma omp parallel num_threads(lrm_host_threads())
    {
        std::vector<uint64_t> codes(RB + 2);
#pragma omp for schedule(dynamic, 4)
        for (uint64_t b = 0; b < nrb; ++b) {
            const BlockRange blk = block_range(b, RB, L);
            const uint64_t lo = blk.lo, hi = blk.hi, NONE = ~0ull;
            for (uint64_t r = (lo ? lo - 1 : lo); r < (hi < L ? hi + 1 : hi); ++r) {
                uint64_t c;
                codes[r + 1 - lo] = code_at(r, c) ? c : NONE;
            }
            for (uint64_t r = lo; r < hi; ++r) {
                const uint64_t cur = codes[r + 1 - lo];
                if (cur == NONE) continue;
                if (r == 0 || codes[r - lo] != cur) lc[2 * cur] = r;
                if (r + 1 == L || codes[r + 2 - lo] != cur) lc[2 * cur + 1] = r;
            }
        }
    }
    return true;
}

int build_failed(lrm_host_index *out) { lrm_host_index_free(out); return -1; }     // the step that failed has set the message

}  // namespace

extern "C" int lrm_host_index_build(const char *cat, uint64_t L, const lrm_mta_entry *mta, int mta_len, int o_ratio,
                                    int hlen, lrm_host_index *out) {
    if (!cat || !out || L < 2 || o_ratio < 1 || hlen < 1 || hlen > 15) { lrm_set_error("bad argument"); return -1; }
    memset(out, 0, sizeof(*out));
    const BuildKnobs knobs = build_knobs();
    if (!copy_text_and_mta(cat, L, mta, mta_len, out) || !lrm_alloc(out->sa.mem, L, "suffix array")) return build_failed(out);
    out->sa.start = 0;
    out->sa.len = L;
    StageTimer tm(knobs.verbose);
    PackedText pt;
    const bool pure = pack_text(cat, L, pt);
    tm.lap("pack 2-bit");
    if (sa_build(cat, L, pure ? &pt : nullptr, knobs, out->sa.mem)) return build_failed(out);
    tm.lap("suffix array");
    const BuildInput in{cat, L, pt, pure, out->sa.mem};
    if (!c_table(in, &out->fmi) || !bwt(in, &out->fmi)) return build_failed(out);
    tm.lap("C + bwt");
    if (!o_table(L, o_ratio, &out->fmi)) return build_failed(out);
    tm.lap("O table");
    if (!csa(in, &out->fmi)) return build_failed(out);
    tm.lap("csa");
    if (!lchash(in, hlen, &out->lch)) return build_failed(out);
    tm.lap("lchash");
    return 0;
}
