// pileup_ins_step.h -- the insertion columns of the pileup (docs/GACT_SPEC.md, "Pileup insertions and the polished
// consensus"): from the byte masks of four op bytes to the inserted bases they count, from a position's insertion words to
// its inserted allele, and from a position's consensus letter and allele to its bytes of the polished sequence.  Read by
// pileup_kernels.hip (pileup_add_ins_kernel, the polish kernels, the site-allele gather) and, as plain C++, by
// lrm_pileup_ins_add_host, lrm_pileup_ins_allele_host and lrm_pileup_polish_host (pileup.hip) and
// tests/models/pileup_ins_harness.cpp: the host rules and the CPU tests run the kernels' own source.  All arithmetic is integer.
#pragma once
#include <stdint.h>
#include "pileup_call_step.h"            // the thresholds, pile_call; pileup_step.h: pile_base_class; op_rows.h: the masks

// The insertion planes of an accumulator with K insertion columns over a window of W positions, 32-bit words in an
// allocation of their own of 4 * K * W words: plane 4 * j + k, insertion column j < K, base class k (A, C, G, T).
#define LRM_PILEUP_INS_WORDS(W, K) (4ull * (uint64_t) (K) * (uint64_t) (W))
#define LRM_PILEUP_INS_PLANE(W, j, k) ((4ull * (uint64_t) (j) + (uint64_t) (k)) * (uint64_t) (W))
// the place of a column in its 'I' run is carried from lane to lane saturated at a lane's 16 columns: K <= 8 < 16
#define LRM_PILEUP_INS_RUN_SAT 16u

// how many of a word's last columns are 'I' (0..4): the columns behind its last column that is none
LRM_OP_FN uint32_t pile_ins_trailing(uint32_t i_mask) {
    const uint32_t none = ~i_mask & 0x80808080u;
    return none ? (uint32_t) __builtin_clz(none) >> 3 : 4u;
}
// the 'I' columns in front of the column behind a word's last one: `run` in front of the word's first column
LRM_OP_FN uint32_t pile_ins_run_behind(uint32_t i_mask, uint32_t run) {
    const uint32_t trail = pile_ins_trailing(i_mask);
    const uint32_t next = trail == 4u ? run + 4u : trail;
    return next < LRM_PILEUP_INS_RUN_SAT ? next : LRM_PILEUP_INS_RUN_SAT;
}

// The inserted bases of one word in column order, K columns per run.  t, q: as pile_word_step takes them -- they do NOT move
// on here (pile_word_step runs over the same word); run: the 'I' columns immediately in front of the word's first column
// (saturated), it moves on by the word.  add(j, k, tcol): once per 'I' column that is the j-th of its run, j < K, behind at
// least one target column (tcol: the column before the run) and whose read byte is a base of class k.
template <typename Add>
LRM_OP_FN void pile_ins_word_step(const OpMasks &m, uint32_t t, uint32_t q, uint32_t &run, uint32_t K, uint32_t q0, uint32_t q1, uint32_t q2,
                                  uint32_t q3, Add add) {
    const uint32_t tm = m.eq | m.x | m.d, qm = m.eq | m.x | m.i | m.s;
    uint32_t ev = m.i;
    while (ev) {
        const uint32_t bit = ev & (0u - ev);                         // 0x80 of the column's byte
        const uint32_t below = bit - 1u;                             // every mask bit of the columns before it
        const uint32_t col = (uint32_t) __builtin_popcount(below & 0x80808080u);
        const uint32_t none = ~m.i & below & 0x80808080u;            // the columns before it that are no 'I'
        const uint32_t j = none ? col - 1u - ((31u - (uint32_t) __builtin_clz(none)) >> 3) : col + run;
        const uint32_t tl = t + (uint32_t) __builtin_popcount(tm & below);
        if (j < K && tl) {
            const uint32_t k = pile_base_class(op_pick_byte(q0, q1, q2, q3, (q + (uint32_t) __builtin_popcount(qm & below)) & 15u));
            if (k < 4u) add(j, k, tl - 1u);
        }
        ev &= ev - 1u;
    }
    run = pile_ins_run_behind(m.i, run);
}

// ---- the inserted allele of one position ----
#define LRM_PILEUP_INS_COLS_LIMIT 8u     // LRM_PILEUP_INS_COLS_MAX of the header
// bases: the allele's letters, byte j for column j, 0 from len on (one 64-bit word: shifts, no indexed bytes in a kernel)
struct PileInsAllele { uint32_t n_col0, len, flags; uint64_t bases; };

// the position enters the polished sequence with its allele: the reads that insert here are the majority of all reads
LRM_OP_FN bool pile_ins_enters(const PileCallRule &r, uint32_t depth, uint32_t n_ins) {
    return depth >= r.min_depth && 2ull * (uint64_t) n_ins > (uint64_t) depth;
}
// s[(4 * j + k) * stride]: the position's insertion words (stride 1: position-major, as lrm_pileup_ins_read_dev writes them;
// stride W: the planes themselves).  sup[j] is the 32-bit sum of a column's four words, wrapping like the counters; len
// counts the leading columns whose support is the majority of the reads that insert here (64-bit products); a tie between
// classes goes to the earlier of A, C, G, T (a strict `>`).
template <typename Stride>
LRM_OP_FN PileInsAllele pile_ins_allele(const PileCallRule &r, uint32_t depth, uint32_t n_ins, const uint32_t *s, Stride stride, uint32_t K) {
    PileInsAllele a;
    a.n_col0 = 0;
    a.len = 0;
    a.bases = 0;
    for (uint32_t j = 0; j < K; ++j) {
        const uint32_t *c = s + (uint64_t) (4u * j) * (uint64_t) stride;
        const uint32_t v0 = c[0], v1 = c[(uint64_t) stride], v2 = c[2ull * (uint64_t) stride], v3 = c[3ull * (uint64_t) stride];
        const uint32_t sup = v0 + v1 + v2 + v3;
        uint32_t best = v0, base = 'A';
        if (v1 > best) { best = v1; base = 'C'; }
        if (v2 > best) { best = v2; base = 'G'; }
        if (v3 > best) { best = v3; base = 'T'; }
        if (j == 0) a.n_col0 = sup;
        if (2ull * (uint64_t) sup <= (uint64_t) n_ins) break;        // the leading columns only
        a.bases |= (uint64_t) base << (8u * j);
        a.len = j + 1u;
    }
    a.flags = (pile_ins_enters(r, depth, n_ins) ? LRM_INS_ENTERS : 0u) | (K != 0u && a.len == K ? LRM_INS_FULL : 0u);
    return a;
}
// the 16-byte record (lrm_pileup_ins_allele: n_col0, then the bytes len, flags, pad[2], then bases[8]) as four words
LRM_OP_FN void pile_ins_allele_words(const PileInsAllele &a, uint32_t (&w)[4]) {
    w[0] = a.n_col0;
    w[1] = a.len | (a.flags << 8);
    w[2] = (uint32_t) a.bases;
    w[3] = (uint32_t) (a.bases >> 32);
}

// ---- the polished sequence ----
// The bytes of one position: its cons letter unless that is '-', then -- when the position enters -- the allele's bases.
// The insertion words are read only where 2 * n_ins > depth: words() is called there and nowhere else.  n bytes, 0 .. 9:
// byte j < 8 is byte j of `b`, byte 8 is `last`.
struct PilePolish { uint32_t n, last; uint64_t b; };
LRM_OP_FN uint32_t pile_polish_byte(const PilePolish &p, uint32_t j) { return j < 8u ? (uint32_t) (p.b >> (8u * j)) & 0xFFu : p.last; }
template <typename Words>
LRM_OP_FN PilePolish pile_polish_at(const PileCallRule &r, uint8_t cons, uint32_t depth, uint32_t n_ins, uint32_t K, Words words) {
    uint32_t len = 0;
    uint64_t bases = 0;
    if (K != 0u && pile_ins_enters(r, depth, n_ins)) {
        const PileInsAllele a = words();
        len = a.len;
        bases = a.bases;
    }
    const bool letter = cons != (uint8_t) '-';
    PilePolish p;
    p.n = (letter ? 1u : 0u) + len;
    p.b = letter ? (uint64_t) cons | (bases << 8) : bases;
    p.last = letter ? (uint32_t) (bases >> 56) : 0u;
    return p;
}

// ---- the rules on the host (lrm_pileup_ins_add_host, lrm_pileup_polish_host; tests/models/pileup_ins_harness.cpp) ----
// One aligned read into the insertion planes (4 * K * (hi - lo) words) of a window [lo, hi), lo < hi, 1 <= K <= 8.  The row
// is walked as a lane of pileup_add_ins_kernel walks it: 16 columns at a time, the 16 read bytes from the lane's first
// query position on (zeros from read_len on), the run carried from lane to lane.
static inline void pile_ins_host_add(const uint8_t *ops, uint64_t n, const uint8_t *read, uint32_t read_len, uint64_t loc, uint64_t lo,
                                     uint64_t hi, uint32_t K, uint32_t *ins) {
    const uint64_t W = hi - lo;
    uint32_t t = 0, q_row = 0, run = 0;
    op_host_walk(ops, n, [&](const uint32_t (&cw)[4], const uint32_t (&pw)[4]) {
        uint32_t qb[4];
        for (int k = 0; k < 4; ++k) qb[k] = op_host_word(read, (uint64_t) q_row + 4u * (uint64_t) k, read_len);
        uint32_t q = 0;
        for (int k = 0; k < 4; ++k) {
            const OpMasks m = op_masks(cw[k], pw[k]);
            pile_ins_word_step(m, t, q, run, K, qb[0], qb[1], qb[2], qb[3], [&](uint32_t j, uint32_t cls, uint32_t tcol) {
                const uint64_t pos = loc + tcol;
                if (pos >= lo && pos < hi) ins[LRM_PILEUP_INS_PLANE(W, j, cls) + (pos - lo)] += 1u;
            });
            t += (uint32_t) __builtin_popcount(m.eq | m.x | m.d);
            q += (uint32_t) __builtin_popcount(m.eq | m.x | m.i | m.s);
        }
        q_row += q;
    });
}
// The polished sequence of `count` positions: cols[k], content[k] and ins_words + 4 * K * k are the record, the text byte
// and the position-major insertion words of position k (K == 0: no insertion words, ins_words is not read).  Bytes into
// out[0 .. cap); returns the length whether or not it fits.
static inline uint64_t pile_host_polish(const lrm_pileup_col *cols, const uint32_t *ins_words, uint32_t K, const char *content, uint64_t count,
                                        const PileCallRule &r, uint8_t *out, uint64_t cap) {
    uint64_t total = 0;
    for (uint64_t g = 0; g < count; ++g) {
        const lrm_pileup_col &c = cols[g];
        const PileCall call = pile_call(r, c.depth, c.n_eq, c.x_a, c.x_c, c.x_g, c.x_t, c.n_del, c.n_ins, (uint8_t) content[g]);
        const PilePolish p = pile_polish_at(r, call.cons, c.depth, c.n_ins, K,
                                            [&]() { return pile_ins_allele(r, c.depth, c.n_ins, ins_words + 4ull * K * g, 1u, K); });
        for (uint32_t j = 0; j < p.n; ++j, ++total)
            if (total < cap) out[total] = (uint8_t) pile_polish_byte(p, j);
    }
    return total;
}
