// pileup_step.h -- the per-word step of the pileup (docs/GACT_SPEC.md, "Pileup"): from the byte masks of four op bytes to
// the counts they add -- which plane, which target column.  Read by pileup_kernels.hip (a lane's 16 columns are four such
// words) and, as plain C++, by lrm_pileup_add_host (pileup.hip) and tests/models/pileup_host_harness.cpp: the host rule and
// the CPU tests run the kernel's own source.
#pragma once
#include <stdint.h>
#include "op_rows.h"                     // the byte masks, a byte out of four words, the walk of a row on the host

// The planes of an accumulator over a window of W positions, all 32-bit words in one allocation of 8 * W + 1 words:
//   [0, W]                     the DIFFERENCE plane of the depth: +1 where a read's covered interval starts, -1 where it ends
//                              (W + 1 words: an interval that ends at `hi` puts its -1 into word W)
//   W + 1 + k * W + [0, W)     event plane k
#define LRM_PILEUP_X_A 0u
#define LRM_PILEUP_X_C 1u
#define LRM_PILEUP_X_G 2u
#define LRM_PILEUP_X_T 3u
#define LRM_PILEUP_X_OTHER 4u
#define LRM_PILEUP_DEL 5u
#define LRM_PILEUP_INS 6u
#define LRM_PILEUP_PLANES 7u
#define LRM_PILEUP_WORDS(W) (8ull * (uint64_t) (W) + 1ull)
#define LRM_PILEUP_EVENT_PLANE(W, k) ((uint64_t) (W) + 1ull + (uint64_t) (k) * (uint64_t) (W))
// Rows longer than this cannot be described: n_ops is a positive int32, and the column, target and query counts of a row
// are 32-bit.  (The 16-bit halves of the scanned word hold the counts of ONE step of 1024 columns, at most 1024 each: they
// set no bound on the row; the running counts are carried as whole words.)
#define LRM_PILEUP_MAX_STRIDE (1ull << 31)

// the class of a read byte: A/a, C/c, G/g, T/t, other (selects, as comp_base of seq_bytes.h folds the case)
LRM_OP_FN uint32_t pile_base_class(uint32_t byte) {
    const uint32_t u = byte & 0xDFu;
    uint32_t r = LRM_PILEUP_X_OTHER;
    r = u == 'A' ? LRM_PILEUP_X_A : r;
    r = u == 'C' ? LRM_PILEUP_X_C : r;
    r = u == 'G' ? LRM_PILEUP_X_G : r;
    r = u == 'T' ? LRM_PILEUP_X_T : r;
    return r;
}

// The counts of one word in column order.  t: target-consuming columns of the ROW before this word, q: query-consuming
// columns of the LANE before this word (the index of the word's first query byte among the lane's 16 read bytes q0..q3);
// both move on by the word.  add(plane, tcol) is called once per 'X' column (the class of its read byte), once per 'D'
// column and once per 'I' column that opens a run behind at least one target column (tcol: the column before it); the
// count belongs to text position loc + tcol.
template <typename Add>
LRM_OP_FN void pile_word_step(const OpMasks &m, uint32_t &t, uint32_t &q, uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, Add add) {
    const uint32_t tm = m.eq | m.x | m.d, qm = m.eq | m.x | m.i | m.s;
    uint32_t ev = m.x | m.d | m.i_open;
    while (ev) {
        const uint32_t bit = ev & (0u - ev);                         // 0x80 of the event's byte
        const uint32_t below = bit - 1u;                             // every mask bit of the columns before it
        const uint32_t tl = t + (uint32_t) __builtin_popcount(tm & below);
        if (m.x & bit) add(pile_base_class(op_pick_byte(q0, q1, q2, q3, (q + (uint32_t) __builtin_popcount(qm & below)) & 15u)), tl);
        else if (m.d & bit) add(LRM_PILEUP_DEL, tl);
        else if (tl) add(LRM_PILEUP_INS, tl - 1u);                   // (a run with no target column before it: nowhere)
        ev &= ev - 1u;
    }
    t += (uint32_t) __builtin_popcount(tm);
    q += (uint32_t) __builtin_popcount(qm);
}

// The eight words of the record of window position g (lrm_pileup_col: depth, n_eq, x_a, x_c, x_g, x_t, n_del, n_ins) from its
// depth and its seven event words: every read that covers the position and is neither an 'X' nor a 'D' there is an '='.
LRM_OP_FN void pile_col_words(const uint32_t *planes, uint64_t W, uint64_t g, uint32_t depth, uint32_t (&w)[8]) {
    uint32_t e[LRM_PILEUP_PLANES];
    for (uint32_t k = 0; k < LRM_PILEUP_PLANES; ++k) e[k] = planes[LRM_PILEUP_EVENT_PLANE(W, k) + g];
    const uint32_t x_all = e[LRM_PILEUP_X_A] + e[LRM_PILEUP_X_C] + e[LRM_PILEUP_X_G] + e[LRM_PILEUP_X_T] + e[LRM_PILEUP_X_OTHER];
    w[0] = depth; w[1] = depth - x_all - e[LRM_PILEUP_DEL]; w[2] = e[LRM_PILEUP_X_A]; w[3] = e[LRM_PILEUP_X_C];
    w[4] = e[LRM_PILEUP_X_G]; w[5] = e[LRM_PILEUP_X_T]; w[6] = e[LRM_PILEUP_DEL]; w[7] = e[LRM_PILEUP_INS];
}

// ---- the rule on the host (lrm_pileup_add_host, lrm_pileup_cols_host; tests/models/pileup_host_harness.cpp) ----
// One aligned read into planes of a window [lo, hi), lo < hi.  The row is walked as a lane of pileup_add_kernel walks it, 16
// columns at a time through pile_word_step: the 16 read bytes from the lane's first query position on (zeros from read_len on).
static inline void pile_host_add(const uint8_t *ops, uint64_t n, const uint8_t *read, uint32_t read_len, uint64_t loc, uint64_t lo,
                                 uint64_t hi, uint32_t *planes) {
    const uint64_t W = hi - lo;
    uint32_t t = 0, q_row = 0;
    op_host_walk(ops, n, [&](const uint32_t (&cw)[4], const uint32_t (&pw)[4]) {
        uint32_t qb[4];
        for (int k = 0; k < 4; ++k) qb[k] = op_host_word(read, (uint64_t) q_row + 4u * (uint64_t) k, read_len);
        uint32_t q = 0;
        for (int k = 0; k < 4; ++k)
            pile_word_step(op_masks(cw[k], pw[k]), t, q, qb[0], qb[1], qb[2], qb[3], [&](uint32_t plane, uint32_t tcol) {
                const uint64_t pos = loc + tcol;
                if (pos >= lo && pos < hi) planes[LRM_PILEUP_EVENT_PLANE(W, plane) + (pos - lo)] += 1u;
            });
        q_row += q;
    });
    const uint64_t a = loc > lo ? loc : lo, end = loc + t, b = end < hi ? end : hi;
    if (a < b) {                                                     // the covered interval clipped to the window
        planes[a - lo] += 1u;
        planes[b - lo] -= 1u;                                        // word W when the interval reaches hi
    }
}
// the records of window positions [first, first + count) from such planes, first + count <= hi - lo
static inline void pile_host_cols(const uint32_t *planes, uint64_t W, uint64_t first, uint64_t count, lrm_pileup_col *out) {
    uint32_t depth = 0;
    for (uint64_t g = 0; g < first + count; ++g) {
        depth += planes[g];
        if (g < first) continue;
        uint32_t w[8];
        pile_col_words(planes, W, g, depth, w);
        out[g - first] = lrm_pileup_col{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
    }
}
