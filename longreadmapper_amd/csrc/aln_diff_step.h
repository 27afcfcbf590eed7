// aln_diff_step.h -- the per-word step of the difference events (docs/GACT_SPEC.md, "Difference events and MD:Z"): from the
// byte masks of four op bytes to their event words.  Read by aln_diff_kernels.hip (a lane's 16 columns are four such words)
// and, as plain C++, by the host rule below (lrm_aln_diff_host): the host rule and the CPU tests run the kernel's own source.
#pragma once
#include <stdint.h>
#include "../../include/lrm_accel.h"      // LRM_DIFF_X / _D_OPEN / _D_MORE: the kinds of an event word
#include "op_rows.h"                      // the byte masks, a byte out of four words, the walk of a row on the host

#define LRM_DIFF_E_SHIFT 10          // bits 10-31: '=' columns before the event
#define LRM_DIFF_MAX_STRIDE (1u << 22)

// The events of one word in column order.  t: target-consuming columns of the lane before this word (the index of the
// word's first target byte among the lane's 16 text bytes t0..t3), e: '=' columns of the row before this word; both move on
// by the word.  emit(word) is called once per 'X' / 'D' column.
template <typename Emit>
LRM_OP_FN void diff_word_step(const OpMasks &m, uint32_t &t, uint32_t &e, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, Emit emit) {
    const uint32_t tm = m.eq | m.x | m.d;
    uint32_t ev = m.x | m.d;
    while (ev) {
        const uint32_t bit = ev & (0u - ev);                         // 0x80 of the event's byte
        const uint32_t below = bit - 1u;                             // every mask bit of the columns before it
        const uint32_t tl = t + (uint32_t) __builtin_popcount(tm & below);
        const uint32_t ee = e + (uint32_t) __builtin_popcount(m.eq & below);
        const uint32_t kind = (m.x & bit) ? LRM_DIFF_X : ((m.d_open & bit) ? LRM_DIFF_D_OPEN : LRM_DIFF_D_MORE);
        emit(op_pick_byte(t0, t1, t2, t3, tl) | (kind << 8) | (ee << LRM_DIFF_E_SHIFT));
        ev &= ev - 1u;
    }
    t += (uint32_t) __builtin_popcount(tm);
    e += (uint32_t) __builtin_popcount(m.eq);
}

// ---- the rule on the host (lrm_aln_diff_host) ----
// The events of a row of n op bytes into events_out (null: only the count).  The row is walked as a lane of aln_diff_kernel walks it,
// 16 columns at a time through diff_word_step: the 16 target bytes from the lane's first target position on (zeros from target_len on).
static inline uint64_t diff_host_events(const uint8_t *ops, uint64_t n, const uint8_t *target, uint64_t target_len, uint32_t *events_out) {
    uint64_t t_row = 0, count = 0;
    uint32_t e = 0;
    op_host_walk(ops, n, [&](const uint32_t (&cw)[4], const uint32_t (&pw)[4]) {
        uint32_t text[4];
        for (int k = 0; k < 4; ++k) text[k] = op_host_word(target, t_row + 4u * (uint64_t) k, target_len);
        uint32_t t = 0;
        for (int k = 0; k < 4; ++k)
            diff_word_step(op_masks(cw[k], pw[k]), t, e, text[0], text[1], text[2], text[3], [&](uint32_t word) {
                if (events_out) events_out[count] = word;
                ++count;
            });
        t_row += t;
    });
    return count;
}
