// aln_diff_step.h -- the per-word step of the difference events (docs/GACT_SPEC.md, "Difference events and MD:Z"): from the
// byte masks of four op bytes to their event words.  Read by aln_diff_kernels.hip (a lane's 16 columns are four such words)
// and, as plain C++, by lrm_aln_diff_host (lrm_api.hip): the host rule and the CPU tests run the kernel's own source.
#pragma once
#include <stdint.h>
#include "../../include/lrm_accel.h"      // LRM_DIFF_X / _D_OPEN / _D_MORE: the kinds of an event word

#if defined(__HIPCC__)
#define LRM_DIFF_FN __host__ __device__ __forceinline__
#else
#define LRM_DIFF_FN inline
#endif

#define LRM_DIFF_E_SHIFT 10          // bits 10-31: '=' columns before the event
#define LRM_DIFF_MAX_STRIDE (1u << 22)

// 0x80 in every byte of w that equals c, 0 in every other: the EXACT zero-byte test on w ^ cccc (the cheaper form,
// (t - 0x01010101) & ~t & 0x80808080, lets a borrow run into the byte above a match: 'I' 'H' would count twice)
LRM_DIFF_FN uint32_t diff_bytes_equal(uint32_t w, uint32_t c) {
    const uint32_t t = w ^ (c * 0x01010101u);
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}

// the masks of one word of op bytes; pw: the column before each of its bytes
struct DiffMasks { uint32_t eq, x, d, d_open; };
LRM_DIFF_FN DiffMasks diff_masks(uint32_t cw, uint32_t pw) {
    DiffMasks m;
    m.eq = diff_bytes_equal(cw, '=');
    m.x = diff_bytes_equal(cw, 'X');
    m.d = diff_bytes_equal(cw, 'D');
    m.d_open = m.d & ~diff_bytes_equal(pw, 'D');
    return m;
}

// byte k (0..15) of 16 text bytes held in four words; selects, no indexed register
LRM_DIFF_FN uint32_t diff_text_byte(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t k) {
    const uint32_t w = (k & 8u) ? ((k & 4u) ? t3 : t2) : ((k & 4u) ? t1 : t0);
    return (w >> (8u * (k & 3u))) & 0xFFu;
}

// The events of one word in column order.  t: target-consuming columns of the lane before this word (the index of the
// word's first target byte among the lane's 16 text bytes t0..t3), e: '=' columns of the row before this word; both move on
// by the word.  emit(word) is called once per 'X' / 'D' column.
template <typename Emit>
LRM_DIFF_FN void diff_word_step(const DiffMasks &m, uint32_t &t, uint32_t &e, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, Emit emit) {
    const uint32_t tm = m.eq | m.x | m.d;
    uint32_t ev = m.x | m.d;
    while (ev) {
        const uint32_t bit = ev & (0u - ev);                         // 0x80 of the event's byte
        const uint32_t below = bit - 1u;                             // every mask bit of the columns before it
        const uint32_t tl = t + (uint32_t) __builtin_popcount(tm & below);
        const uint32_t ee = e + (uint32_t) __builtin_popcount(m.eq & below);
        const uint32_t kind = (m.x & bit) ? LRM_DIFF_X : ((m.d_open & bit) ? LRM_DIFF_D_OPEN : LRM_DIFF_D_MORE);
        emit(diff_text_byte(t0, t1, t2, t3, tl) | (kind << 8) | (ee << LRM_DIFF_E_SHIFT));
        ev &= ev - 1u;
    }
    t += (uint32_t) __builtin_popcount(tm);
    e += (uint32_t) __builtin_popcount(m.eq);
}
