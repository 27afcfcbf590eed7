// SPDX-License-Identifier: MIT
// End clipping of the anchored extension mode (docs/GACT_SPEC.md, "End clipping"): the lane-local fold and the merge
// operator of anchor_clip_kernel (anchor_kernels.hip).  The file compiles for the device and as plain C for the host,
// so tests/test_clip_cpu.py checks on the CPU the very source the kernel runs.
//
// A SEGMENT of op bytes c[0 .. len) is summarised as (sum, key): sum = s[len] of the spec's prefix scores s[k]
// ('=' +1, every other column -P), key = the best prefix of the segment, "largest score, then smallest k", as one
// unsigned word ((s[k] + AC_BIAS) << 32) | ~k under max.  Summaries merge associatively: the key of A ++ B is
// max(key_A, key_B moved by sum_A and |A|), and moving a key is one 64-bit addition.
#ifndef LRM_ANCHOR_CLIP_H
#define LRM_ANCHOR_CLIP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define AC_FN __host__ __device__ __forceinline__
#else
#define AC_FN static inline
#endif

#define AC_BIAS 0x80000000u          // scores lie in (-15 * 2^27, 2^27): s + AC_BIAS fits 32 bits
#define AC_LANE_COLS 16              // columns one lane folds per step (one 16-byte load)

struct AcSeg { int32_t sum; uint64_t key; };

AC_FN uint64_t ac_key(int32_t s, uint32_t k) { return ((uint64_t) ((uint32_t) s + AC_BIAS) << 32) | (uint64_t) (0xFFFFFFFFu - k); }
AC_FN int32_t ac_key_score(uint64_t key) { return (int32_t) ((uint32_t) (key >> 32) - AC_BIAS); }
AC_FN uint32_t ac_key_pos(uint64_t key) { return 0xFFFFFFFFu - (uint32_t) key; }
// the key of a segment that starts at column `len` of a row whose columns before it sum to `sum`
AC_FN uint64_t ac_key_move(uint64_t key, int32_t sum, uint32_t len) { return key + ((uint64_t) (int64_t) sum << 32) - (uint64_t) len; }

AC_FN struct AcSeg ac_empty(void) { struct AcSeg e; e.sum = 0; e.key = ac_key(0, 0); return e; }

// a: the row so far, len_a columns; b: the segment behind it
AC_FN struct AcSeg ac_merge(struct AcSeg a, uint32_t len_a, struct AcSeg b) {
    const uint64_t kb = ac_key_move(b.key, a.sum, len_a);
    struct AcSeg r;
    r.sum = a.sum + b.sum;
    r.key = kb > a.key ? kb : a.key;
    return r;
}

// 0x80 in every byte of x that is zero, 0 in the others (exact: no borrow crosses a byte)
AC_FN uint32_t ac_zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
// bit c set <=> byte c of the 16 bytes w[0 .. 4) (little endian) equals ch
AC_FN uint32_t ac_eq_mask(const uint32_t w[4], uint32_t ch) {
    const uint32_t rep = ch * 0x01010101u;
    uint32_t m = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t z = ac_zero_bytes(w[i] ^ rep) >> 7;                 // 0x01 per equal byte
        m |= (((z * 0x00204081u) >> 21) & 0xFu) << (4 * i);                // bytes' low bits gathered into 4 bits
    }
    return m;
}

// One lane's 16 columns, of which the first nvalid (0 .. 16) belong to the row: columns beyond them count for nothing.
// Inside the lane the key is 32 bits: ((s + 256) << 5) | (31 - k), s in [-240, 16], k in [0, 16].
AC_FN struct AcSeg ac_fold16(const uint32_t w[4], uint32_t nvalid, uint32_t P) {
    uint32_t eq = ac_eq_mask(w, '=');
    eq &= nvalid >= 16 ? 0xFFFFu : ((1u << nvalid) - 1u);                  // a column beyond the row is never '=' ...
    const int32_t up = (int32_t) P + 1;
    int32_t s = 256;
    uint32_t key = ((uint32_t) s << 5) | 31u;
    for (uint32_t c = 0; c < AC_LANE_COLS; ++c) {
        s += (int32_t) ((eq >> c) & 1u) * up - (int32_t) P;
        const uint32_t cand = ((uint32_t) s << 5) | (30u - c);
        key = cand > key ? cand : key;                                      // ... so it lowers s and never becomes the maximum
    }
    struct AcSeg r;
    r.sum = s - 256 + (int32_t) (P * (AC_LANE_COLS - (nvalid < 16 ? nvalid : 16)));     // and its -P is taken back here
    r.key = ac_key((int32_t) (key >> 5) - 256, 31u - (key & 31u));
    return r;
}

// The rule's last line: clipping must gain more than the end bonus B, else the row is kept whole.
AC_FN uint32_t ac_keep(struct AcSeg row, uint32_t m, uint32_t B) {
    return ac_key_score(row.key) - row.sum > (int32_t) B ? ac_key_pos(row.key) : m;
}

// columns of 16 bytes, among the first nvalid, that are NOT ch
AC_FN uint32_t ac_count_not(const uint32_t w[4], uint32_t nvalid, uint32_t ch) {
    const uint32_t valid = nvalid >= 16 ? 0xFFFFu : ((1u << nvalid) - 1u);
    return (uint32_t) __builtin_popcount(~ac_eq_mask(w, ch) & valid);
}
#endif
