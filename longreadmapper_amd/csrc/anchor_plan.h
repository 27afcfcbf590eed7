// anchor_plan.h -- what the scan's key of a read means: the key, the plan of the read's two jobs, the lrm_anchor record
// (anchor_kernels.hip; the debug tap in extend_taps.hip reads a key the same way)
#pragma once
#include <hip/hip_runtime.h>
#include "lrm_internal.h"

#define AN_HALF (LRM_ANCHOR_DIAGS / 2)

// ---- the key: larger is better -----------------------------------------------------------------------------------
// bits 40..63 length | 33..38 32 - |delta| | 32 delta < 0 | 0..31 ~j : longest run, then smallest |delta|, then
// smallest delta, then smallest j
__host__ __device__ static inline uint64_t an_key(uint32_t len, int delta, uint32_t j) {
    const uint32_t ad = (uint32_t) (delta < 0 ? -delta : delta);
    return ((uint64_t) len << 40) | ((uint64_t) (AN_HALF - ad) << 33) | ((uint64_t) (delta < 0) << 32) | (uint64_t) (0xFFFFFFFFu - j);
}

struct AnPlan {                               // what the key of a read means for its two jobs
    uint32_t flags, j, len;
    int32_t delta;
    uint64_t p;                               // text position of read[j]
    uint64_t left_loc;                        // start of the left job's target on the reverse-complement half
    uint32_t right_tlen, left_tlen;
};
__host__ __device__ static inline AnPlan an_plan(uint64_t key, uint64_t L, uint32_t n, uint64_t S, uint64_t len_s) {
    AnPlan a = {};
    if (key == 0) { a.flags = LRM_ANCHOR_FALLBACK; a.p = L; return a; }
    a.len = (uint32_t) (key >> 40);
    const int ad = AN_HALF - (int) ((key >> 33) & 63u);
    a.delta = ((key >> 32) & 1u) ? -ad : ad;
    a.j = 0xFFFFFFFFu - (uint32_t) key;
    a.p = (uint64_t) ((int64_t) L + a.delta + (int64_t) a.j);
    a.flags = LRM_ANCHOR_ANCHORED;
    const uint64_t nr = n - a.j, wr = nr + (nr + 7) / 8, room_r = S + len_s - a.p;
    a.right_tlen = (uint32_t) (wr < room_r ? wr : room_r);
    if (wr > room_r) a.flags |= LRM_ANCHOR_RIGHT_CLIPPED;
    if (a.j == 0) { a.flags |= LRM_ANCHOR_NO_LEFT; return a; }
    const uint64_t nl = a.j, wl = nl + (nl + 7) / 8, room_l = a.p - S;
    a.left_tlen = (uint32_t) (wl < room_l ? wl : room_l);
    if (wl > room_l) a.flags |= LRM_ANCHOR_LEFT_CLIPPED;
    a.left_loc = 2 * S + 2 * len_s - a.p;     // mirror of p - 1: y = 2S + 2 len_s - 1 - x
    return a;
}

// the record of a read: its plan, the ops of the reversed left job in front of the anchor, the soft-clip flags
__host__ __device__ static inline lrm_anchor an_record(const AnPlan &a, uint32_t left_ops, uint32_t soft_flags) {
    lrm_anchor an;
    an.text_pos = a.p; an.read_pos = a.j; an.len = a.len; an.delta = a.delta; an.left_ops = left_ops;
    an.flags = a.flags | soft_flags;
    return an;
}
