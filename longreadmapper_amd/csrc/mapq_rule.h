// SPDX-License-Identifier: MIT
// Mapping quality (docs/GACT_SPEC.md, "Mapping quality"): the arithmetic of the rival-locus vote -- radius, window test,
// the two staggered histograms, the formula.  The file compiles for the device (mapq_kernels.hip), for the host
// (lrm_api.hip) and as plain C, so tests/test_mapq_cpu.py checks on the CPU the very source the kernel runs.
//
// Keys are the vote keys SA[row] - j with 64-bit wrap: SA < 2^39 (LRM_LOCATED_BIT) and j < 2^32, so a key lies in
// [0, 2^39) or, wrapped, in [2^64 - 2^32, 2^64).
#ifndef LRM_MAPQ_RULE_H
#define LRM_MAPQ_RULE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MQ_FN __host__ __device__ __forceinline__
#else
#define MQ_FN static inline
#endif

#define MQ_MIN_LOG2 9                // R = 512 up to reads of 4096 bases

// r = log2 R: 9 for len <= 4096, else ceil(log2 len) - 3 (R between len / 8 and len / 4)
MQ_FN uint32_t mq_radius_log2(uint32_t len) {
    uint32_t c = 0;                  // ceil(log2 len)
    while (c < 32 && (1ull << c) < (uint64_t) len) ++c;
    return c <= 12 ? MQ_MIN_LOG2 : c - 3;
}
MQ_FN uint32_t mq_radius(uint32_t len) { return 1u << mq_radius_log2(len); }

// |key - best| <= R on the signed difference of the wrapped values
MQ_FN int mq_inside(uint64_t key, uint64_t best, uint32_t r) {
    const uint64_t R = 1ull << r;
    return key - best + R <= 2 * R;
}

// bucket of a key in histogram h (0: key >> (r + 1); 1: (key + R) >> (r + 1)): width 2 R, staggered by R, so that a
// cluster at most R wide lies whole in one bucket of one of the two
MQ_FN uint64_t mq_bucket(uint64_t key, uint32_t r, uint32_t h) {
    return (key + (h ? 1ull << r : 0ull)) >> (r + 1);
}

// (histogram, bucket) as one 32-bit word of the LDS table.  r + 1 >= 10, so the bucket of a key in [0, 2^39) is below
// 2^29 (+ 1) and the low 31 bits of the bucket of a wrapped key lie in [2^31 - 2^22, 2^31): the low 31 bits identify the
// bucket, and no bucket has the low bits 2^30 -- that word marks an empty slot.
#define MQ_TAG_EMPTY 0x80000000u
MQ_FN uint32_t mq_tag(uint64_t key, uint32_t r, uint32_t h) {
    return ((uint32_t) mq_bucket(key, r, h) << 1) | (h & 1u);
}

// 60 * (n1 - min(n2, n1)) * min(n1, 10) / (10 * n1), integer division; 0 without support
MQ_FN uint32_t mq_value(uint32_t n1, uint32_t n2) {
    if (n1 == 0) return 0;
    const uint64_t lead = n1 - (n2 < n1 ? n2 : n1);
    const uint64_t cap = n1 < 10 ? n1 : 10;
    return (uint32_t) (60ull * lead * cap / (10ull * n1));
}

#endif
