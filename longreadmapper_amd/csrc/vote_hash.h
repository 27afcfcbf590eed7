// SPDX-License-Identifier: MIT
// The hash of a vote bucket (bucket = key >> 4) and the two places the vote kernels (vote_kernels.hip) take from it besides
// the slot: the pass of a bucket in the multi-pass workgroup tier of the exact kernel, and its counter in the sketch of the
// fast kernels.  Like mapq_rule.h the file compiles for the device, for the host and as plain C, so
// tests/test_vote_block_cases_cpu.py says on the CPU in which pass and on which counter a constructed bucket lands.
#ifndef LRM_VOTE_HASH_H
#define LRM_VOTE_HASH_H
#include <stdint.h>

#if defined(__HIPCC__)
#define VH_FN __host__ __device__ __forceinline__
#else
#define VH_FN static inline
#endif

VH_FN uint32_t bucket_hash(uint64_t bucket) {
    uint32_t x = (uint32_t) bucket ^ (uint32_t) (bucket >> 29);
    x *= 0x9E3779B1u;
    x ^= x >> 15;
    return x * 0x85EBCA6Bu;
}

// the pass that admits the bucket with this hash, of `passes` > 1 (vote_admit)
VH_FN uint32_t bucket_pass(uint32_t hash, uint32_t passes) { return (hash >> 16) % passes; }

// the 16-bit sketch counter of the bucket with this hash; mask: counters - 1 (fast_hits)
VH_FN uint32_t sketch_counter(uint32_t hash, uint32_t mask) { return (hash >> 5) & mask; }

#endif
