// SPDX-License-Identifier: MIT
// C entry points over longreadmapper_amd/csrc/vote_hash.h for tests/vote_block_cases.py: the header is the source the vote
// kernels compile.  The tests ask it where a constructed bucket lands -- in which pass of the multi-pass tier, on which
// sketch counter -- to choose cases and to prove their predicates; no expected vote result comes from here.
#include "../../longreadmapper_amd/csrc/vote_hash.h"

void vh_hash(const uint64_t *bucket, int n, uint32_t *out) {
    for (int i = 0; i < n; ++i) out[i] = bucket_hash(bucket[i]);
}

void vh_pass(const uint64_t *bucket, int n, uint32_t passes, uint32_t *out) {
    for (int i = 0; i < n; ++i) out[i] = passes > 1 ? bucket_pass(bucket_hash(bucket[i]), passes) : 0u;
}

void vh_counter(const uint64_t *bucket, int n, uint32_t mask, uint32_t *out) {
    for (int i = 0; i < n; ++i) out[i] = sketch_counter(bucket_hash(bucket[i]), mask);
}
