// mapq_table.h -- the LDS of one read of the rival vote: the open-addressing table of (histogram, bucket) pairs and the
// per-wavefront staging lists, shared by mapq_vote_kernel (mapq_kernels.hip) and rival_locus_kernel (secondary_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include "mapq_rule.h"

#define MQ_U 4                              // SA gathers in flight per lane
#define MQ_WAVES 4

struct MqWaveLds {                          // repeat seeds of one chunk of 64 survivors
    uint64_t srec[64];
    uint32_t off[64 + 4];
    uint32_t sq[64];
};
struct MqLds {
    uint32_t tag[LRM_MAPQ_SLOTS];
    uint32_t count[LRM_MAPQ_SLOTS];
    MqWaveLds w[MQ_WAVES];
    uint32_t n1, overflow;
    uint32_t wmax[MQ_WAVES];
};
static_assert(sizeof(MqLds) <= 40 * 1024, "four workgroups per CU: 160 KiB of LDS");

// One hit into the rival table.  False only when the table holds `slots` other pairs already, i.e. when the read has more
// distinct pairs than slots -- whichever hit finds that out, some hit does (the outcome does not depend on the order).
__device__ __forceinline__ bool mq_insert(MqLds &L, uint32_t tag, uint32_t slots) {
    uint32_t slot = ((tag * 0x9E3779B1u) >> 7) & (slots - 1u);
    for (uint32_t probe = 0; probe < slots; ++probe) {
        const uint32_t prev = atomicCAS(&L.tag[slot], MQ_TAG_EMPTY, tag);
        if (prev == MQ_TAG_EMPTY || prev == tag) { atomicAdd(&L.count[slot], 1u); return true; }
        slot = (slot + 1u) & (slots - 1u);
    }
    return false;
}
