// lrm_hip_util.h -- host helpers and wavefront primitives shared by the .hip files of liblrm_accel.so (lrm_internal.h is also read by plain C++)
#pragma once
#include <hip/hip_runtime.h>
#include "lrm_internal.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    lrm_set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// device buffer owned by a guard (debug taps): an early HIPCHK return frees it
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void) hipFree(p); }
    int alloc(uint64_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess ? 0 : -1; }
};

// x extent of a one-dimensional grid of `blocks` workgroups
static inline int lrm_grid_1d(uint64_t blocks, const char *what, uint32_t *out) {
    if (blocks > 0x7fffffffull) { lrm_set_error("%s grid too large: split the batch", what); return -1; }
    *out = (uint32_t) blocks;
    return 0;
}

#if defined(__HIPCC__)
// ---- wavefront primitives on the DPP network (seed_kernels.hip, anchor_kernels.hip) ----
// inclusive prefix sum over the 64 lanes on the DPP network: four row shifts inside the rows of 16, then the
// row totals are broadcast to the following rows (row_bcast:15 / row_bcast:31) -- six v_add_u32_dpp, no LDS
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, false);      // row_shr:1
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, false);      // row_shr:2
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, false);      // row_shr:4
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, false);      // row_shr:8
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false);      // row_bcast:15 -> rows 1, 3
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false);      // row_bcast:31 -> rows 2, 3
    return v;
}

// max over the 64 lanes, returned in every lane: the prefix-max runs on the DPP network like wave_incl_scan (row
// shifts inside the rows of 16, then row_bcast:15 / row_bcast:31), lane 63 ends up with the maximum and two readlanes
// broadcast it.  (The first version was a butterfly of __shfl_xor: twelve ds_bpermute per reduction, a third of the
// LDS instructions of a small vote item.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp_max_step(uint64_t v) {
    const uint32_t lo = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) v, CTRL, ROW_MASK, 0xf, false);
    const uint32_t hi = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) (v >> 32), CTRL, ROW_MASK, 0xf, false);
    const uint64_t o = ((uint64_t) hi << 32) | lo;                 // 0 where the lane has no source: the identity of max
    return o > v ? o : v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    v = dpp_max_step<0x111, 0xf>(v);      // row_shr:1
    v = dpp_max_step<0x112, 0xf>(v);      // row_shr:2
    v = dpp_max_step<0x114, 0xf>(v);      // row_shr:4
    v = dpp_max_step<0x118, 0xf>(v);      // row_shr:8
    v = dpp_max_step<0x142, 0xa>(v);      // row_bcast:15 -> rows 1, 3
    v = dpp_max_step<0x143, 0xc>(v);      // row_bcast:31 -> rows 2, 3
    const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) v, 63);
    const uint32_t hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) (v >> 32), 63);
    return ((uint64_t) hi << 32) | lo;
}
#endif
