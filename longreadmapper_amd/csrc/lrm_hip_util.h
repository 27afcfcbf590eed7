// lrm_hip_util.h -- host helpers shared by the .hip files of liblrm_accel.so (lrm_internal.h is also read by plain C++)
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
