// compact_rows.h -- what the stages that make a second, compact batch on the device share (split_kernels.hip: the clipped
// ends; secondary_kernels.hip: the candidates of a secondary alignment): the workgroup step of the count / scan / mark order
// and the realigned 16-byte load of the row gather (device code only).  Past one workgroup, one scan tile and one chunk both
// stages are pinned by tests/test_gpu_compact_rows.py on the inputs of tests/compact_cases.py (tests/test_compact_cases_cpu.py
// ties those inputs to the host plans)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SP_BLOCK 256                          // reads per workgroup of the count / mark kernels
#define SP_CHUNK 4096                         // bytes of a row one workgroup of a gather kernel moves

// sum and maximum over the workgroup's 4 wavefronts; `before`: the sum of the wavefronts below this one
__device__ __forceinline__ void sp_block_totals(uint32_t wave_sum, uint32_t wave_max, uint32_t *s_sum, uint32_t *s_max,
                                                uint32_t *before, uint32_t *all, uint32_t *longest) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 63) { s_sum[wave] = wave_sum; s_max[wave] = wave_max; }
    __syncthreads();
    uint32_t b = 0, a = 0, m = 0;
#pragma unroll
    for (uint32_t w = 0; w < SP_BLOCK / 64; ++w) {
        const uint32_t t = s_sum[w];
        a += t;
        b += w < wave ? t : 0u;
        m = max(m, s_max[w]);
    }
    *before = b; *all = a; *longest = m;
}

// the bytes src[0 .. cnt), cnt in 1 .. 16, as two 64-bit words (o0: bytes 0 .. 7); src at any byte: the lane loads the two
// aligned 16-byte words that hold its bytes -- the second only when its bytes reach into it -- and realigns them in registers
// (one 64-bit select for the word offset, one funnel shift for the byte offset).  Bytes from cnt on are whatever follows.
__device__ __forceinline__ void sp_load16(const char *src, uint32_t cnt, uint64_t &o0, uint64_t &o1) {
    const uint32_t off = (uint32_t) ((uintptr_t) src & 15u);
    const uint4 *a = reinterpret_cast<const uint4 *>(src - off);
    const uint4 lo = a[0];
    const uint4 hi = off + cnt > 16 ? a[1] : make_uint4(0, 0, 0, 0);       // only when the lane's bytes reach into it
    uint64_t w0 = lo.x | ((uint64_t) lo.y << 32), w1 = lo.z | ((uint64_t) lo.w << 32);
    uint64_t w2 = hi.x | ((uint64_t) hi.y << 32);
    const uint64_t w3 = hi.z | ((uint64_t) hi.w << 32);
    if (off & 8u) { w0 = w1; w1 = w2; w2 = w3; }
    const uint32_t sh = (off & 7u) * 8;
    o0 = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
    o1 = sh ? (w1 >> sh) | (w2 << (64 - sh)) : w1;
}
// zeros from byte cnt on (cnt < 16)
__device__ __forceinline__ void sp_keep_bytes(uint32_t cnt, uint64_t &o0, uint64_t &o1) {
    o0 &= cnt >= 8 ? ~0ull : (1ull << (8 * cnt)) - 1;
    o1 &= cnt > 8 ? (1ull << (8 * (cnt - 8))) - 1 : 0ull;
}
