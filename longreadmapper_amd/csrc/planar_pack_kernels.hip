// planar_pack_kernels.hip -- bit-planar images of reads and text: 32 bases = {low code bits, high code bits} in one 64-bit
// word (A 0, C 1, T 2, G 3).  Read by the bit-sliced extension kernel (gact_bs_kernels.hip) and by the anchor scan
// (anchor_kernels.hip).
//
//   bs_pack_reads    the reads of a batch or a job table into an LrmBsScratch, with per-read "holds a byte other than ACGT" flags
//   bs_pack_content  a text; the index handle owns the planar copy of its text (lrm_bs_prepare_index)
#include <hip/hip_runtime.h>
#include "lrm_hip_util.h"
#include "extend_stage.h"
#include "base_words.h"

#define BS_PADW LRM_BS_PADW

// ----------------------------------------------------------------------------------------
// planar packing: one lane per base, the two code bits of 64 bases are two ballots
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ void bs_pack_group(const uint8_t *src, uint64_t len, uint64_t g, int lane,
                                              uint64_t *out, uint32_t *flag) {
    const uint64_t p = g * 64 + (uint64_t) lane;
    const uint32_t c = p < len ? src[p] : (uint32_t) 'A';          // bases past the end pack as A, unflagged
    const uint32_t code = ((c >> 1) ^ (c >> 2)) & 3u;                      // A 0, C 1, T 2, G 3 (any bijection works)
    const bool bad = !(c == 'A' || c == 'C' || c == 'G' || c == 'T');     // bytes compare by equality in the spec:
    const uint64_t lo = __ballot(code & 1u), hi = __ballot(code >> 1);    // anything else goes to the byte kernels
    const uint64_t nb = __ballot(bad);
    if (lane == 0) {
        out[2 * g] = (lo & 0xffffffffull) | (hi << 32);
        out[2 * g + 1] = (lo >> 32) | (hi & 0xffffffff00000000ull);
        if (nb && flag) atomicOr(flag, 1u);
    }
}

// reads: word w of read r at out + r*wpr + BS_PADW + w; padding words are zeroed.
// One wavefront per BS_PACK_G groups of 64 bases (1 KiB of a read): every lane takes 16 bases with two ALIGNED
// 16-byte loads (rows start at any byte: stride = max_read_len + 1) and v_alignbyte, turns them into 16 low and 16
// high plane bits with multiplies (no ballots), and pairs of lanes assemble the 64-bit words.  (The first version
// loaded one byte per lane and built the planes with 48 ballots per KiB: 0.72 ms per Gbp [r2].)
#define BS_PACK_G 16
// the per-byte test that not_acgt4 (base_words.h) replaced in the kernel below: ~(A | C | G | T matches) & 0x80808080
__device__ __forceinline__ uint32_t bs_bytes_equal(uint32_t x, uint32_t c4) {    // 0x80 in every byte of x equal to c4's
    const uint32_t z = x ^ c4;
    return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu);
}
__global__ __launch_bounds__(256) void bs_pack_reads_kernel(const char *__restrict__ reads, uint64_t stride,
                                                            const uint32_t *__restrict__ lens,
                                                            uint64_t *__restrict__ out, uint64_t wpr,
                                                            uint32_t *__restrict__ flags, uint64_t n,
                                                            uint32_t groups_per_read, uint32_t waves_per_read) {
    const uint64_t wave_id = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint64_t r = wave_id / waves_per_read;
    const uint32_t part = (uint32_t) (wave_id % waves_per_read);
    if (r >= n) return;
    const uint32_t len = lens[r];
    uint64_t *o = out + r * wpr;
    if (part == 0) {
        for (uint64_t w = lane; w < BS_PADW; w += 64) o[w] = 0;
        for (uint64_t w = BS_PADW + 2ull * groups_per_read + lane; w < wpr; w += 64) o[w] = 0;
    }
    const uint8_t *row = reinterpret_cast<const uint8_t *>(reads) + r * stride;
    const uint32_t g0 = part * BS_PACK_G;
    const uint32_t p0 = g0 * 64 + 16 * (uint32_t) lane;               // this lane's 16 bases: [p0, p0 + 16)
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t *src = row + p0;
    const uint32_t sh = (uint32_t) ((uintptr_t) src & 15u);           // the same in every lane of the wavefront
    if (p0 < len) {                                                   // both loads touch a 16-byte line that holds a base of the read
        const uint4 q0 = *reinterpret_cast<const uint4 *>(src - sh);
        d[0] = q0.x; d[1] = q0.y; d[2] = q0.z; d[3] = q0.w;
        if (sh && p0 + (16 - sh) < len) {
            const uint4 q1 = *reinterpret_cast<const uint4 *>(src - sh + 16);
            d[4] = q1.x; d[5] = q1.y; d[6] = q1.z; d[7] = q1.w;
        }
    }
    const uint32_t ws = sh >> 2, bs = sh & 3;                          // dword and byte part of the shift (wave-uniform)
    uint32_t lo = 0, hi = 0, bad = 0, xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t a_ = d[k], b_ = d[k + 1];
        if (ws == 1) { a_ = d[k + 1]; b_ = d[k + 2]; }
        else if (ws == 2) { a_ = d[k + 2]; b_ = d[k + 3]; }
        else if (ws == 3) { a_ = d[k + 3]; b_ = d[k + 4]; }
        xs[k] = __builtin_amdgcn_alignbyte(b_, a_, bs);                // bases p0 + 4k .. p0 + 4k + 3
    }
    if (p0 + 16 > len) {                                               // only the lanes at and past the read's end
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pk = p0 + 4 * (uint32_t) k;
            const uint32_t keep = bw_keep(len > pk ? len - pk : 0u);   // bases of this dword inside the read
            xs[k] = (xs[k] & keep) | (0x41414141u & ~keep);            // bases past the end pack as A, unflagged
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x = xs[k];
        const uint32_t code = codes4(x);
        lo |= ((((code & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (4 * k);
        hi |= (((((code >> 1) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (4 * k);
        bad |= not_acgt4(x);                                           // by the codes already made, a permute and an xor
    }
    const uint32_t mine = lo | (hi << 16);
    const uint32_t other = (uint32_t) __shfl_xor((int) mine, 1);
    if (!(lane & 1) && g0 + (uint32_t) (lane >> 2) < groups_per_read) {
        // word (lane >> 1) of the wavefront's 32: low planes of 32 bases in the low half, high planes in the high half
        const uint64_t w = (uint64_t) (mine & 0xFFFFu) | ((uint64_t) (other & 0xFFFFu) << 16) |
                           ((uint64_t) (mine >> 16) << 32) | ((uint64_t) (other >> 16) << 48);
        o[BS_PADW + 2ull * g0 + (uint32_t) (lane >> 1)] = w;
    }
    if (__ballot(bad != 0) && lane == 0) atomicOr(flags + r, 1u);
}

// reference text: one wavefront per 64 KiB
__global__ __launch_bounds__(256) void bs_pack_content_kernel(const char *__restrict__ content, uint64_t len,
                                                              uint64_t *__restrict__ out, uint64_t groups,
                                                              uint32_t *__restrict__ flag) {
    const uint64_t wave_id = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint64_t g0 = wave_id * 1024;
    for (uint64_t g = g0; g < g0 + 1024 && g < groups; ++g)
        bs_pack_group(reinterpret_cast<const uint8_t *>(content), len, g, lane, out, flag);
}

// ----------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------
uint64_t lrm_bs_planar_words(uint64_t len) { return 2 * ((len + 63) / 64) + 2 * (uint64_t) BS_PADW; }

// planar text into a caller-provided buffer of lrm_bs_planar_words(len) words (+ a flag word)
int lrm_bs_pack_text(const char *d_text, uint64_t len, uint64_t *d_out, uint32_t *d_flag, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const uint64_t words = lrm_bs_planar_words(len), groups = (len + 63) / 64;
    HIPCHK(hipMemsetAsync(d_out, 0, words * 8, stream));
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, stream));
    if (groups == 0) return 0;
    const uint64_t waves = (groups + 1023) / 1024;
    hipLaunchKernelGGL(bs_pack_content_kernel, dim3((uint32_t) ((waves + 3) / 4)), dim3(256), 0, stream, d_text, len,
                       d_out + BS_PADW, groups, d_flag);
    HIPCHK(hipGetLastError());
    return 0;
}

// planar copy of the reference text, owned by the index handle (device memory, +25 % of the text)
int lrm_bs_prepare_index(lrm_index *idx) {
    idx->d_cpl = nullptr;
    idx->cpl_ok = 0;
    // the text ends with the FM terminator (accaln.c: content length == fmi length); no window reaches it
    const uint64_t len = idx->view.con_len > 0 ? idx->view.con_len - 1 : 0;
    if (len == 0) return 0;
    const uint64_t words = lrm_bs_planar_words(len);
    uint64_t *d = nullptr;
    uint32_t *flag = nullptr;
    uint32_t h = 0;
    const bool ok = hipMalloc(&d, words * 8 + 16) == hipSuccess && hipMalloc(&flag, 16) == hipSuccess &&
                    lrm_bs_pack_text(idx->view.content, len, d, flag, nullptr) == 0 &&
                    hipMemcpy(&h, flag, 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (flag) (void) hipFree(flag);
    if (!ok) {                                   // nothing leaks on a failed allocation / pack / copy
        if (d) (void) hipFree(d);
        lrm_set_error("planar text for the bit-sliced extension: %s", hipGetErrorString(hipGetLastError()));
        return -1;
    }
    idx->d_cpl = d;
    idx->cpl_ok = h == 0;          // a text with bytes other than ACGT keeps the byte kernels
    return 0;
}

void lrm_bs_free_index(lrm_index *idx) {
    if (idx->d_cpl) (void) hipFree(idx->d_cpl);
    idx->d_cpl = nullptr;
}

// planar reads + per-read "has a byte other than ACGT" flags into the scratch
int lrm_bs_pack_reads(const char *d_reads, uint64_t stride, const uint32_t *d_lens, uint64_t n, uint32_t max_len,
                      const LrmBsScratch &bs, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const uint32_t gpr = (max_len + 63) / 64;
    uint32_t wv = (gpr + BS_PACK_G - 1) / BS_PACK_G;   // 16 groups (1 KiB of read) per wavefront
    if (wv == 0) wv = 1;
    uint32_t grid;
    if (lrm_grid_1d((n * wv + 3) / 4, "planar pack", &grid)) return -1;
    HIPCHK(hipMemsetAsync(bs.rflags, 0, n * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(bs_pack_reads_kernel, dim3(grid), dim3(256), 0, stream, d_reads, stride, d_lens, bs.qpl, bs.wpr,
                       bs.rflags, n, gpr, wv);
    return 0;
}
