// result_pack_kernels.hip -- the dense result image of a unit of the host pipeline (host_pipeline.hip): the used part of
// every CIGAR row (or its run-length text) and the reverse-complemented reads, packed on the device so that they cross the
// link as contiguous DMA pieces.
#include <hip/hip_runtime.h>
#include "lrm_hip_util.h"
#include "op_rows.h"                      // op_row_absent

namespace {

// pack kernel: row i of a pitched device array (len[i] bytes; 0 = skip) -> dense[off[i] ..), 16 bytes per lane.
// Rows start at any byte (the hardware takes the unaligned dwords); dense offsets are 16-byte aligned.
__global__ __launch_bounds__(256) void pack_rows_kernel(const uint8_t *__restrict__ src, uint64_t pitch,
                                                        const uint32_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                        uint8_t *__restrict__ dense, uint64_t rows) {
    const uint64_t row = blockIdx.x;
    if (row >= rows) return;
    const uint32_t l = len[row];
    const uint8_t *s = src + row * pitch;
    uint8_t *d = dense + off[row];
    for (uint32_t o = (blockIdx.y * 256 + threadIdx.x) * 16; o < l; o += gridDim.y * 256 * 16) {
        uint32_t w[4] = {0, 0, 0, 0};
        if (o + 16 <= l) __builtin_memcpy(w, s + o, 16);
        else for (uint32_t e = 0; o + e < l; ++e) w[e >> 2] |= (uint32_t) s[o + e] << (8 * (e & 3));
        *reinterpret_cast<uint4 *>(d + o) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// Run-length CIGAR text on the device (what parse_cigar prints, alnmain.c:497-498: '=' and 'X' columns as M): one
// workgroup per read walks the op bytes 4096 columns at a time; a run is printed where it ENDS, its start comes from a
// prefix maximum of the run starts, its place in the text from a prefix sum of the bytes the earlier runs print.
// WRITE = false: only the text length (tlen[row]); WRITE = true: the text at dense + off[row], NUL-terminated.
// Reads without an alignment (no ops, locus outside every sequence, score -1) print "*".
__device__ __forceinline__ uint32_t op_class(uint32_t b) { return (b == '=' || b == 'X') ? (uint32_t) 'M' : b; }
__host__ __device__ constexpr uint32_t dec_digits(uint32_t v) {
    return v < 10 ? 1u : v < 100 ? 2u : v < 1000 ? 3u : v < 10000 ? 4u : v < 100000 ? 5u : v < 1000000 ? 6u : v < 10000000 ? 7u :
           v < 100000000 ? 8u : v < 1000000000 ? 9u : 10u;
}
// no read the tests can afford has a run of 10^7 ops: the ladder is pinned here, at every power of ten a uint32_t holds
constexpr bool dec_digits_ok() {
    uint64_t p = 10;
    for (uint32_t k = 1; k <= 9; ++k, p *= 10)
        if (dec_digits((uint32_t) (p - 1)) != k || dec_digits((uint32_t) p) != k + 1) return false;
    return dec_digits(0) == 1 && dec_digits(0xFFFFFFFFu) == 10;
}
static_assert(dec_digits_ok(), "dec_digits: one digit per power of ten");
template <bool IS_MAX>
__device__ __forceinline__ int block_excl_scan(int v, int *s_w, int *total) {       // exclusive scan over 256 threads (max with -1 / sum with 0)
    const int lane = (int) (threadIdx.x & 63u), wave = (int) (threadIdx.x >> 6);
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x = IS_MAX ? (y > x ? y : x) : x + y;
    }
    __syncthreads();                                               // s_w of the previous scan has been read
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    int before = IS_MAX ? -1 : 0, all = IS_MAX ? -1 : 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int t = s_w[w];
        all = IS_MAX ? (t > all ? t : all) : all + t;
        if (w < wave) before = IS_MAX ? (t > before ? t : before) : before + t;
    }
    int excl = __shfl_up(x, 1, 64);
    if (lane == 0) excl = IS_MAX ? -1 : 0;
    *total = all;
    return IS_MAX ? (excl > before ? excl : before) : excl + before;
}
template <bool WRITE>
__global__ __launch_bounds__(256) void cigar_text_kernel(const uint8_t *__restrict__ store, uint64_t pitch, const int32_t *__restrict__ n_ops,
                                                         const int32_t *__restrict__ score, const int32_t *__restrict__ meta_r,
                                                         uint32_t *__restrict__ tlen, const uint64_t *__restrict__ off,
                                                         uint8_t *__restrict__ dense, uint64_t rows) {
    __shared__ int s_w[4];
    const uint64_t row = blockIdx.x;
    if (row >= rows) return;
    const int n = n_ops[row];
    const bool none = op_row_absent(n, meta_r, score, row);
    uint8_t *out = WRITE ? dense + off[row] : nullptr;
    if (none) {
        if (threadIdx.x == 0) { if (WRITE) { out[0] = '*'; out[1] = 0; } else tlen[row] = 1; }
        return;
    }
    const uint8_t *ops = store + row * pitch;
    int carry_start = 0, carry_out = 0;
    for (int base = 0; base < n; base += 4096) {
        const int c0 = base + (int) threadIdx.x * 16;
        uint32_t cl[18];                                           // classes of columns c0 - 1 .. c0 + 16 (0 = outside the read)
#pragma unroll
        for (int k = 0; k < 18; ++k) {
            const int col = c0 - 1 + k;
            cl[k] = col >= 0 && col < n ? op_class(ops[col]) : 0u;
        }
        int last_start = -1;
#pragma unroll
        for (int k = 0; k < 16; ++k) if (c0 + k < n && cl[k + 1] != cl[k]) last_start = c0 + k;
        int any_start;
        const int before = block_excl_scan<true>(last_start, s_w, &any_start);
        const int open = before >= 0 ? before : carry_start;       // start of the run that is open at my first column
        int bytes = 0, cs = open;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int col = c0 + k;
            if (col < n) {
                if (cl[k + 1] != cl[k]) cs = col;
                if (cl[k + 2] != cl[k + 1]) bytes += (int) dec_digits((uint32_t) (col - cs + 1)) + 1;
            }
        }
        int chunk_bytes;
        int o = carry_out + block_excl_scan<false>(bytes, s_w, &chunk_bytes);
        if (WRITE) {
            cs = open;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int col = c0 + k;
                if (col < n) {
                    if (cl[k + 1] != cl[k]) cs = col;
                    if (cl[k + 2] != cl[k + 1]) {
                        uint32_t len = (uint32_t) (col - cs + 1);
                        const int nd = (int) dec_digits(len);
                        for (int d = nd - 1; d >= 0; --d) { out[o + d] = (uint8_t) ('0' + len % 10u); len /= 10u; }
                        out[o + nd] = (uint8_t) cl[k + 1];
                        o += nd + 1;
                    }
                }
            }
        }
        carry_out += chunk_bytes;
        if (any_start >= 0) carry_start = any_start;
    }
    if (threadIdx.x == 0) { if (WRITE) out[carry_out] = 0; else tlen[row] = (uint32_t) carry_out; }
}

}  // namespace

// rows of up to row_cap bytes (sizes the y extent of the grid: 4096 bytes per workgroup and pass)
int lrm_launch_pack_rows(const uint8_t *d_src, uint64_t pitch, uint64_t row_cap, const uint32_t *d_len, const uint64_t *d_off,
                         uint8_t *d_dense, uint64_t rows, void *stream) {
    const uint32_t gy = (uint32_t) ((row_cap + 4095) / 4096);
    hipLaunchKernelGGL(pack_rows_kernel, dim3((uint32_t) rows, gy ? gy : 1), dim3(256), 0, (hipStream_t) stream, d_src, pitch, d_len, d_off, d_dense, rows);
    HIPCHK(hipGetLastError());
    return 0;
}

// d_dense == null: the text lengths into d_tlen; else the texts at d_dense + d_off[row]
int lrm_launch_cigar_text(const uint8_t *d_store, uint64_t pitch, const int32_t *d_n_ops, const int32_t *d_score, const int32_t *d_meta_r,
                          uint32_t *d_tlen, const uint64_t *d_off, uint8_t *d_dense, uint64_t rows, void *stream) {
    if (d_dense) hipLaunchKernelGGL(cigar_text_kernel<true>, dim3((uint32_t) rows), dim3(256), 0, (hipStream_t) stream, d_store, pitch, d_n_ops, d_score, d_meta_r, (uint32_t *) nullptr, d_off, d_dense, rows);
    else hipLaunchKernelGGL(cigar_text_kernel<false>, dim3((uint32_t) rows), dim3(256), 0, (hipStream_t) stream, d_store, pitch, d_n_ops, d_score, d_meta_r, d_tlen, (const uint64_t *) nullptr, (uint8_t *) nullptr, rows);
    HIPCHK(hipGetLastError());
    return 0;
}
