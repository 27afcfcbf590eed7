// aln_summary_kernels.hip -- the alignment summary records (lrm_aln_summary; docs/GACT_SPEC.md, "Alignment summary and
// PAF"): what an alignment consists of, counted over its op bytes while they are still in HBM.  A pure stream: one byte
// read per column, 32 bytes written per read.
#include <hip/hip_runtime.h>
#include "lrm_hip_util.h"
#include "aln_diff_step.h"

namespace {

constexpr uint32_t TOPS = 0x80808080u;

// the exact byte mask of both kernels over op bytes (aln_diff_step.h)
__device__ __forceinline__ uint32_t bytes_equal(uint32_t w, uint32_t c) { return diff_bytes_equal(w, c); }
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    return (uint32_t) __builtin_amdgcn_readlane((int) wave_incl_scan(v), 63);
}

// 16 op bytes of a row from column c0 on (lrm_hip_util.h): a step whole inside the row, and the row's last step
__device__ __forceinline__ uint4 load_step(const uint8_t *__restrict__ ops, uint32_t c0) { return row_load_step<uint32_t>(ops, c0); }
__device__ __forceinline__ uint4 load_last_step(const uint8_t *__restrict__ ops, uint32_t c0, uint32_t n) { return row_load_last_step<uint32_t>(ops, c0, n); }

// what a wavefront has counted so far in its row; `carry`: the last byte of the previous step (uniform), 0 before column 0
struct RowCounts {
    uint32_t eq = 0, x = 0, ins = 0, del = 0, ins_runs = 0, del_runs = 0;
    uint32_t first_inv = 0, last_end = 0;      // ~(first column that is not 'S') and 1 + the last such column; 0: none yet
    uint32_t carry = 0;
};
// One step: the lane's 16 columns from c0 on (zeros from column n on).  Per 32-bit word one exact byte mask per class and its
// popcount; a run starts where the mask has a column whose previous column is outside the mask -- the previous column of a
// word's first byte is the last byte of the lane's previous word, of a lane's first byte the last byte of the lane before
// it (DPP wave_shr:1), of a step's first byte the last byte of the previous step (a scalar), of column 0 "no op" (0).
__device__ __forceinline__ void count_step(RowCounts &r, const uint4 cur, uint32_t c0, uint32_t n) {
    const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
    const uint32_t mine = w[3] >> 24;
    uint32_t prev = (uint32_t) __builtin_amdgcn_update_dpp((int) r.carry, (int) mine, 0x138, 0xf, 0xf, false);   // wave_shr:1; lane 0 keeps the carry
    r.carry = (uint32_t) __builtin_amdgcn_readlane((int) mine, 63);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t col = c0 + 4u * k;
        const uint32_t cw = w[k], pw = (cw << 8) | prev;               // byte j of pw: the column before byte j of cw
        prev = cw >> 24;
        const uint32_t mi = bytes_equal(cw, 'I'), md = bytes_equal(cw, 'D');
        r.eq += __popc(bytes_equal(cw, '='));
        r.x += __popc(bytes_equal(cw, 'X'));
        r.ins += __popc(mi);
        r.del += __popc(md);
        r.ins_runs += __popc(mi & ~bytes_equal(pw, 'I'));
        r.del_runs += __popc(md & ~bytes_equal(pw, 'D'));
        // columns of this word inside the row that are not 'S' (a byte outside the alphabet is one)
        const uint32_t left = col < n ? n - col : 0u;
        const uint32_t inside = left >= 4u ? TOPS : TOPS & ((1u << (8u * left)) - 1u);
        const uint32_t other = inside & ~bytes_equal(cw, 'S');
        const uint32_t lo = col + ((uint32_t) __builtin_ctz(other | 0x80000000u) >> 3);      // (the guard bit only matters when other == 0)
        const uint32_t hi = col + ((31u - (uint32_t) __builtin_clz(other | 1u)) >> 3);
        const uint32_t lo_inv = other ? ~lo : 0u;
        r.first_inv = r.first_inv > lo_inv ? r.first_inv : lo_inv;
        r.last_end = other ? hi + 1u : r.last_end;                     // a lane's columns ascend
    }
}

// One wavefront per read, four per workgroup; no LDS, no barrier.  A step is 1 KiB of the row, 16 columns per lane; two
// steps are asked for together wherever both lie whole inside the row (one straight block: two 16-byte loads in flight per
// lane, the first step counted while the second is on its way), the end of a row goes through the masked loads.
__global__ __launch_bounds__(256) void aln_summary_kernel(const uint8_t *__restrict__ store, uint64_t pitch, const int32_t *__restrict__ n_ops,
                                                          const int32_t *__restrict__ score, const int32_t *__restrict__ meta_r,
                                                          uint64_t rows, lrm_aln_summary *__restrict__ out) {
    const uint64_t row = (uint64_t) blockIdx.x * 4u + (uint64_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    if (row >= rows) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int nn = n_ops[row];
    uint4 *rec = reinterpret_cast<uint4 *>(out + row);
    if (nn <= 0 || meta_r[row] == 0 || score[row] == -1) {           // the reads cigar_text_kernel prints as "*"
        if (lane == 0) { rec[0] = make_uint4(0, 0, 0, 0); rec[1] = make_uint4(0, 0, 0, 0); }
        return;
    }
    const uint32_t n = (uint32_t) nn;                                // (uniform: every branch on it is a scalar one)
    const uint8_t *ops = store + row * pitch;
    RowCounts r;
    uint32_t base = 0;
    for (; base + 2048u <= n; base += 2048u) {
        const uint32_t c0 = base + lane * 16u;
        const uint4 a = load_step(ops, c0), b = load_step(ops, c0 + 1024u);
        count_step(r, a, c0, n);
        count_step(r, b, c0 + 1024u, n);
    }
    for (; base < n; base += 1024u) {
        const uint32_t c0 = base + lane * 16u;
        count_step(r, load_last_step(ops, c0, n), c0, n);
    }
    const uint32_t s_eq = wave_sum_u32(r.eq), s_x = wave_sum_u32(r.x), s_i = wave_sum_u32(r.ins), s_d = wave_sum_u32(r.del);
    const uint32_t s_ri = wave_sum_u32(r.ins_runs), s_rd = wave_sum_u32(r.del_runs);
    const uint32_t f_inv = wave_max_u32(r.first_inv), l_end = wave_max_u32(r.last_end);
    if (lane == 0) {
        const uint32_t clip_left = l_end ? ~f_inv : n, clip_right = l_end ? n - l_end : 0u;    // a row of 'S' alone: all of it on the left
        rec[0] = make_uint4(s_eq, s_x, s_i, s_d);
        rec[1] = make_uint4(s_ri, s_rd, clip_left, clip_right);
    }
}

}  // namespace

int lrm_launch_aln_summary(const uint8_t *d_store, uint64_t pitch, const int32_t *d_n_ops, const int32_t *d_score, const int32_t *d_meta_r,
                           uint64_t rows, lrm_aln_summary *d_out, void *stream) {
    if (rows == 0) return 0;
    uint32_t grid;
    if (lrm_grid_1d((rows + 3) / 4, "alignment summary", &grid)) return -1;
    hipLaunchKernelGGL(aln_summary_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, d_store, pitch, d_n_ops, d_score, d_meta_r, rows, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}
