// aln_summary_kernels.hip -- the alignment summary records (lrm_aln_summary; docs/GACT_SPEC.md, "Alignment summary and
// PAF"): what an alignment consists of, counted over its op bytes while they are still in HBM.  A pure stream: one byte
// read per column, 32 bytes written per read.
#include <hip/hip_runtime.h>
#include "op_rows.h"

namespace {

constexpr uint32_t TOPS = 0x80808080u;

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return (uint32_t) __builtin_amdgcn_readlane((int) wave_incl_scan(v), 63); }

// what a wavefront has counted so far in its row; `carry`: the last byte of the previous step (uniform), 0 before column 0
struct RowCounts {
    uint32_t eq = 0, x = 0, ins = 0, del = 0, ins_runs = 0, del_runs = 0;
    uint32_t first_inv = 0, last_end = 0;      // ~(first column that is not 'S') and 1 + the last such column; 0: none yet
    uint32_t carry = 0;
};
// One step: the lane's 16 columns from c0 on (zeros from column n on).  Per 32-bit word one exact byte mask per class and its
// popcount; a run starts where the mask has a column whose previous column is outside the mask -- the previous column of a
// word's first byte is the last byte of the lane's previous word, of a lane's first byte op_prev_byte's.
__device__ __forceinline__ void count_step(RowCounts &r, const uint4 cur, uint32_t c0, uint32_t n) {
    const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
    uint32_t prev = op_prev_byte(r.carry, w[3]);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t col = c0 + 4u * k;
        const OpMasks m = op_masks(w[k], (w[k] << 8) | prev);          // byte j of the second word: the column before byte j of w[k]
        prev = w[k] >> 24;
        r.eq += __popc(m.eq);
        r.x += __popc(m.x);
        r.ins += __popc(m.i);
        r.del += __popc(m.d);
        r.ins_runs += __popc(m.i_open);
        r.del_runs += __popc(m.d_open);
        // columns of this word inside the row that are not 'S' (a byte outside the alphabet is one)
        const uint32_t left = col < n ? n - col : 0u;
        const uint32_t inside = left >= 4u ? TOPS : TOPS & ((1u << (8u * left)) - 1u);
        const uint32_t other = inside & ~m.s;
        const uint32_t lo = col + ((uint32_t) __builtin_ctz(other | 0x80000000u) >> 3);      // (the guard bit only matters when other == 0)
        const uint32_t hi = col + ((31u - (uint32_t) __builtin_clz(other | 1u)) >> 3);
        const uint32_t lo_inv = other ? ~lo : 0u;
        r.first_inv = r.first_inv > lo_inv ? r.first_inv : lo_inv;
        r.last_end = other ? hi + 1u : r.last_end;                     // a lane's columns ascend
    }
}

// One wavefront per read, four per workgroup; no LDS, no barrier: the walk of op_rows.h.
__global__ __launch_bounds__(256) void aln_summary_kernel(const uint8_t *__restrict__ store, uint64_t pitch, const int32_t *__restrict__ n_ops,
                                                          const int32_t *__restrict__ score, const int32_t *__restrict__ meta_r,
                                                          uint64_t rows, lrm_aln_summary *__restrict__ out) {
    uint64_t row; uint32_t lane;
    if (!op_row_of_wave(rows, row, lane)) return;
    const int nn = n_ops[row];
    uint4 *rec = reinterpret_cast<uint4 *>(out + row);
    if (op_row_absent(nn, meta_r, score, row)) {
        if (lane == 0) { rec[0] = make_uint4(0, 0, 0, 0); rec[1] = make_uint4(0, 0, 0, 0); }
        return;
    }
    const uint32_t n = (uint32_t) nn;
    RowCounts r;
    op_row_walk(store + row * pitch, n, lane, [&](const uint4 cur, uint32_t c0) { count_step(r, cur, c0, n); });
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

int lrm_launch_aln_summary(const LrmOpRows &b, lrm_aln_summary *d_out, void *stream) {
    if (b.rows == 0) return 0;
    uint32_t grid;
    if (op_rows_grid(b.rows, "alignment summary", &grid)) return -1;
    hipLaunchKernelGGL(aln_summary_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, b.store, b.pitch, b.n_ops, b.score, b.meta_r, b.rows, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}
