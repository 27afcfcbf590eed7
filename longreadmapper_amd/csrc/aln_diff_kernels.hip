// aln_diff_kernels.hip -- the difference events (docs/GACT_SPEC.md, "Difference events and MD:Z"): one 32-bit word per 'X' or
// 'D' column of an alignment -- the reference base, the kind, the '=' columns before it -- made over the op bytes while they
// are still in HBM, packed per read at the offsets the alignment summary records give (n_x + n_del events per read).  A
// stream like aln_summary_kernels.hip: one byte of ops and one byte of text read per column, four bytes written per event.
#include <hip/hip_runtime.h>
#include "aln_diff_step.h"

namespace {

// (the loads are op_rows.h's row loads: the op bytes by 32-bit columns; the text -- 16 target bytes from a position on,
//  nothing at or behind content + con_len -- by 64-bit positions)
// what a wavefront carries from step to step of its row, all uniform: the target-consuming and the '=' columns so far, and
// the last op byte of the previous step (0 before column 0)
struct RowState { uint32_t t = 0, e = 0, carry = 0; };

// One step: the lane's 16 columns (zeros from column n on).  The packed scan of the lane's target-consuming and its '='
// columns gives the lane's target offset, its e and -- events are the target columns that are not '=' -- its event
// position.  The lane's at most 16 target bytes are contiguous: one unaligned 16-byte read, every event's byte picked out
// of the four registers.
__device__ __forceinline__ void diff_step(RowState &r, const uint4 cur, const uint8_t *__restrict__ content, uint64_t con_len, uint64_t loc,
                                          uint32_t *__restrict__ ev, uint32_t room) {
    const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
    uint32_t prev = op_prev_byte(r.carry, w[3]);
    OpMasks m[4];
    uint32_t tc = 0, ec = 0, any = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        m[k] = op_masks(w[k], (w[k] << 8) | prev);
        prev = w[k] >> 24;
        tc += (uint32_t) __popc(m[k].eq | m[k].x | m[k].d);
        ec += (uint32_t) __popc(m[k].eq);
        any |= m[k].x | m[k].d;
    }
    uint32_t t_lane, e_lane;
    op_scan_pair(tc, ec, r.t, r.e, t_lane, e_lane);
    if (!any) return;
    const uint4 text = row_load_last_step<uint64_t>(content, loc + t_lane, con_len);
    uint32_t pos = t_lane - e_lane, t = 0, e = e_lane;               // events of the row before this lane's
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        diff_word_step(m[k], t, e, text.x, text.y, text.z, text.w, [&](uint32_t word) {
            if (pos < room) ev[pos] = word;                          // (a caller's offsets that disagree with the ops write nothing outside the read's range)
            ++pos;
        });
}

// One wavefront per read, four per workgroup; no LDS, no barrier: the walk of op_rows.h.  A read without an alignment, and a
// read whose events end behind `cap`, write nothing.
__global__ __launch_bounds__(256) void aln_diff_kernel(const uint8_t *__restrict__ store, uint64_t pitch, const int32_t *__restrict__ n_ops,
                                                       const int32_t *__restrict__ score, const int32_t *__restrict__ meta_r,
                                                       const lrm_seq_meta *__restrict__ meta, const uint8_t *__restrict__ content, uint64_t con_len,
                                                       uint64_t rows, const uint64_t *__restrict__ off, uint64_t cap, uint32_t *__restrict__ events) {
    uint64_t row; uint32_t lane;
    if (!op_row_of_wave(rows, row, lane)) return;
    const int nn = n_ops[row];
    if (op_row_absent(nn, meta_r, score, row)) return;
    const uint64_t lo = off[row], hi = off[row + 1];
    if (hi > cap || hi <= lo) return;
    const uint64_t span = hi - lo;
    const uint32_t room = span > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) span;
    const uint64_t loc = meta[row].loc;
    uint32_t *ev = events + lo;
    RowState r;
    op_row_walk(store + row * pitch, (uint32_t) nn, lane, [&](const uint4 cur, uint32_t) { diff_step(r, cur, content, con_len, loc, ev, room); });
}

// exclusive prefix sums of n_x + n_del over the records, 64-bit; off[i + 1]: the sum up to and with record i
__global__ __launch_bounds__(1024) void aln_diff_offsets_kernel(const lrm_aln_summary *__restrict__ sum, uint64_t n, uint64_t *__restrict__ off) {
    if (threadIdx.x == 0) off[0] = 0;
    block1024_excl_scan<uint64_t>(n, [&](uint64_t i) { return (uint64_t) sum[i].n_x + (uint64_t) sum[i].n_del; },
                                  [&](uint64_t i, uint64_t excl, uint64_t mine) { off[i + 1] = excl + mine; });
}

}  // namespace

int lrm_launch_aln_diff(const LrmOpRows &b, const char *d_content, uint64_t con_len, const uint64_t *d_off, uint64_t cap, uint32_t *d_events,
                        void *stream) {
    if (b.rows == 0) return 0;
    uint32_t grid;
    if (op_rows_grid(b.rows, "difference events", &grid)) return -1;
    hipLaunchKernelGGL(aln_diff_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, b.store, b.pitch, b.n_ops, b.score, b.meta_r, b.meta,
                       (const uint8_t *) d_content, con_len, b.rows, d_off, cap, d_events);
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_aln_diff_offsets(const lrm_aln_summary *d_sum, uint64_t rows, uint64_t *d_off, void *stream) {
    hipLaunchKernelGGL(aln_diff_offsets_kernel, dim3(1), dim3(1024), 0, (hipStream_t) stream, d_sum, rows, d_off);
    HIPCHK(hipGetLastError());
    return 0;
}
