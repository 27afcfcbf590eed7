// aln_diff_kernels.hip -- the difference events (docs/GACT_SPEC.md, "Difference events and MD:Z"): one 32-bit word per 'X' or
// 'D' column of an alignment -- the reference base, the kind, the '=' columns before it -- made over the op bytes while they
// are still in HBM, packed per read at the offsets the alignment summary records give (n_x + n_del events per read).  A
// stream like aln_summary_kernels.hip: one byte of ops and one byte of text read per column, four bytes written per event.
#include <hip/hip_runtime.h>
#include "lrm_hip_util.h"
#include "aln_diff_step.h"

namespace {

// (the loads are lrm_hip_util.h's row loads: the op bytes by 32-bit columns; the text -- 16 target bytes from a position on,
//  nothing at or behind content + con_len -- by 64-bit positions)

// what a wavefront carries from step to step of its row, all uniform: the target-consuming and the '=' columns so far, and
// the last op byte of the previous step (0 before column 0)
struct RowState { uint32_t t = 0, e = 0, carry = 0; };

// One step: the lane's 16 columns (zeros from column n on).  The lane's count of target-consuming columns and its count of
// '=' columns share one word, so ONE inclusive scan gives the lane's target offset, its e and -- events are the target
// columns that are not '=' -- its event position.  The lane's at most 16 target bytes are contiguous: one unaligned 16-byte
// read, every event's byte picked out of the four registers.  The previous column of a lane's first byte comes over the DPP
// network (wave_shr:1), as in count_step of the summary kernel.
__device__ __forceinline__ void diff_step(RowState &r, const uint4 cur, const uint8_t *__restrict__ content, uint64_t con_len, uint64_t loc,
                                          uint32_t *__restrict__ ev, uint32_t room) {
    const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
    const uint32_t mine = w[3] >> 24;
    uint32_t prev = (uint32_t) __builtin_amdgcn_update_dpp((int) r.carry, (int) mine, 0x138, 0xf, 0xf, false);   // wave_shr:1; lane 0 keeps the carry
    r.carry = (uint32_t) __builtin_amdgcn_readlane((int) mine, 63);
    DiffMasks m[4];
    uint32_t tc = 0, ec = 0, any = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        m[k] = diff_masks(w[k], (w[k] << 8) | prev);
        prev = w[k] >> 24;
        tc += (uint32_t) __popc(m[k].eq | m[k].x | m[k].d);
        ec += (uint32_t) __popc(m[k].eq);
        any |= m[k].x | m[k].d;
    }
    const uint32_t mine2 = tc | (ec << 16);                          // at most 1024 each in a step: the halves never meet
    const uint32_t incl = wave_incl_scan(mine2), excl = incl - mine2;
    const uint32_t t_lane = r.t + (excl & 0xFFFFu), e_lane = r.e + (excl >> 16);
    const uint32_t total = (uint32_t) __builtin_amdgcn_readlane((int) incl, 63);
    r.t += total & 0xFFFFu;
    r.e += total >> 16;
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

// One wavefront per read, four per workgroup; no LDS, no barrier.  As in the summary kernel two steps are asked for together
// wherever both lie whole inside the row, and the end of a row goes through the masked loads.  A read without an alignment,
// and a read whose events end behind `cap`, write nothing.
__global__ __launch_bounds__(256) void aln_diff_kernel(const uint8_t *__restrict__ store, uint64_t pitch, const int32_t *__restrict__ n_ops,
                                                       const int32_t *__restrict__ score, const int32_t *__restrict__ meta_r,
                                                       const lrm_seq_meta *__restrict__ meta, const uint8_t *__restrict__ content, uint64_t con_len,
                                                       uint64_t rows, const uint64_t *__restrict__ off, uint64_t cap, uint32_t *__restrict__ events) {
    const uint64_t row = (uint64_t) blockIdx.x * 4u + (uint64_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    if (row >= rows) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int nn = n_ops[row];
    if (nn <= 0 || meta_r[row] == 0 || score[row] == -1) return;
    const uint64_t lo = off[row], hi = off[row + 1];
    if (hi > cap || hi <= lo) return;
    const uint64_t span = hi - lo;
    const uint32_t room = span > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) span;
    const uint32_t n = (uint32_t) nn;                                // (uniform: every branch on it is a scalar one)
    const uint8_t *ops = store + row * pitch;
    const uint64_t loc = meta[row].loc;
    uint32_t *ev = events + lo;
    RowState r;
    uint32_t base = 0;
    for (; base + 2048u <= n; base += 2048u) {                       // two steps whole inside the row: both loads in flight
        const uint32_t c0 = base + lane * 16u;
        const uint4 a = row_load_step<uint32_t>(ops, c0), b = row_load_step<uint32_t>(ops, c0 + 1024u);
        diff_step(r, a, content, con_len, loc, ev, room);
        diff_step(r, b, content, con_len, loc, ev, room);
    }
    for (; base < n; base += 1024u)
        diff_step(r, row_load_last_step<uint32_t>(ops, base + lane * 16u, n), content, con_len, loc, ev, room);
}

// exclusive prefix sums of n_x + n_del over the records, 64-bit: one workgroup of 1024 that loops over the records, a scan
// over the wavefront (shuffles), the 16 wavefront totals through LDS
__global__ __launch_bounds__(1024) void aln_diff_offsets_kernel(const lrm_aln_summary *__restrict__ sum, uint64_t n, uint64_t *__restrict__ off) {
    __shared__ uint64_t wave_total[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t running = 0;
    if (tid == 0) off[0] = 0;
    for (uint64_t base = 0; base < n; base += 1024u) {
        const uint64_t i = base + tid;
        uint64_t v = i < n ? (uint64_t) sum[i].n_x + (uint64_t) sum[i].n_del : 0ull;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t o = (uint64_t) __shfl_up((unsigned long long) v, d, 64);
            if (lane >= d) v += o;
        }
        if (lane == 63u) wave_total[wave] = v;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint64_t wt = wave_total[k];
            before += k < wave ? wt : 0ull;
            all += wt;
        }
        if (i < n) off[i + 1] = running + before + v;
        running += all;
        __syncthreads();                                             // wave_total is rewritten by the next round
    }
}

}  // namespace

int lrm_launch_aln_diff(const uint8_t *d_store, uint64_t pitch, const int32_t *d_n_ops, const int32_t *d_score, const int32_t *d_meta_r,
                        const lrm_seq_meta *d_meta, const char *d_content, uint64_t con_len, uint64_t rows, const uint64_t *d_off,
                        uint64_t cap, uint32_t *d_events, void *stream) {
    if (rows == 0) return 0;
    uint32_t grid;
    if (lrm_grid_1d((rows + 3) / 4, "difference events", &grid)) return -1;
    hipLaunchKernelGGL(aln_diff_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, d_store, pitch, d_n_ops, d_score, d_meta_r, d_meta,
                       (const uint8_t *) d_content, con_len, rows, d_off, cap, d_events);
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_aln_diff_offsets(const lrm_aln_summary *d_sum, uint64_t rows, uint64_t *d_off, void *stream) {
    hipLaunchKernelGGL(aln_diff_offsets_kernel, dim3(1), dim3(1024), 0, (hipStream_t) stream, d_sum, rows, d_off);
    HIPCHK(hipGetLastError());
    return 0;
}
