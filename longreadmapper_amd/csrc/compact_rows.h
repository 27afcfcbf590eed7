// compact_rows.h -- what the stages that make a second, compact batch on the device share (split_kernels.hip: the clipped
// ends; secondary_kernels.hip: the candidates of a secondary alignment).  A stage is a RULE -- how many rows a read
// contributes, how long they are, the records written at their place -- and everything else is here, once:
//
//   compact_count<Rule>  per workgroup of 256 reads: how many rows they have, and the longest
//   compact_scan         ONE workgroup: exclusive scan of those counts in place, the total and the longest row of the batch
//   (host)               the 8 bytes {total, longest} cross to pinned memory; the call sleeps on an event until they are there
//   (host)               the room check: table, row stride, store stride, workspace, gather grid
//   compact_mark<Rule>   one lane per read: the rule's records at the read's place in the order
//   compact_gather<Rule> row s of the compact batch: the source span the rule names, straight or mirrored, zeros behind it
//
// Order: a read's first row index is an exclusive prefix sum of the per-read counts -- wave_incl_scan on the DPP network
// inside a wavefront, the wavefront totals through LDS inside a workgroup, the workgroup totals through compact_scan.  No
// atomics: the table is the same whatever the scheduling, and it is the table the stage's plan computes on the host.
// The kernels that are no templates and the host steps are in compact_rows.hip.  Past one workgroup, one scan tile and one
// chunk both stages are pinned by tests/test_gpu_compact_rows.py on the inputs of tests/compact_cases.py
// (tests/test_compact_cases_cpu.py ties those inputs to the host plans)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lrm_hip_util.h"
#include "seq_bytes.h"

#define SP_BLOCK 256                          // reads per workgroup of the count / mark kernels
#define SP_CHUNK 4096                         // bytes of a row one workgroup of a gather kernel moves

// sum and maximum over the workgroup's 4 wavefronts; `before`: the sum of the wavefronts below this one;
// MAX = false: the sum alone, s_max is not touched
template <bool MAX = true>
__device__ __forceinline__ void sp_block_totals(uint32_t wave_sum, uint32_t wave_max, uint32_t *s_sum, uint32_t *s_max,
                                                uint32_t *before, uint32_t *all, uint32_t *longest) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 63) { s_sum[wave] = wave_sum; if (MAX) s_max[wave] = wave_max; }
    __syncthreads();
    uint32_t b = 0, a = 0, m = 0;
#pragma unroll
    for (uint32_t w = 0; w < SP_BLOCK / 64; ++w) {
        const uint32_t t = s_sum[w];
        a += t;
        b += w < wave ? t : 0u;
        if (MAX) m = max(m, s_max[w]);
    }
    *before = b; *all = a; *longest = m;
}

// A Rule is a small struct passed by value as the kernel argument:
//   typedef ... Item;                                    what items() hands to write()
//   uint32_t items(n, r, Item &item, uint32_t &longest)  rows of read r and the longest of them; 0 beyond the batch, and
//                                                        `longest` stays the 0 it comes with
//   void write(r, item, k, at, cap)                      the records of the read's k > 0 rows at `at`; none from `cap` on
// (and what the gather asks: below)
template <typename Rule>
__global__ __launch_bounds__(SP_BLOCK) void compact_count_kernel(Rule rule, uint64_t n, uint2 *__restrict__ blk) {
    __shared__ uint32_t s_sum[SP_BLOCK / 64], s_max[SP_BLOCK / 64];
    typename Rule::Item item;
    uint32_t longest = 0;
    const uint32_t k = rule.items(n, (uint64_t) blockIdx.x * SP_BLOCK + threadIdx.x, item, longest);
    const uint32_t incl = wave_incl_scan(k);
    const uint32_t wmax = (uint32_t) wave_max_u64(longest);
    uint32_t before, all, lmax;
    sp_block_totals(incl, wmax, s_sum, s_max, &before, &all, &lmax);
    if (threadIdx.x == 0) blk[blockIdx.x] = make_uint2(all, lmax);
}

template <typename Rule>
__global__ __launch_bounds__(SP_BLOCK) void compact_mark_kernel(Rule rule, uint64_t n, const uint2 *__restrict__ blk, uint64_t cap) {
    __shared__ uint32_t s_sum[SP_BLOCK / 64];
    const uint64_t r = (uint64_t) blockIdx.x * SP_BLOCK + threadIdx.x;
    typename Rule::Item item;
    uint32_t longest = 0;
    const uint32_t k = rule.items(n, r, item, longest);
    const uint32_t incl = wave_incl_scan(k);
    uint32_t before, all, lmax;
    sp_block_totals<false>(incl, 0, s_sum, nullptr, &before, &all, &lmax);
    if (k) rule.write(r, item, k, (uint64_t) blk[blockIdx.x].x + before + incl - k, cap);
}

// The gather: row s of the compact batch from the table the mark kernel wrote.  The rule adds
//   static constexpr bool MIRRORS                        can a source span be mirrored at all (false: the path is not compiled)
//   Span span(s)                                         {first byte, bases} of row s's source
//   bool mirrored(s)                                     (when MIRRORS) is the row the reverse complement of that span
//   static uint64_t zeros_to(len, row_stride)            the row byte before which the zeros behind the span end
// Grid (rows, chunks of SP_CHUNK row bytes); every lane one aligned 16-byte store, the source realigned in registers
// (seq_bytes.h: sp_row16, sp_row16_mirrored).
struct CompactSpan { const char *src; uint32_t len; };
template <typename Rule>
__global__ __launch_bounds__(256) void compact_gather_kernel(Rule rule, uint64_t n_rows, char *__restrict__ rows, uint64_t row_stride) {
    const uint64_t s = blockIdx.x;
    if (s >= n_rows) return;
    const uint64_t d = (uint64_t) blockIdx.y * SP_CHUNK + 16ull * threadIdx.x;
    if (d + 16 > row_stride) return;                                 // (row_stride > len and % 16 == 0: never cuts a row short)
    const CompactSpan sp = rule.span(s);
    if (d >= Rule::zeros_to(sp.len, row_stride)) return;
    uint4 o = make_uint4(0, 0, 0, 0);
    if (d < sp.len) {
        const uint32_t cnt = sp.len - d < 16 ? (uint32_t) (sp.len - d) : 16u;     // (below 16: the span's last word, zeros behind its end)
        bool mirrored = false;
        if constexpr (Rule::MIRRORS) mirrored = rule.mirrored(s);
        o = mirrored ? sp_row16_mirrored(sp.src + (sp.len - d), cnt) : sp_row16(sp.src + d, cnt);     // mirrored: row[d + k] = comp(src[len - 1 - d - k])
    }
    *reinterpret_cast<uint4 *>(rows + s * row_stride + d) = o;
}

// ---- host side (compact_rows.hip) -----------------------------------------------------------------------------------------
struct LrmCompactScratch {
    uint2 *blk; uint64_t blk_cap;             // per workgroup {rows, longest}; after compact_scan .x = rows before it
    uint32_t *d_tot;                          // {total, longest}
    uint32_t *h_tot;                          // ... in pinned host memory
    hipEvent_t ev;
};
// room for n_blk count workgroups (a zeroed *s: everything; more than it has: blk again), booked in ws->bytes
LRM_LOCAL int lrm_compact_scratch(lrm_workspace *ws, LrmCompactScratch *s, uint64_t n_blk, const char *stage);
LRM_LOCAL void lrm_compact_scratch_free(LrmCompactScratch *s);
// behind the count launch, inside its lrm_time_begin: the scan, lrm_time_end, and the one wait of the stage
LRM_LOCAL int lrm_compact_scan_wait(lrm_workspace *ws, LrmCompactScratch &s, uint32_t n_blk, hipStream_t stream, uint64_t *total, uint32_t *longest);
template <typename Rule>
static inline int lrm_compact_count(lrm_workspace *ws, LrmCompactScratch &s, const Rule &rule, uint64_t n, uint32_t n_blk,
                                    hipStream_t stream, uint64_t *total, uint32_t *longest) {
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(compact_count_kernel<Rule>, dim3(n_blk), dim3(SP_BLOCK), 0, stream, rule, n, s.blk);
    return lrm_compact_scan_wait(ws, s, n_blk, stream, total, longest);
}
// what a stage calls itself and its rows in a message
struct LrmCompactNouns { const char *stage, *rows, *row; };
// is there room for `total` rows, the longest of `longest` bases, in the stage's output (cap rows, row_stride, store_stride):
// -3 for a full table, -1 for a row stride up to the longest, a store stride below store_need, a workspace for shorter reads
// or a gather grid of more than 65535 chunks of gather_bytes; 0 with the gather grid (total rows, chunks of SP_CHUNK bytes)
// -- also for no rows at all, unchecked
LRM_LOCAL int lrm_compact_room(const lrm_workspace *ws, const LrmCompactNouns &w, uint64_t total, uint32_t longest, uint64_t cap,
                               uint64_t row_stride, uint64_t store_stride, uint64_t store_need, uint64_t gather_bytes, dim3 *grid);
