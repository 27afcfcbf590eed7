// split_kernels.hip -- gfx950 kernels of the SPLIT READS stage (docs/GACT_SPEC.md, "Split reads"): the soft-clipped ends
// of a batch become a second batch without the reads leaving the device
//
//   split_count     per workgroup of 256 reads: how many segments they have, and the longest
//   split_scan      ONE workgroup: exclusive scan of those counts in place, the total and the longest segment of the batch
//   (host)          the 8 bytes {total, longest} cross to pinned memory; the call sleeps on an event until they are there
//   split_mark      one lane per read: its 0, 1 or 2 lrm_segment records and their lengths, at its place in the order
//   split_gather    R[start .. start + len) of every segment into row s of the segment batch
//   (seed, ext.)    lrm_launch_seed and lrm_launch_extend_anchored (clip on), unchanged, over the segment rows on ws_seg,
//                   in chunks of ws_seg->n_max rows
//   split_flag      LRM_SEG_ALIGNED from the segment's meta_r and its anchor record
//
// Order: a read's first segment index is an exclusive prefix sum of the per-read counts -- wave_incl_scan on the DPP network
// inside a wavefront, the wavefront totals through LDS inside a workgroup, the workgroup totals through split_scan.  No
// atomics: the table is the same whatever the scheduling, and it is the table lrm_split_plan computes on the host.
//
// Gather: a lane moves 16 bytes per step.  The destination row is 16-byte aligned, the source is not (a right segment
// starts at n - cr): the lane loads the two aligned 16-byte words that hold its bytes and realigns them in registers
// (one 64-bit select for the word offset, one funnel shift for the byte offset).  The bytes between the segment's end and
// the next multiple of 16 are written as 0.
#include <hip/hip_runtime.h>
#include "lrm_hip_util.h"
#include "extend_stage.h"
#include "compact_rows.h"                     // SP_BLOCK, SP_CHUNK, sp_block_totals, sp_load16

struct LrmSplitScratch {
    uint2 *blk; uint64_t blk_cap;             // per workgroup {segments, longest}; after split_scan .x = segments before it
    uint32_t *d_tot;                          // {total, longest}
    uint32_t *h_tot;                          // ... in pinned host memory
    hipEvent_t ev;
};

// segments of this lane's read (0 beyond the batch)
__device__ __forceinline__ uint32_t sp_segments(const uint32_t *__restrict__ lens, const lrm_clip *__restrict__ clip, uint64_t n,
                                                uint64_t r, uint32_t M, lrm_segment two[2]) {
    if (r >= n) return 0;
    const uint2 c = *reinterpret_cast<const uint2 *>(clip + r);
    return lrm_split_segments((uint32_t) r, lens[r], c.x, c.y, M, two);
}

__global__ __launch_bounds__(SP_BLOCK) void split_count_kernel(const uint32_t *__restrict__ lens, const lrm_clip *__restrict__ clip,
                                                               uint64_t n, uint32_t M, uint2 *__restrict__ blk) {
    __shared__ uint32_t s_sum[SP_BLOCK / 64], s_max[SP_BLOCK / 64];
    lrm_segment two[2] = {};
    const uint32_t k = sp_segments(lens, clip, n, (uint64_t) blockIdx.x * SP_BLOCK + threadIdx.x, M, two);
    const uint32_t longest = max(k > 0 ? two[0].len : 0u, k > 1 ? two[1].len : 0u);
    const uint32_t incl = wave_incl_scan(k);
    const uint32_t wmax = (uint32_t) wave_max_u64(longest);
    uint32_t before, all, lmax;
    sp_block_totals(incl, wmax, s_sum, s_max, &before, &all, &lmax);
    if (threadIdx.x == 0) blk[blockIdx.x] = make_uint2(all, lmax);
}

// one workgroup walks the workgroup totals in tiles of 256 with a carried sum
__global__ __launch_bounds__(SP_BLOCK) void split_scan_kernel(uint2 *__restrict__ blk, uint32_t n_blk, uint32_t *__restrict__ tot) {
    __shared__ uint32_t s_sum[SP_BLOCK / 64], s_max[SP_BLOCK / 64];
    uint32_t carry = 0, longest = 0;
    for (uint32_t base = 0; base < n_blk; base += SP_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint2 v = i < n_blk ? blk[i] : make_uint2(0, 0);
        const uint32_t incl = wave_incl_scan(v.x);
        const uint32_t wmax = (uint32_t) wave_max_u64(v.y);
        uint32_t before, all, lmax;
        __syncthreads();                                           // the totals of the tile before have been read
        sp_block_totals(incl, wmax, s_sum, s_max, &before, &all, &lmax);
        if (i < n_blk) blk[i].x = carry + before + incl - v.x;
        carry += all;
        longest = max(longest, lmax);
    }
    if (threadIdx.x == 0) { tot[0] = carry; tot[1] = longest; }
}

__global__ __launch_bounds__(SP_BLOCK) void split_mark_kernel(const uint32_t *__restrict__ lens, const lrm_clip *__restrict__ clip,
                                                              uint64_t n, uint32_t M, const uint2 *__restrict__ blk,
                                                              lrm_segment *__restrict__ seg, uint32_t *__restrict__ seg_lens,
                                                              uint64_t cap) {
    __shared__ uint32_t s_sum[SP_BLOCK / 64], s_max[SP_BLOCK / 64];
    lrm_segment two[2] = {};
    const uint32_t k = sp_segments(lens, clip, n, (uint64_t) blockIdx.x * SP_BLOCK + threadIdx.x, M, two);
    const uint32_t incl = wave_incl_scan(k);
    uint32_t before, all, lmax;
    sp_block_totals(incl, 0, s_sum, s_max, &before, &all, &lmax);
    const uint64_t at = (uint64_t) blk[blockIdx.x].x + before + incl - k;
    if (k > 0 && at < cap) {
        *reinterpret_cast<uint4 *>(seg + at) = make_uint4(two[0].read, two[0].start, two[0].len, two[0].flags);
        seg_lens[at] = two[0].len;
    }
    if (k > 1 && at + 1 < cap) {
        *reinterpret_cast<uint4 *>(seg + at + 1) = make_uint4(two[1].read, two[1].start, two[1].len, two[1].flags);
        seg_lens[at + 1] = two[1].len;
    }
}

// grid (segments, chunks of SP_CHUNK row bytes); every lane one aligned 16-byte store
__global__ __launch_bounds__(256) void split_gather_kernel(const char *__restrict__ reads, uint64_t stride,
                                                           const lrm_segment *__restrict__ seg, uint64_t n_seg,
                                                           char *__restrict__ rows, uint64_t row_stride) {
    const uint64_t s = blockIdx.x;
    if (s >= n_seg) return;
    const uint4 sg = *reinterpret_cast<const uint4 *>(seg + s);    // read, start, len, flags
    const uint32_t len = sg.z;
    const uint64_t d = (uint64_t) blockIdx.y * SP_CHUNK + 16ull * threadIdx.x;
    if (d >= len || d + 16 > row_stride) return;                   // (row_stride > len and % 16 == 0: the second never cuts a row short)
    const uint32_t cnt = len - d < 16 ? (uint32_t) (len - d) : 16u;
    uint64_t o0, o1;
    sp_load16(reads + (uint64_t) sg.x * stride + sg.y + d, cnt, o0, o1);
    if (cnt < 16) sp_keep_bytes(cnt, o0, o1);                       // the segment's last word: zeros behind its end
    *reinterpret_cast<uint4 *>(rows + s * row_stride + d) =
        make_uint4((uint32_t) o0, (uint32_t) (o0 >> 32), (uint32_t) o1, (uint32_t) (o1 >> 32));
}

__global__ __launch_bounds__(256) void split_flag_kernel(lrm_segment *__restrict__ seg, const int32_t *__restrict__ meta_r,
                                                         const lrm_anchor *__restrict__ anchor, uint64_t n_seg) {
    const uint64_t s = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seg) return;
    if (meta_r[s] != 0 && (anchor[s].flags & LRM_ANCHOR_ANCHORED)) seg[s].flags |= LRM_SEG_ALIGNED;
}

void lrm_split_scratch_free(lrm_workspace *ws) {
    LrmSplitScratch *s = ws ? ws->sp : nullptr;
    if (!s) return;
    lrm_dev_free({s->blk, s->d_tot});
    if (s->h_tot) (void) hipHostFree(s->h_tot);
    if (s->ev) (void) hipEventDestroy(s->ev);
    free(s);
    ws->sp = nullptr;
}

// the stage's own scratch: 8 bytes per 256 reads of the primary batch, the total on the device and in pinned memory
static int split_scratch(lrm_workspace *ws, uint64_t n_blk) {
    if (!ws->sp) {
        LrmSplitScratch *s = (LrmSplitScratch *) calloc(1, sizeof(LrmSplitScratch));
        if (!s) { lrm_set_error("out of memory"); return -1; }
        ws->sp = s;
        if (hipMalloc((void **) &s->d_tot, 8) != hipSuccess || hipHostMalloc((void **) &s->h_tot, 64, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) != hipSuccess) {
            (void) hipGetLastError();
            lrm_split_scratch_free(ws);
            lrm_set_error("allocation of the split stage's scratch failed");
            return -1;
        }
        ws->bytes += 8;
    }
    LrmSplitScratch *s = ws->sp;
    if (n_blk > s->blk_cap) {
        // (freed behind everything queued on the device: the kernels of an earlier call may still read it)
        if (s->blk) { (void) hipFree(s->blk); ws->bytes -= s->blk_cap * sizeof(uint2); s->blk = nullptr; s->blk_cap = 0; }
        if (hipMalloc((void **) &s->blk, n_blk * sizeof(uint2)) != hipSuccess) {
            (void) hipGetLastError();
            lrm_set_error("hipMalloc of %llu bytes of split-stage scratch failed", (unsigned long long) (n_blk * sizeof(uint2)));
            return -1;
        }
        s->blk_cap = n_blk;
        ws->bytes += n_blk * sizeof(uint2);
    }
    return 0;
}

int lrm_launch_split(lrm_index *idx, lrm_workspace *ws, const LrmSplitArgs &a, const lrm_split_dev &out, uint64_t *n_seg_out,
                     void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const uint64_t n = a.n;
    uint32_t n_blk;
    if (lrm_grid_1d((n + SP_BLOCK - 1) / SP_BLOCK, "split mark", &n_blk)) return -1;
    if (split_scratch(ws, n_blk)) return -1;
    LrmSplitScratch &s = *ws->sp;

    // count, then the one wait of the stage
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(split_count_kernel, dim3(n_blk), dim3(SP_BLOCK), 0, stream, a.lens, a.clip, n, a.split_min_len, s.blk);
    hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(SP_BLOCK), 0, stream, s.blk, n_blk, s.d_tot);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.h_tot, s.d_tot, 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(s.ev, stream));
    if (lrm_wait_event(s.ev)) return -1;
    const uint64_t n_seg = s.h_tot[0];
    const uint32_t longest = s.h_tot[1];
    *n_seg_out = n_seg;
    if (n_seg > out.cap) {
        lrm_set_error("%llu segments, room for %llu", (unsigned long long) n_seg, (unsigned long long) out.cap);
        return -3;
    }
    if (n_seg == 0) return 0;
    if (out.row_stride <= longest) {
        lrm_set_error("split: row_stride %llu <= longest segment %u", (unsigned long long) out.row_stride, longest);
        return -1;
    }
    if (out.store_stride < lrm_anchored_store_stride(longest)) {
        lrm_set_error("split: store_stride %llu < 2*L + L/8 + 2 = %llu for the longest segment", (unsigned long long) out.store_stride,
                      (unsigned long long) lrm_anchored_store_stride(longest));
        return -1;
    }
    if (longest > ws->max_len) {
        lrm_set_error("split: segment workspace holds reads of up to %u bases, the longest segment has %u", ws->max_len, longest);
        return -1;
    }
    const uint32_t chunks = (longest + SP_CHUNK - 1) / SP_CHUNK;
    uint32_t gx;
    if (lrm_grid_1d(n_seg, "split gather", &gx)) return -1;
    if (chunks > 65535u) { lrm_set_error("split: segment of %u bases too long", longest); return -1; }
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(split_mark_kernel, dim3(n_blk), dim3(SP_BLOCK), 0, stream, a.lens, a.clip, n, a.split_min_len, s.blk, out.seg,
                       out.lens, out.cap);
    hipLaunchKernelGGL(split_gather_kernel, dim3(gx, chunks), dim3(256), 0, stream, a.reads, a.stride, out.seg, n_seg, out.rows,
                       out.row_stride);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());

    // the segment batch through the unchanged stages, ws->n_max rows at a time
    const LrmMapTune &mt = idx->mtune;
    for (uint64_t o = 0; o < n_seg; o += ws->n_max) {
        const uint64_t m = n_seg - o < ws->n_max ? n_seg - o : ws->n_max;
        char *rows = out.rows + o * out.row_stride;
        if (lrm_launch_seed(idx, ws, rows, out.row_stride, out.lens + o, m, a.seed_len, a.thres, out.best + o, mt, stream_)) return -1;
        const LrmExtendBatch b = {rows, out.row_stride, out.lens + o, m, longest, out.best + o, out.store + o * out.store_stride,
                                  out.store_stride, out.n_ops + o, out.score + o, out.meta + o, out.meta_r + o};
        if (lrm_launch_extend_anchored(idx, ws, b, a.gp, out.anchor + o, a.anchor_min_len,
                                       LrmClipOpt{1, a.clip_penalty, a.clip_end_bonus, out.clip + o}, mt, stream_)) return -1;
    }
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(split_flag_kernel, dim3((uint32_t) ((n_seg + 255) / 256)), dim3(256), 0, stream, out.seg, out.meta_r, out.anchor,
                       n_seg);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());
    return 0;
}
