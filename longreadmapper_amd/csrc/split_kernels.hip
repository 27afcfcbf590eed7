// split_kernels.hip -- gfx950 kernels of the SPLIT READS stage (docs/GACT_SPEC.md, "Split reads"): the soft-clipped ends
// of a batch become a second batch without the reads leaving the device
//
//   compact_count / compact_scan / (host) / compact_mark<SplitRule>   the segment table in its order (compact_rows.h):
//                   a read has 0, 1 or 2 lrm_segment records, lrm_split_sides says which
//   compact_gather<SplitRule>   R[start .. start + len) of every segment into row s of the segment batch
//   (seed, ext.)    lrm_launch_seed and lrm_launch_extend_anchored (clip on), unchanged, over the segment rows on ws_seg,
//                   in chunks of ws_seg->n_max rows
//   split_flag      LRM_SEG_ALIGNED from the segment's meta_r and its anchor record
//
// Gather: the shared kernel (compact_rows.h), never mirrored -- the rows are cut from the reads as the extension left them.
// The destination row is 16-byte aligned, the source is not (a right segment starts at n - cr).  The bytes between the
// segment's end and the next multiple of 16 are written as 0, nothing behind that.
#include <hip/hip_runtime.h>
#include "lrm_hip_util.h"
#include "extend_stage.h"
#include "compact_rows.h"

// the stage's rule: the sides of a read that qualify, left before right
struct SplitRule {
    const char *__restrict__ reads; uint64_t stride;
    const uint32_t *__restrict__ lens; const lrm_clip *__restrict__ clip; uint32_t M;
    lrm_segment *__restrict__ seg; uint32_t *__restrict__ seg_lens;
    typedef LrmSplitSides Item;
    __device__ uint32_t items(uint64_t n, uint64_t r, Item &s, uint32_t &longest) const {
        if (r >= n) return 0;
        const uint2 c = *reinterpret_cast<const uint2 *>(clip + r);
        s = lrm_split_sides(lens[r], c.x, c.y, M);
        longest = max(s.left, s.right);
        return (s.left != 0) + (s.right != 0);
    }
    __device__ void put(uint64_t at, uint32_t read, uint32_t start, uint32_t len, uint32_t flags) const {
        *reinterpret_cast<uint4 *>(seg + at) = make_uint4(read, start, len, flags);
        seg_lens[at] = len;
    }
    __device__ void write(uint64_t r, const Item &s, uint32_t, uint64_t at, uint64_t cap) const {
        if (s.left && at < cap) put(at, (uint32_t) r, 0u, s.left, 0u);
        at += s.left != 0;
        if (s.right && at < cap) put(at, (uint32_t) r, s.right_start, s.right, LRM_SEG_RIGHT);
    }
    // the gather: a segment's span is in its record
    static constexpr bool MIRRORS = false;
    __device__ CompactSpan span(uint64_t s) const {
        const uint4 sg = *reinterpret_cast<const uint4 *>(seg + s);    // read, start, len, flags
        return CompactSpan{reads + (uint64_t) sg.x * stride + sg.y, sg.z};
    }
    __device__ static uint64_t zeros_to(uint32_t len, uint64_t) { return len; }     // (the store that holds the last base: to the next multiple of 16)
};

__global__ __launch_bounds__(256) void split_flag_kernel(lrm_segment *__restrict__ seg, const int32_t *__restrict__ meta_r,
                                                         const lrm_anchor *__restrict__ anchor, uint64_t n_seg) {
    const uint64_t s = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seg) return;
    if (meta_r[s] != 0 && (anchor[s].flags & LRM_ANCHOR_ANCHORED)) seg[s].flags |= LRM_SEG_ALIGNED;
}

void lrm_split_scratch_free(lrm_workspace *ws) {
    if (!ws || !ws->sp) return;
    lrm_compact_scratch_free(ws->sp);
    free(ws->sp);
    ws->sp = nullptr;
}

int lrm_launch_split(lrm_index *idx, lrm_workspace *ws, const LrmSplitArgs &a, const lrm_split_dev &out, uint64_t *n_seg_out,
                     void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const uint64_t n = a.n;
    uint32_t n_blk;
    if (lrm_grid_1d((n + SP_BLOCK - 1) / SP_BLOCK, "split mark", &n_blk)) return -1;
    // the stage's own scratch grows with the primary batch
    if (!ws->sp && !(ws->sp = (LrmCompactScratch *) calloc(1, sizeof(LrmCompactScratch)))) { lrm_set_error("out of memory"); return -1; }
    LrmCompactScratch &s = *ws->sp;
    if (lrm_compact_scratch(ws, &s, n_blk, "split")) return -1;

    const SplitRule rule = {a.reads, a.stride, a.lens, a.clip, a.split_min_len, out.seg, out.lens};
    uint64_t n_seg;
    uint32_t longest;
    if (lrm_compact_count(ws, s, rule, n, n_blk, stream, &n_seg, &longest)) return -1;
    *n_seg_out = n_seg;
    dim3 grid;
    const int room = lrm_compact_room(ws, LrmCompactNouns{"split", "segments", "segment"}, n_seg, longest, out.cap, out.row_stride,
                                      out.store_stride, lrm_anchored_store_stride(longest), longest, &grid);
    if (room || n_seg == 0) return room;
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(compact_mark_kernel<SplitRule>, dim3(n_blk), dim3(SP_BLOCK), 0, stream, rule, n, (const uint2 *) s.blk, out.cap);
    hipLaunchKernelGGL(compact_gather_kernel<SplitRule>, grid, dim3(256), 0, stream, rule, n_seg, out.rows, out.row_stride);
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
