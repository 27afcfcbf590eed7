// compact_rows.hip -- the steps of the compact-batch stages (compact_rows.h) that do not depend on the stage's rule: the scan
// kernel, the scratch of the count / scan / mark order, the wait for {total, longest} and the room check behind it
#include <hip/hip_runtime.h>
#include <cstring>
#include "compact_rows.h"

// one workgroup walks the workgroup totals in tiles of 256 with a carried sum
__global__ __launch_bounds__(SP_BLOCK) void compact_scan_kernel(uint2 *__restrict__ blk, uint32_t n_blk, uint32_t *__restrict__ tot) {
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

void lrm_compact_scratch_free(LrmCompactScratch *s) {
    lrm_dev_free({s->blk, s->d_tot});
    if (s->h_tot) (void) hipHostFree(s->h_tot);
    if (s->ev) (void) hipEventDestroy(s->ev);
    memset(s, 0, sizeof(*s));
}

// 8 bytes per 256 reads, the total on the device and in pinned memory
int lrm_compact_scratch(lrm_workspace *ws, LrmCompactScratch *s, uint64_t n_blk, const char *stage) {
    if (!s->d_tot) {
        if (hipMalloc((void **) &s->d_tot, 8) != hipSuccess || hipHostMalloc((void **) &s->h_tot, 64, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) != hipSuccess) {
            (void) hipGetLastError();
            lrm_compact_scratch_free(s);
            lrm_set_error("allocation of the %s stage's scratch failed", stage);
            return -1;
        }
        ws->bytes += 8;
    }
    if (n_blk > s->blk_cap) {
        // (freed behind everything queued on the device: the kernels of an earlier call may still read it)
        if (s->blk) { (void) hipFree(s->blk); ws->bytes -= s->blk_cap * sizeof(uint2); s->blk = nullptr; s->blk_cap = 0; }
        if (hipMalloc((void **) &s->blk, n_blk * sizeof(uint2)) != hipSuccess) {
            (void) hipGetLastError();
            lrm_set_error("hipMalloc of %llu bytes of %s-stage scratch failed", (unsigned long long) (n_blk * sizeof(uint2)), stage);
            return -1;
        }
        s->blk_cap = n_blk;
        ws->bytes += n_blk * sizeof(uint2);
    }
    return 0;
}

int lrm_compact_scan_wait(lrm_workspace *ws, LrmCompactScratch &s, uint32_t n_blk, hipStream_t stream, uint64_t *total, uint32_t *longest) {
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(SP_BLOCK), 0, stream, s.blk, n_blk, s.d_tot);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.h_tot, s.d_tot, 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(s.ev, stream));
    if (lrm_wait_event(s.ev)) return -1;
    *total = s.h_tot[0];
    *longest = s.h_tot[1];
    return 0;
}

int lrm_compact_room(const lrm_workspace *ws, const LrmCompactNouns &w, uint64_t total, uint32_t longest, uint64_t cap, uint64_t row_stride,
                     uint64_t store_stride, uint64_t store_need, uint64_t gather_bytes, dim3 *grid) {
    if (total > cap) {
        lrm_set_error("%llu %s, room for %llu", (unsigned long long) total, w.rows, (unsigned long long) cap);
        return -3;
    }
    if (total == 0) return 0;
    if (row_stride <= longest) {
        lrm_set_error("%s: row_stride %llu <= longest %s %u", w.stage, (unsigned long long) row_stride, w.row, longest);
        return -1;
    }
    if (store_stride < store_need) {
        lrm_set_error("%s: store_stride %llu < %llu for the longest %s", w.stage, (unsigned long long) store_stride, (unsigned long long) store_need, w.row);
        return -1;
    }
    if (longest > ws->max_len) {
        lrm_set_error("%s: the workspace holds reads of up to %u bases, the longest %s has %u", w.stage, ws->max_len, w.row, longest);
        return -1;
    }
    const uint64_t chunks = (gather_bytes + SP_CHUNK - 1) / SP_CHUNK;
    if (total > 0x7fffffffull) { lrm_set_error("%s gather grid too large: split the batch", w.stage); return -1; }
    if (chunks > 65535u) { lrm_set_error("%s: rows of %llu bytes too long", w.stage, (unsigned long long) gather_bytes); return -1; }
    *grid = dim3((uint32_t) total, (uint32_t) chunks);
    return 0;
}
