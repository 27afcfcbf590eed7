// locus_kernels.hip -- what both extension modes start with (reference: alnmain.c:408-451 -- seq_lookup :151-176,
// _rev_comp_in_place :27-60)
//
//   locus_resolve  one lane per read: seq_lookup with the reference's u64 arithmetic
//   revcomp        reverse-complement reads that resolved to the reverse strand, in place
#include <hip/hip_runtime.h>
#include "lrm_hip_util.h"
#include "extend_stage.h"
#include "seq_bytes.h"

__global__ __launch_bounds__(256) void locus_resolve_kernel(LrmIndexView ix, const lrm_entry *__restrict__ best,
                                                            const uint32_t *__restrict__ lens, uint64_t n,
                                                            lrm_seq_meta *__restrict__ meta,
                                                            int32_t *__restrict__ meta_r) {
    uint64_t read = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (read >= n) return;
    const uint64_t loc = best[read].key;                       // alnmain.c:427
    const uint32_t qlen = lens[read];
    lrm_seq_meta m;
    m.loc = 0; m.off = 0; m.seq_id = -1; m.strand = 0;
    int mr = 0;
    for (int i = 0; i < ix.mta_len; ++i) {                     // alnmain.c:155-174
        uint64_t sl = ix.mta[i].seq_len;
        uint64_t start = ix.mta[i].offset;
        uint64_t end = start + sl * 2;
        if (loc >= start && loc + qlen <= start + sl) {
            m.strand = 0; m.seq_id = i; m.loc = loc; m.off = loc - start;
            mr = 1;
            break;
        } else if (loc >= start + sl && loc + qlen <= end) {
            m.strand = 1; m.seq_id = i; m.off = end - loc - qlen; m.loc = m.off + start;
            mr = 1;
            break;
        }
    }
    // Fences: the reference consumes an uninitialised struct when the lookup fails,
    // and a wrapped u64 locus can pass the test while pointing outside the text.
    if (mr && (qlen == 0 || m.loc >= ix.con_len || (uint64_t) qlen > ix.con_len - m.loc)) mr = 0;
    if (!mr) { m.loc = 0; m.off = 0; m.seq_id = -1; m.strand = 0; }
    meta[read] = m;
    meta_r[read] = mr;
}

// In place, with ALIGNED 16-byte accesses only (rows start at any byte: stride = max_read_len + 1).  A workgroup owns
// `seg` bases of the front half of a read and their mirror bases; it copies both spans into LDS with aligned
// 16-byte loads (the first and last chunk reach a few bytes outside the span: loaded, never used), and after the
// barrier every thread builds whole aligned 16-byte chunks of each span from the other one (five LDS dwords,
// v_alignbyte, byte swap + complement).  Chunks that straddle a span's ends are written bytewise.  Measured [r2]:
// one unaligned dword per thread 1.5 ms per Gbp, one unaligned 16-byte access per thread 2.2 ms, this version
// see profiles/r2.
#define RC_SEG 4096
__device__ __forceinline__ void revcomp_span(const uint8_t *__restrict__ src, uint32_t src_off, char *gdst,
                                             uint32_t dst_off, uint32_t cnt, uint32_t tid) {
    // destination bytes i in [0, cnt) live at gdst_aligned + dst_off + i; byte i = comp(src[src_off + cnt-1-i])
    const uint32_t nchunk = (dst_off + cnt + 15) / 16;
    const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
    for (uint32_t c = tid; c < nchunk; c += 256) {
        const int32_t i0 = (int32_t) (16 * c) - (int32_t) dst_off;           // first destination byte of the chunk
        if (i0 >= 0 && (uint32_t) i0 + 16 <= cnt) {
            const uint32_t lo = src_off + cnt - 16 - (uint32_t) i0;          // source bytes [lo, lo + 16)
            const uint32_t q = lo >> 2, sh = lo & 3;
            uint32_t d[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) d[e] = src32[q + e];
            *reinterpret_cast<uint4 *>(gdst + 16 * c) = revcomp16([&](int e) { return __builtin_amdgcn_alignbyte(d[e + 1], d[e], sh); });
        } else {
            for (int k = 0; k < 16; ++k) {
                const int32_t i = i0 + k;
                if (i >= 0 && (uint32_t) i < cnt) gdst[16 * c + k] = comp_base((char) src[src_off + cnt - 1 - (uint32_t) i]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void revcomp_kernel(char *__restrict__ reads, uint64_t stride,
                                                      const uint32_t *__restrict__ lens,
                                                      const lrm_seq_meta *__restrict__ meta,
                                                      const int32_t *__restrict__ meta_r, uint64_t n,
                                                      uint32_t chunks_per_read, uint32_t seg) {
    __shared__ __attribute__((aligned(16))) uint8_t s_a[RC_SEG + 48], s_b[RC_SEG + 48];
    const uint64_t read = blockIdx.x / chunks_per_read;
    const uint32_t chunk = blockIdx.x % chunks_per_read;
    if (read >= n) return;
    if (!meta_r[read] || meta[read].strand != 1) return;       // alnmain.c:433
    const uint32_t len = lens[read], half = len / 2;
    char *r = reads + read * stride;
    const uint32_t tid = threadIdx.x;
    if (chunk == 0 && tid == 0 && (len & 1)) r[half] = comp_base(r[half]);
    const uint32_t s = chunk * seg;
    if (s >= half) return;
    const uint32_t e = s + seg < half ? s + seg : half, cnt = e - s;          // front [s, e), mirror [len-e, len-s)
    char *ga = r + s, *gb = r + (len - e);
    const uint32_t off_a = (uint32_t) ((uintptr_t) ga & 15), off_b = (uint32_t) ((uintptr_t) gb & 15);
    ga -= off_a;
    gb -= off_b;
    for (uint32_t c = tid; 16 * c < off_a + cnt; c += 256)
        *reinterpret_cast<uint4 *>(s_a + 16 * c) = *reinterpret_cast<const uint4 *>(ga + 16 * c);
    for (uint32_t c = tid; 16 * c < off_b + cnt; c += 256)
        *reinterpret_cast<uint4 *>(s_b + 16 * c) = *reinterpret_cast<const uint4 *>(gb + 16 * c);
    __syncthreads();
    revcomp_span(s_b, off_b, ga, off_a, cnt, tid);
    revcomp_span(s_a, off_a, gb, off_b, cnt, tid);
}

// locus_resolve + in-place reverse complement: what both extension modes start with
int lrm_launch_locus_revcomp(lrm_index *idx, lrm_workspace *ws, const LrmExtendBatch &b, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    lrm_time_begin(ws, LRM_K_LOCUS, stream);
    hipLaunchKernelGGL(locus_resolve_kernel, dim3((uint32_t) ((b.n + 255) / 256)), dim3(256), 0, stream,
                       idx->view, b.best, b.lens, b.n, b.meta, b.meta_r);
    lrm_time_end(ws, stream);
    const uint32_t half = b.max_len / 2 + 1;
    const uint32_t cpr = (half + RC_SEG - 1) / RC_SEG;                                  // workgroups per read
    const uint32_t seg = ((half + cpr - 1) / cpr + 15) & ~15u;                           // <= RC_SEG bases each
    uint32_t grid;
    if (lrm_grid_1d(b.n * cpr, "revcomp", &grid)) return -1;
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(revcomp_kernel, dim3(grid), dim3(256), 0, stream, b.reads, b.stride, b.lens, b.meta, b.meta_r, b.n,
                       cpr, seg);
    lrm_time_end(ws, stream);
    return 0;
}
