// lrm_hip_util.h -- host helpers and wavefront primitives shared by the .hip files of liblrm_accel.so (lrm_internal.h and extend_stage.h are also read by plain C++)
#pragma once
#include <hip/hip_runtime.h>
#include <initializer_list>
#include "lrm_internal.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    lrm_set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// device buffer owned by a guard (debug taps): an early HIPCHK return frees it
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void) hipFree(p); }
    int alloc(uint64_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess ? 0 : -1; }
};

// a table of device buffers: hipMalloc of every entry, its bytes added to *total.  On a failure the message is
// "hipMalloc of <bytes> <what> failed" and the caller releases its whole object (the entries not reached are still null)
struct LrmDevAlloc { void **p; uint64_t bytes; };
template <size_t N>
static inline int lrm_dev_alloc_table(const LrmDevAlloc (&table)[N], const char *what, uint64_t *total) {
    for (const LrmDevAlloc &a : table) {
        if (hipMalloc(a.p, a.bytes) != hipSuccess) {
            lrm_set_error("hipMalloc of %llu %s failed", (unsigned long long) a.bytes, what);
            return -1;
        }
        *total += a.bytes;
    }
    return 0;
}
static inline void lrm_dev_free(std::initializer_list<void *> bufs) {
    for (void *b : bufs) if (b) (void) hipFree(b);
}

// x extent of a one-dimensional grid of `blocks` workgroups
static inline int lrm_grid_1d(uint64_t blocks, const char *what, uint32_t *out) {
    if (blocks > 0x7fffffffull) { lrm_set_error("%s grid too large: split the batch", what); return -1; }
    *out = (uint32_t) blocks;
    return 0;
}

#if defined(__HIPCC__)
// bits lo .. hi-1 of a word of type T, 0 <= lo <= hi <= the width of T
template <typename T>
__host__ __device__ static inline T bit_range(int lo, int hi) {
    return (hi >= (int) (8 * sizeof(T)) ? ~(T) 0 : (((T) 1 << hi) - (T) 1)) & ~(((T) 1 << lo) - (T) 1);
}

// ---- wavefront primitives on the DPP network (seed_kernels.hip, vote_kernels.hip, anchor_kernels.hip) ----
#define DPP_WAVE_SHR1 0x138  // wave_shr:1, lane L <- lane L-1 (gact_kernels.hip, op_rows.h)
// inclusive prefix sum over the 64 lanes on the DPP network: four row shifts inside the rows of 16, then the
// row totals are broadcast to the following rows (row_bcast:15 / row_bcast:31) -- six v_add_u32_dpp, no LDS
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, false);      // row_shr:1
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, false);      // row_shr:2
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, false);      // row_shr:4
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, false);      // row_shr:8
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false);      // row_bcast:15 -> rows 1, 3
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false);      // row_bcast:31 -> rows 2, 3
    return v;
}

// max over the 64 lanes, returned in every lane: the prefix-max runs on the DPP network like wave_incl_scan (row
// shifts inside the rows of 16, then row_bcast:15 / row_bcast:31), lane 63 ends up with the maximum and two readlanes
// broadcast it.  (The first version was a butterfly of __shfl_xor: twelve ds_bpermute per reduction, a third of the
// LDS instructions of a small vote item.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp_max_step(uint64_t v) {
    const uint32_t lo = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) v, CTRL, ROW_MASK, 0xf, false);
    const uint32_t hi = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) (v >> 32), CTRL, ROW_MASK, 0xf, false);
    const uint64_t o = ((uint64_t) hi << 32) | lo;                 // 0 where the lane has no source: the identity of max
    return o > v ? o : v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    v = dpp_max_step<0x111, 0xf>(v);      // row_shr:1
    v = dpp_max_step<0x112, 0xf>(v);      // row_shr:2
    v = dpp_max_step<0x114, 0xf>(v);      // row_shr:4
    v = dpp_max_step<0x118, 0xf>(v);      // row_shr:8
    v = dpp_max_step<0x142, 0xa>(v);      // row_bcast:15 -> rows 1, 3
    v = dpp_max_step<0x143, 0xc>(v);      // row_bcast:31 -> rows 2, 3
    const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) v, 63);
    const uint32_t hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) (v >> 32), 63);
    return ((uint64_t) hi << 32) | lo;
}

// the same for 32-bit values -- one DPP operand and one v_max_u32 / v_or_b32 per step instead of two moves, a 64-bit
// compare and two selects: a third of the instructions of wave_max_u64
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_src_u32(uint32_t v) {
    return (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, CTRL, ROW_MASK, 0xf, false);   // 0 where the lane has no source
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    uint32_t o;
    o = dpp_src_u32<0x111, 0xf>(v); v = o > v ? o : v;
    o = dpp_src_u32<0x112, 0xf>(v); v = o > v ? o : v;
    o = dpp_src_u32<0x114, 0xf>(v); v = o > v ? o : v;
    o = dpp_src_u32<0x118, 0xf>(v); v = o > v ? o : v;
    o = dpp_src_u32<0x142, 0xa>(v); v = o > v ? o : v;
    o = dpp_src_u32<0x143, 0xc>(v); v = o > v ? o : v;
    return (uint32_t) __builtin_amdgcn_readlane((int) v, 63);
}
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v) {
    v |= dpp_src_u32<0x111, 0xf>(v);
    v |= dpp_src_u32<0x112, 0xf>(v);
    v |= dpp_src_u32<0x114, 0xf>(v);
    v |= dpp_src_u32<0x118, 0xf>(v);
    v |= dpp_src_u32<0x142, 0xa>(v);
    v |= dpp_src_u32<0x143, 0xc>(v);
    return (uint32_t) __builtin_amdgcn_readlane((int) v, 63);
}

// ---- exclusive prefix sums by one workgroup of 1024 that loops over its n items (pileup_tile_scan_kernel, aln_diff_offsets_kernel); the 64-bit wave scan is on shuffles ----
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t o = (uint64_t) __shfl_up((unsigned long long) v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
// load(i) -> the value of item i; a scan over the wavefront, the 16 wavefront totals through LDS, the total so far carried
// from round to round; store(i, excl, mine): the sum of the items before i, and item i itself
template <typename T, typename Load, typename Store>
__device__ __forceinline__ void block1024_excl_scan(uint64_t n, Load load, Store store) {
    __shared__ T wave_total[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    T running = 0;
    for (uint64_t base = 0; base < n; base += 1024u) {
        const uint64_t i = base + tid;
        const T mine = i < n ? load(i) : (T) 0;
        const T incl = wave_incl_scan(mine);
        if (lane == 63u) wave_total[wave] = incl;
        __syncthreads();
        T before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const T wt = wave_total[k];
            before += k < wave ? wt : (T) 0;
            all += wt;
        }
        if (i < n) store(i, running + before + incl - mine, mine);
        running += all;
        __syncthreads();                                             // wave_total is rewritten by the next round
    }
}

// ---- index gathers shared by the seed-table build (index_tables.hip), the hit walk of the vote kernels (vote_hits.h) and the mapping-quality vote (mapq_kernels.hip) ----
// ----------------------------------------------------------------------------------------
// FM LF-mapping: lf(c, loc) = C[c] + rank(c, loc), rank = # of c in bwt[0..loc] == _occ_access (fmidx.c:277-293)
// and C[] as fmi_aln adds it (fmidx.c:305-311).  One 16-byte gather {C[c] + prefix, mask}, one shift and one
// popcount.  The seed kernel is bound by the number of per-lane memory requests, then by its 64-bit index arithmetic,
// so the layout is built to make an LF step ONE request and the packer folds C[c] into the stored prefix (the
// first version selected C[c] from four scalar pairs in every step: 14 of its ~63 vector instructions).
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t occ_lf_of(const ulonglong2 e, uint64_t loc) {
    return e.x + (uint64_t) __popcll(e.y << (63u - ((uint32_t) loc & 63u)));          // bits 0 .. loc % 64 of the mask
}

// SA[row].  Full SA: one 8-byte gather (sa_access, fmidx.c:18-33).  Sampled SA (LRM_SA_SAMPLED=r): only rows
// i*r are stored -- the reference's csa table (fmidx.c:153-163) -- and the other rows walk LF steps until
// they reach a stored row or the '$' row: SA[row] = SA[LF^t(row)] + t (csa_access, fmidx.c:315-331).  The
// bwt symbol of a row is the symbol whose occurrence mask holds the row's bit; the masks of the four symbols
// of a block share one 64-byte line.  The reference's own LF step there subtracts one row too many
// (fmidx.c:323, `- 1` on top of the inclusive rank: its walk leaves the text order and gives up after 5*ratio
// steps); this is the textbook LF, so that the locate equals sa_access on every row -- the two modes of this
// library give identical results, and csa_access itself is never called on the reference's hot path.
__device__ __forceinline__ uint64_t sa_locate(const LrmIndexView &ix, uint64_t row) {
    if (ix.sa_shift == 0) return ix.sa[row];
    const uint64_t rmask = (1ull << ix.sa_shift) - 1ull;
    uint64_t t = 0;
    while (row & rmask) {
        if (row == ix.dollar_row) return t;                             // SA[row] == 0
        const LrmOccBlock *b = &ix.occ[row >> 6];
        const uint32_t r = (uint32_t) row & 63u;
        const ulonglong2 e0 = *reinterpret_cast<const ulonglong2 *>(&b->sym[0]);
        const ulonglong2 e1 = *reinterpret_cast<const ulonglong2 *>(&b->sym[1]);
        const ulonglong2 e2 = *reinterpret_cast<const ulonglong2 *>(&b->sym[2]);
        const ulonglong2 e3 = *reinterpret_cast<const ulonglong2 *>(&b->sym[3]);
        const uint32_t c = (uint32_t) ((e1.y >> r) & 1ull) | ((uint32_t) ((e2.y >> r) & 1ull) << 1) | ((uint32_t) ((e3.y >> r) & 1ull) * 3u);
        const ulonglong2 e = c == 0 ? e0 : c == 1 ? e1 : c == 2 ? e2 : e3;
        row = occ_lf_of(e, row);                                        // LF(row) = C[c] + rank(c, row)
        ++t;
    }
    return ix.sa[row >> ix.sa_shift] + t;
}

// A survivor record's row field (40 bits) with bit 39 set holds the TEXT POSITION of a unique seed instead of its row: the
// seed table stores SA[k] next to such a seed (count code 0), so the vote stage has nothing to gather for it.  (Rows and
// positions stay below 2^39: 288 GB of HBM hold no longer text.)
#define LRM_LOCATED_BIT (1ull << 39)
__device__ __forceinline__ uint64_t sa_of_unique(const LrmIndexView &ix, uint64_t rec) {
    const uint64_t kk = rec & ((1ull << 40) - 1ull);
    return (kk & LRM_LOCATED_BIT) ? (kk & (LRM_LOCATED_BIT - 1ull)) : sa_locate(ix, kk);
}

// # of set bits of a wave mask below this lane
__device__ __forceinline__ uint32_t mask_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
}
#endif
