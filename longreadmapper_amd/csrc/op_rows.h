// op_rows.h -- what the stream kernels over rows of op bytes share (aln_summary_kernels.hip, aln_diff_kernels.hip,
// pileup_kernels.hip): the byte masks, the "no alignment" rule, the walk of a row on the host, and -- on the device -- the row
// loads, a wavefront's walk over its row, the previous-column carry, the packed scan.  The first half is plain C++ too.
#pragma once
#include <stdint.h>
#include "../../include/lrm_accel.h"      // lrm_seq_meta

#if defined(__HIPCC__)
#define LRM_OP_FN __host__ __device__ __forceinline__
#else
#define LRM_OP_FN inline
#endif

// 0x80 in every byte of w that equals c, 0 in every other: the EXACT zero-byte test on w ^ cccc (the cheaper form,
// (t - 0x01010101) & ~t & 0x80808080, lets a borrow run into the byte above a match: 'I' 'H' would count twice)
LRM_OP_FN uint32_t op_bytes_equal(uint32_t w, uint32_t c) {
    const uint32_t t = w ^ (c * 0x01010101u);
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}
// the masks of one word of op bytes; pw: the column before each of its bytes.  A stage reads the fields it needs.
struct OpMasks { uint32_t eq, x, d, i, s, d_open, i_open; };
LRM_OP_FN OpMasks op_masks(uint32_t cw, uint32_t pw) {
    OpMasks m;
    m.eq = op_bytes_equal(cw, '=');
    m.x = op_bytes_equal(cw, 'X');
    m.d = op_bytes_equal(cw, 'D');
    m.i = op_bytes_equal(cw, 'I');
    m.s = op_bytes_equal(cw, 'S');
    m.d_open = m.d & ~op_bytes_equal(pw, 'D');
    m.i_open = m.i & ~op_bytes_equal(pw, 'I');
    return m;
}

// byte k (0..15) of 16 bytes held in four words; selects, no indexed register
LRM_OP_FN uint32_t op_pick_byte(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t k) {
    const uint32_t w = (k & 8u) ? ((k & 4u) ? t3 : t2) : ((k & 4u) ? t1 : t0);
    return (w >> (8u * (k & 3u))) & 0xFFu;
}
// A row without an alignment: the reads cigar_text_kernel prints as "*".  n_ops: the row's own, already loaded; the two
// arrays are read only as far as the answer needs them (aln_summary_kernel is 4 % slower with the three loads made up front).
LRM_OP_FN bool op_row_absent(int32_t n_ops, const int32_t *meta_r, const int32_t *score, uint64_t row) { return n_ops <= 0 || meta_r[row] == 0 || score[row] == -1; }

// the rows a stage streams: op bytes at store + row * pitch, and what the extension left beside them
struct LrmOpRows {
    const uint8_t *store; uint64_t pitch; const int32_t *n_ops, *score, *meta_r;
    const lrm_seq_meta *meta; uint64_t rows;   // meta: null where the stage does not ask where a row lies (the summary)
};
// ---- a row on the host, walked as a lane of the kernels walks it ----
// bytes p[at .. at + 4) as a word, zeros from p + n on: nothing at or behind p + n is read
static inline uint32_t op_host_word(const uint8_t *p, uint64_t at, uint64_t n) {
    uint32_t v = 0;
    for (uint64_t k = 0; k < 4 && at + k < n; ++k) v |= (uint32_t) p[at + k] << (8 * k);
    return v;
}
// lane(cw, pw) once per 16 columns: their four words (zeros from column n on) and the column before each of their bytes,
// the previous column of a word's first byte carried along (0 before column 0)
template <typename Lane>
static inline void op_host_walk(const uint8_t *ops, uint64_t n, Lane lane) {
    uint32_t prev = 0;
    for (uint64_t c0 = 0; c0 < n; c0 += 16) {
        uint32_t cw[4], pw[4];
        for (int k = 0; k < 4; ++k) {
            cw[k] = op_host_word(ops, c0 + 4u * (uint64_t) k, n);
            pw[k] = (cw[k] << 8) | prev;
            prev = cw[k] >> 24;
        }
        lane(cw, pw);
    }
}
#if defined(__HIPCC__)
#include "lrm_hip_util.h"
// ---- row loads ----
// 16 bytes of a row of n bytes from position c0 on.  Rows start at any byte (the hardware takes the unaligned dwords, as in
// pack_rows_kernel).  row_load_step: a step that lies whole inside the row, one 16-byte load per lane.  row_load_last_step:
// the row's last step -- zeros from position n on, and nothing at or behind p + n is read.  I: the type positions are counted in.
template <typename I>
__device__ __forceinline__ uint4 row_load_step(const uint8_t *__restrict__ p, I c0) {
    uint4 v;
    __builtin_memcpy(&v, p + c0, 16);
    return v;
}
template <typename I>
__device__ __forceinline__ uint32_t row_load_word(const uint8_t *__restrict__ p, I col, I n) {
    uint32_t v = 0;
    if (col + 4 <= n) __builtin_memcpy(&v, p + col, 4);
    else if (col < n) {
        v = p[col];
        if (col + 1 < n) v |= (uint32_t) p[col + 1] << 8;
        if (col + 2 < n) v |= (uint32_t) p[col + 2] << 16;
    }
    return v;
}
template <typename I>
__device__ __forceinline__ uint4 row_load_last_step(const uint8_t *__restrict__ p, I c0, I n) {
    if (c0 + 16 <= n) return row_load_step(p, c0);
    return make_uint4(row_load_word<I>(p, c0, n), row_load_word<I>(p, c0 + 4, n), row_load_word<I>(p, c0 + 8, n), row_load_word<I>(p, c0 + 12, n));
}

// ---- one wavefront per row, four per workgroup: the grid, the row of this wavefront (uniform) and the lane in it ----
static inline int op_rows_grid(uint64_t rows, const char *what, uint32_t *grid) { return lrm_grid_1d((rows + 3) / 4, what, grid); }
__device__ __forceinline__ bool op_row_of_wave(uint64_t rows, uint64_t &row, uint32_t &lane) {
    row = (uint64_t) blockIdx.x * 4u + (uint64_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    lane = threadIdx.x & 63u;
    return row < rows;                                               // false: no such row
}
// The walk over a row of n op bytes (n uniform: every branch on it is a scalar one).  A step is 1 KiB of the row, 16 columns
// per lane from column c0 on: step(cur, c0).  Two steps are asked for together wherever both lie whole inside the row (one
// straight block: two 16-byte loads in flight per lane, the first step worked on while the second is on its way), the end
// of a row goes through the masked loads.
template <typename Step>
__device__ __forceinline__ void op_row_walk(const uint8_t *__restrict__ ops, uint32_t n, uint32_t lane, Step step) {
    uint32_t base = 0;
    for (; base + 2048u <= n; base += 2048u) {
        const uint32_t c0 = base + lane * 16u;
        const uint4 a = row_load_step<uint32_t>(ops, c0), b = row_load_step<uint32_t>(ops, c0 + 1024u);
        step(a, c0);
        step(b, c0 + 1024u);
    }
    for (; base < n; base += 1024u) {
        const uint32_t c0 = base + lane * 16u;
        step(row_load_last_step<uint32_t>(ops, c0, n), c0);
    }
}

// The column before a lane's first byte: the last byte of the lane before it (DPP wave_shr:1), for lane 0 the last byte of
// the previous step (`carry`, uniform; 0 before column 0).  w3: the lane's last word; its last byte becomes the next carry.
__device__ __forceinline__ uint32_t op_prev_byte(uint32_t &carry, uint32_t w3) {
    const uint32_t mine = w3 >> 24;
    const uint32_t prev = (uint32_t) __builtin_amdgcn_update_dpp((int) carry, (int) mine, DPP_WAVE_SHR1, 0xf, 0xf, false);   // lane 0 keeps the carry
    carry = (uint32_t) __builtin_amdgcn_readlane((int) mine, 63);
    return prev;
}

// Two counts of a lane's 16 columns share one word (at most 1024 each in a step: the halves never meet), so ONE inclusive scan
// gives both: lane_lo / lane_hi are the running totals plus the lanes before this one, run_lo / run_hi move on by the step's totals.
__device__ __forceinline__ void op_scan_pair(uint32_t lo16, uint32_t hi16, uint32_t &run_lo, uint32_t &run_hi, uint32_t &lane_lo, uint32_t &lane_hi) {
    const uint32_t mine = lo16 | (hi16 << 16);
    const uint32_t incl = wave_incl_scan(mine), excl = incl - mine;
    lane_lo = run_lo + (excl & 0xFFFFu);
    lane_hi = run_hi + (excl >> 16);
    const uint32_t total = (uint32_t) __builtin_amdgcn_readlane((int) incl, 63);
    run_lo += total & 0xFFFFu;
    run_hi += total >> 16;
}
#endif
