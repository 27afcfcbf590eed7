// pileup_kernels.hip -- the pileup (docs/GACT_SPEC.md, "Pileup"): per text position of a window, the depth and the allele
// counts of every alignment of every batch, accumulated in HBM.  pileup_add_kernel is a stream like aln_diff_kernel -- one
// byte of ops read per column -- whose atomics are proportional to the DIFFERENCES, not to the columns: one add per 'X',
// 'D' and opening 'I' column into planar event arrays, and two adds per read into a difference plane of the depth.  The
// read-back turns the difference plane into depths by a tiled prefix sum and writes the 32-byte records; it leaves the
// planes as they are.  The call stage (docs/GACT_SPEC.md, "Pileup calls") reads the same planes and the text: the sites --
// the positions where the reads disagree with the text -- compacted into a table by count, scan, write at the prefix sum
// (the idiom of compact_rows.h: no atomics, the same table whatever the scheduling), and one consensus byte per position.
// The insertion side (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus"): an accumulator with insertion
// planes launches pileup_add_ins_kernel, the same row walk compiled with the inserted bases counted too; the polish kernels
// write the consensus letters and the inserted bases as one sequence, compacted by the same idiom over byte counts.
// The variant stage (docs/GACT_SPEC.md, "Pileup variants and VCF"): the sites as variant records, adjacent deleted positions
// merged into one run by a segmented scan of per-tile summaries -- count, scan, write once more, over record counts.
#include <hip/hip_runtime.h>
#include "pileup_step.h"
#include "pileup_call_step.h"
#include "pileup_ins_step.h"
#include "pileup_var_step.h"

namespace {

// relaxed, agent scope, result unused: one global_atomic_add_u32 without return (read in the gfx950 disassembly: no
// compare-and-swap loop)
__device__ __forceinline__ void pile_add(uint32_t *p, uint32_t v) {
    (void) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a wavefront carries from step to step of its row, all uniform: the target-consuming and the query-consuming columns
// so far, and the last op byte of the previous step (0 before column 0)
// (run: with insertion planes, the 'I' columns that end the previous step, saturated -- pile_ins_carry)
struct PileRow { uint32_t t = 0, q = 0, carry = 0, run = 0; };

// the window as a kernel sees it: text positions [lo, hi), W = hi - lo, the event planes behind the W + 1 depth words
struct PileWindow { uint64_t lo, hi, W; uint32_t *planes; };
// the insertion planes of an accumulator that has them (pileup_ins_step.h): K columns, 4 * K planes of W words
struct PileIns { uint32_t *planes; uint32_t K; };

// The 'I' columns immediately in front of a lane's first column, saturated at 16: the trailing 'I' columns of the lane before
// it (DPP wave_shr:1) -- a lane whose 16 columns are all 'I' hands on "at least 16", which no K reaches, so no scan is
// needed -- and for lane 0 those of the previous step's lane 63 (`carry`, uniform; 0 before column 0): op_prev_byte's shape.
__device__ __forceinline__ uint32_t pile_ins_carry(uint32_t &carry, uint32_t trail) {
    const uint32_t in = (uint32_t) __builtin_amdgcn_update_dpp((int) carry, (int) trail, DPP_WAVE_SHR1, 0xf, 0xf, false);   // lane 0 keeps the carry
    carry = (uint32_t) __builtin_amdgcn_readlane((int) trail, 63);
    return in;
}

// One step: the lane's 16 columns (zeros from column n on).  The packed scan of the lane's target-consuming and its
// query-consuming columns gives the lane's target column and its first query byte.  The lane's at most 16 query bytes are
// contiguous: one unaligned 16-byte read (nothing at or behind read + len), every 'X' column's byte picked out of the four
// registers.  INS: the variant of an accumulator with insertion planes -- the same masks and the same 16 query bytes also
// give the inserted bases (pile_ins_word_step); a lane whose only event is a continuing 'I' column goes on.
template <bool INS>
__device__ __forceinline__ void pile_step(PileRow &r, const uint4 cur, const uint8_t *__restrict__ read, uint32_t len, uint64_t loc,
                                          const PileWindow &win, const PileIns &ins) {
    const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
    uint32_t prev = op_prev_byte(r.carry, w[3]);
    OpMasks m[4];
    uint32_t tc = 0, qc = 0, any = 0, any_x = 0, trail = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        m[k] = op_masks(w[k], (w[k] << 8) | prev);
        prev = w[k] >> 24;
        tc += (uint32_t) __popc(m[k].eq | m[k].x | m[k].d);
        qc += (uint32_t) __popc(m[k].eq | m[k].x | m[k].i | m[k].s);
        any |= m[k].x | m[k].d | (INS ? m[k].i : m[k].i_open);
        any_x |= m[k].x | (INS ? m[k].i : 0u);
        if (INS) trail = pile_ins_run_behind(m[k].i, trail);
    }
    uint32_t run = 0;
    if (INS) run = pile_ins_carry(r.run, trail);
    uint32_t t_lane, q_lane;
    op_scan_pair(tc, qc, r.t, r.q, t_lane, q_lane);
    if (!any) return;
    uint4 qb = make_uint4(0u, 0u, 0u, 0u);
    if (any_x) qb = row_load_last_step<uint32_t>(read, q_lane, len);
    uint32_t t = t_lane, q = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (INS)                                                     // (before pile_word_step moves t and q on by the word)
            pile_ins_word_step(m[k], t, q, run, ins.K, qb.x, qb.y, qb.z, qb.w, [&](uint32_t j, uint32_t cls, uint32_t tcol) {
                const uint64_t pos = loc + tcol;
                if (pos >= win.lo && pos < win.hi) pile_add(ins.planes + LRM_PILEUP_INS_PLANE(win.W, j, cls) + (pos - win.lo), 1u);
            });
        pile_word_step(m[k], t, q, qb.x, qb.y, qb.z, qb.w, [&](uint32_t plane, uint32_t tcol) {
            const uint64_t pos = loc + tcol;
            if (pos >= win.lo && pos < win.hi) pile_add(win.planes + LRM_PILEUP_EVENT_PLANE(win.W, plane) + (pos - win.lo), 1u);
        });
    }
}

// One wavefront per read, four per workgroup; no LDS, no barrier: the walk of op_rows.h.  A read without an alignment, a
// filtered read and a read that starts at or behind the window's end leave before their first row load.  Lane 0 makes the
// two depth adds once the row's target span is known.
template <bool INS>
__device__ __forceinline__ void pile_add_row(const uint8_t *__restrict__ reads, uint64_t stride, const uint32_t *__restrict__ lens,
                                             const uint8_t *__restrict__ store, uint64_t pitch, const int32_t *__restrict__ n_ops,
                                             const int32_t *__restrict__ score, const int32_t *__restrict__ meta_r,
                                             const lrm_seq_meta *__restrict__ meta, uint64_t rows, const lrm_mapq *__restrict__ mapq,
                                             uint32_t min_mapq, const PileWindow &win, const PileIns &ins) {
    uint64_t row; uint32_t lane;
    if (!op_row_of_wave(rows, row, lane)) return;
    const int nn = n_ops[row];
    if (op_row_absent(nn, meta_r, score, row)) return;
    if (mapq && (uint32_t) mapq[row].mapq < min_mapq) return;
    const uint64_t loc = meta[row].loc;
    if (loc >= win.hi) return;                                       // every count of the read lies at or behind loc
    const uint8_t *read = reads + row * stride;
    const uint32_t len = lens[row];
    PileRow r;
    op_row_walk(store + row * pitch, (uint32_t) nn, lane, [&](const uint4 cur, uint32_t) { pile_step<INS>(r, cur, read, len, loc, win, ins); });
    if (lane == 0) {
        const uint64_t a = loc > win.lo ? loc : win.lo, end = loc + r.t, b = end < win.hi ? end : win.hi;
        if (a < b) {                                                 // the covered interval clipped to the window
            pile_add(win.planes + (a - win.lo), 1u);
            pile_add(win.planes + (b - win.lo), 0xFFFFFFFFu);        // -1; word W when the interval reaches hi
        }
    }
}
// the kernel of a plain accumulator, and the variant of one with insertion planes: the same row walk, compiled twice
__global__ __launch_bounds__(256) void pileup_add_kernel(const uint8_t *__restrict__ reads, uint64_t stride, const uint32_t *__restrict__ lens,
                                                         const uint8_t *__restrict__ store, uint64_t pitch, const int32_t *__restrict__ n_ops,
                                                         const int32_t *__restrict__ score, const int32_t *__restrict__ meta_r,
                                                         const lrm_seq_meta *__restrict__ meta, uint64_t rows, const lrm_mapq *__restrict__ mapq,
                                                         uint32_t min_mapq, PileWindow win) {
    pile_add_row<false>(reads, stride, lens, store, pitch, n_ops, score, meta_r, meta, rows, mapq, min_mapq, win, PileIns{nullptr, 0u});
}
__global__ __launch_bounds__(256) void pileup_add_ins_kernel(const uint8_t *__restrict__ reads, uint64_t stride, const uint32_t *__restrict__ lens,
                                                             const uint8_t *__restrict__ store, uint64_t pitch, const int32_t *__restrict__ n_ops,
                                                             const int32_t *__restrict__ score, const int32_t *__restrict__ meta_r,
                                                             const lrm_seq_meta *__restrict__ meta, uint64_t rows, const lrm_mapq *__restrict__ mapq,
                                                             uint32_t min_mapq, PileWindow win, PileIns ins) {
    pile_add_row<true>(reads, stride, lens, store, pitch, n_ops, score, meta_r, meta, rows, mapq, min_mapq, win, ins);
}

// the sum over the 256 threads of a workgroup, returned in every thread, and the inclusive prefix of this thread: a scan
// over the wavefront on the DPP network, the four wavefront totals through LDS (lds: 4 words; two barriers)
__device__ __forceinline__ uint32_t block256_incl_scan(uint32_t v, uint32_t *lds, uint32_t &all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v);
    __syncthreads();                                                 // lds is read by the previous round
    if (lane == 63u) lds[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    all = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t wt = lds[k];
        before += k < wave ? wt : 0u;
        all += wt;
    }
    return before + incl;
}

// read-back 1: the sum of the difference plane over every tile of LRM_PILEUP_TILE positions, one workgroup per tile
__global__ __launch_bounds__(256) void pileup_tile_sums_kernel(const uint32_t *__restrict__ diff, uint64_t W, uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t lds[4];
    const uint64_t base = (uint64_t) blockIdx.x * LRM_PILEUP_TILE;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < LRM_PILEUP_TILE / 256u; ++j) {
        const uint64_t g = base + j * 256u + threadIdx.x;
        v += g < W ? diff[g] : 0u;
    }
    uint32_t all;
    (void) block256_incl_scan(v, lds, all);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// read-back 2: exclusive prefix sums of the tile sums (the depth in front of every tile), 32-bit and wrapping like the counters
__global__ __launch_bounds__(1024) void pileup_tile_scan_kernel(const uint32_t *__restrict__ tile_sum, uint64_t n, uint32_t *__restrict__ tile_base) {
    block1024_excl_scan<uint32_t>(n, [&](uint64_t i) { return tile_sum[i]; }, [&](uint64_t i, uint32_t excl, uint32_t) { tile_base[i] = excl; });
}

// The depth of every position of a tile, by a workgroup of 256: the tile is rescanned from its base, 256 positions a round,
// and body(g, depth) runs in every thread of every round -- it may hold barriers.  g may lie behind W: the range test is the body's.
template <typename Body>
__device__ __forceinline__ void pile_tile_rescan(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base,
                                                 uint64_t tile, uint32_t *lds, Body body) {
    uint32_t running = tile_base[tile];
#pragma unroll 1
    for (uint32_t j = 0; j < LRM_PILEUP_TILE / 256u; ++j) {
        const uint64_t g = tile * LRM_PILEUP_TILE + j * 256u + threadIdx.x;
        uint32_t all;
        const uint32_t depth = running + block256_incl_scan(g < W ? planes[g] : 0u, lds, all);
        running += all;
        body(g, depth);
    }
}

// read-back 3: the records of the window positions [first, first + count), one workgroup per tile that holds any of them
// (tile0: the tile of `first`).  A position inside the range reads its seven event words and writes its record with two
// aligned 16-byte stores.
__global__ __launch_bounds__(256) void pileup_cols_kernel(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base,
                                                          uint64_t tile0, uint64_t first, uint64_t count, lrm_pileup_col *__restrict__ out) {
    __shared__ uint32_t lds[4];
    pile_tile_rescan(planes, W, tile_base, tile0 + blockIdx.x, lds, [&](uint64_t g, uint32_t depth) {
        if (g < first || g - first >= count) return;                 // (first + count <= W: g < W here)
        uint32_t w[8];
        pile_col_words(planes, W, g, depth, w);
        uint4 *o = reinterpret_cast<uint4 *>(out + (g - first));
        o[0] = make_uint4(w[0], w[1], w[2], w[3]);
        o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    });
}

// ---- the call stage ----
typedef uint32_t pile_u32x4 __attribute__((ext_vector_type(4)));
// one position inside the requested range: its record's words, its text byte (text: content + lo), the rule
struct PilePos { uint32_t n_eq, n_del, n_ins, byte; PileCall call; };
__device__ __forceinline__ PilePos pile_call_at(const uint32_t *__restrict__ planes, uint64_t W, uint64_t g, uint32_t depth,
                                                const uint8_t *__restrict__ text, const PileCallRule &rule) {
    uint32_t w[8];
    pile_col_words(planes, W, g, depth, w);
    PilePos p;
    p.n_eq = w[1];
    p.n_del = w[6];
    p.n_ins = w[7];
    p.byte = text[g];
    p.call = pile_call(rule, depth, p.n_eq, w[2], w[3], w[4], w[5], p.n_del, p.n_ins, p.byte);
    return p;
}

// calls 1: one workgroup per tile that holds a requested position (tile0: the tile of `first`).  A position inside the
// range is evaluated, its cons byte written when the caller asked (a byte store at cons + (g - first): `first` is
// arbitrary, so nothing wider is aligned at the range's ends, and nothing outside cons[0 .. count) is touched); the tile's
// number of sites goes to tile_sites[blockIdx.x].
__global__ __launch_bounds__(256) void pileup_call_kernel(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base,
                                                          uint64_t tile0, uint64_t first, uint64_t count, const uint8_t *__restrict__ text,
                                                          PileCallRule rule, uint8_t *__restrict__ cons, uint32_t *__restrict__ tile_sites) {
    __shared__ uint32_t lds[4];
    uint32_t mine = 0;
    pile_tile_rescan(planes, W, tile_base, tile0 + blockIdx.x, lds, [&](uint64_t g, uint32_t depth) {
        if (g < first || g - first >= count) return;                 // (first + count <= W: g < W here)
        const PilePos p = pile_call_at(planes, W, g, depth, text, rule);
        if (cons) cons[g - first] = p.call.cons;
        mine += p.call.kinds ? 1u : 0u;
    });
    uint32_t all;
    (void) block256_incl_scan(mine, lds, all);
    if (threadIdx.x == 0) tile_sites[blockIdx.x] = all;
}

// calls 2 is pileup_tile_scan_kernel over the tiles' site counts.  calls 3: one workgroup per tile again.  The last one
// writes the total -- its own rank plus its own count -- as 64 bits.  A tile without a site, or whose first site already
// lies at or behind cap, leaves after its scalar loads.  Otherwise the tile is evaluated again from the planes (no
// per-position array between the two kernels: sites are few, so few tiles come back here, and a kinds byte per position
// would be W more bytes written and kept for every call); the sites of a round are ranked by a block scan of the site flag
// in every thread, the running rank carried as the depth is, and a record goes to sites[rank] with two aligned 16-byte stores when rank < cap.
__global__ __launch_bounds__(256) void pileup_sites_kernel(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base,
                                                           uint64_t tile0, uint64_t first, uint64_t count, uint64_t lo,
                                                           const uint8_t *__restrict__ text, PileCallRule rule,
                                                           const uint32_t *__restrict__ tile_sites, const uint32_t *__restrict__ tile_rank,
                                                           lrm_pileup_site *__restrict__ sites, uint64_t cap, uint64_t *__restrict__ n_sites) {
    __shared__ uint32_t lds[4];
    const uint32_t n_here = tile_sites[blockIdx.x];
    uint64_t rank = tile_rank[blockIdx.x];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_sites = rank + n_here;
    if (n_here == 0 || rank >= cap) return;
    pile_tile_rescan(planes, W, tile_base, tile0 + blockIdx.x, lds, [&](uint64_t g, uint32_t depth) {
        PilePos p = {};
        if (g >= first && g - first < count) p = pile_call_at(planes, W, g, depth, text, rule);
        const uint32_t flag = p.call.kinds ? 1u : 0u;
        uint32_t all;
        const uint64_t at = rank + (block256_incl_scan(flag, lds, all) - flag);
        rank += all;
        if (flag && at < cap) {
            uint32_t w[8];
            pile_call_site_words(p.call, lo + g, depth, p.n_eq, p.n_del, p.n_ins, p.byte, w);
            // (each half pinned in four consecutive registers: left alone, the compiler merges the two stores and cuts the
            // 32 bytes at the 64-bit position instead, 8 + 12 + 12)
            pile_u32x4 h0 = {w[0], w[1], w[2], w[3]}, h1 = {w[4], w[5], w[6], w[7]};
            asm volatile("" : "+v"(h0), "+v"(h1));
            pile_u32x4 *o = reinterpret_cast<pile_u32x4 *>(sites + at);
            o[0] = h0;
            o[1] = h1;
        }
    });
}

// ---- the insertion side (docs/GACT_SPEC.md, "Pileup insertions and the polished consensus") ----
// the bytes of one position inside the requested range: its cons letter and, where it enters, its inserted allele.  The
// position's 4 * K insertion words are read only where 2 * n_ins > depth (pile_polish_at): 16 * K bytes per position otherwise.
__device__ __forceinline__ PilePolish pile_polish_pos(const uint32_t *__restrict__ planes, uint64_t W, uint64_t g, uint32_t depth,
                                                      const uint8_t *__restrict__ text, const PileCallRule &rule, const PileIns &ins) {
    const PilePos p = pile_call_at(planes, W, g, depth, text, rule);
    return pile_polish_at(rule, p.call.cons, depth, p.n_ins, ins.K, [&]() { return pile_ins_allele(rule, depth, p.n_ins, ins.planes + g, W, ins.K); });
}

// polish 1: one workgroup per tile that holds a requested position; the tile's number of BYTES goes to tile_bytes[blockIdx.x]
__global__ __launch_bounds__(256) void pileup_polish_count_kernel(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base,
                                                                  uint64_t tile0, uint64_t first, uint64_t count, const uint8_t *__restrict__ text,
                                                                  PileCallRule rule, PileIns ins, uint32_t *__restrict__ tile_bytes) {
    __shared__ uint32_t lds[4];
    uint32_t mine = 0;
    pile_tile_rescan(planes, W, tile_base, tile0 + blockIdx.x, lds, [&](uint64_t g, uint32_t depth) {
        if (g < first || g - first >= count) return;                 // (first + count <= W: g < W here)
        mine += pile_polish_pos(planes, W, g, depth, text, rule, ins).n;
    });
    uint32_t all;
    (void) block256_incl_scan(mine, lds, all);
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = all;
}

// polish 2 is pileup_tile_scan_kernel over the tiles' byte counts.  polish 3: one workgroup per tile again; the last one
// writes the total as 64 bits.  A tile without a byte, or whose first byte already lies at or behind cap, leaves after its
// scalar loads.  Otherwise the tile is evaluated again; a round's byte counts (0 .. K + 1 per thread) are ranked by a block
// scan, the running offset carried as the depth is, and every byte goes to seq[tile base + rank] when that lies below cap:
// byte stores (the offsets are arbitrary), nothing outside seq[0 .. cap).
__global__ __launch_bounds__(256) void pileup_polish_write_kernel(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base,
                                                                  uint64_t tile0, uint64_t first, uint64_t count, const uint8_t *__restrict__ text,
                                                                  PileCallRule rule, PileIns ins, const uint32_t *__restrict__ tile_bytes,
                                                                  const uint32_t *__restrict__ tile_rank, uint8_t *__restrict__ seq, uint64_t cap,
                                                                  uint64_t *__restrict__ len_out) {
    __shared__ uint32_t lds[4];
    const uint32_t n_here = tile_bytes[blockIdx.x];
    uint64_t rank = tile_rank[blockIdx.x];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *len_out = rank + n_here;
    if (n_here == 0 || rank >= cap) return;
    pile_tile_rescan(planes, W, tile_base, tile0 + blockIdx.x, lds, [&](uint64_t g, uint32_t depth) {
        PilePolish p = {};
        if (g >= first && g - first < count) p = pile_polish_pos(planes, W, g, depth, text, rule, ins);
        uint32_t all;
        const uint64_t at = rank + (block256_incl_scan(p.n, lds, all) - p.n);
        rank += all;
#pragma unroll
        for (uint32_t j = 0; j <= LRM_PILEUP_INS_COLS_LIMIT; ++j)
            if (j < p.n && at + j < cap) seq[at + j] = (uint8_t) pile_polish_byte(p, j);
    });
}

// the insertion words of positions [first, first + items / K), position-major: one thread per position and insertion column
// reads the column's four planes and writes one aligned 16-byte group
__global__ __launch_bounds__(256) void pileup_ins_read_kernel(const uint32_t *__restrict__ ins, uint64_t W, uint32_t K, uint64_t first, uint64_t items,
                                                              uint4 *__restrict__ out) {
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const uint64_t g = first + i / K;                                // (first + items / K <= W)
    const uint32_t *s = ins + LRM_PILEUP_INS_PLANE(W, i % K, 0u) + g;
    out[i] = make_uint4(s[0], s[W], s[2u * W], s[3u * W]);
}

// the inserted allele of every record of a site table, one thread per site: depth and n_ins are the record's, so no scan;
// a pos outside the window gives an all-zero record
__global__ __launch_bounds__(256) void pileup_site_alleles_kernel(const uint32_t *__restrict__ ins, uint64_t lo, uint64_t hi, uint32_t K,
                                                                  PileCallRule rule, const lrm_pileup_site *__restrict__ sites, uint64_t n,
                                                                  uint4 *__restrict__ out) {
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 *s = reinterpret_cast<const uint4 *>(sites + i);
    const uint4 h0 = s[0], h1 = s[1];                                // pos, depth, n_ref | n_alt, n_del, n_ins, the four bytes
    const uint64_t pos = (uint64_t) h0.x | ((uint64_t) h0.y << 32);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (pos >= lo && pos < hi) pile_ins_allele_words(pile_ins_allele(rule, h0.z, h1.z, ins + (pos - lo), hi - lo, K), w);
    out[i] = make_uint4(w[0], w[1], w[2], w[3]);
}

// the merge of two accumulators (docs/GACT_SPEC.md, "Pileup on the host-buffer path and across replicas"): dst[w] += src[w] for
// w < words, 32-bit and wrapping like the counters.  A plain stream, no LDS, no atomics (the caller orders the writers of dst):
// the first `quads` groups of four words go through 16-byte loads and one 16-byte store each -- quads is words / 4 when both
// pointers are 16-byte aligned, 0 otherwise --, the words behind them one by one.  An allocation holds 8 W + 1 words, so
// there is always such a tail.  Nothing at or behind word `words` of either side is touched.
__global__ __launch_bounds__(256) void pileup_merge_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t words, uint64_t quads) {
    const uint64_t tid = (uint64_t) blockIdx.x * 256u + threadIdx.x, step = (uint64_t) gridDim.x * 256u;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    for (uint64_t q = tid; q < quads; q += step) {
        const uint4 a = d4[q], b = s4[q];
        d4[q] = make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    for (uint64_t w = 4u * quads + tid; w < words; w += step) dst[w] += src[w];
}

// ---- the variant stage (docs/GACT_SPEC.md, "Pileup variants and VCF"; the rule: pileup_var_step.h) ----
// What a workgroup keeps of its tile: the words of the block scan, the LRM_CALL_DEL flags of the tile's requested positions
// as a bit map (bit i of word i / 32: the tile's position i; positions outside the range are 0), and the flag of the position
// in front of the tile (0 when that lies outside the range).
struct PileVarLds { uint32_t scan[4], map[LRM_PILEUP_TILE / 32u], prev; };

// The first pass over a tile: every requested position evaluated, the map and `prev` left in LDS behind a barrier.  The
// position in front of the tile has the depth tile_base[tile] -- the exclusive prefix is its inclusive one -- so one thread
// evaluates it directly.  A wavefront's 64 flags of a round are one ballot: two words of the map, no atomics.  Returns this
// thread's number of SNV and INS records.
__device__ __forceinline__ uint32_t pile_var_map(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base, uint64_t tile,
                                                 uint64_t first, uint64_t count, const uint8_t *__restrict__ text, const PileCallRule &rule, PileVarLds &s) {
    if (threadIdx.x == 0) {
        const uint64_t g0 = tile * LRM_PILEUP_TILE;
        uint32_t prev = 0;
        if (g0 > first) prev = (pile_call_at(planes, W, g0 - 1u, tile_base[tile], text, rule).call.kinds & LRM_CALL_DEL) ? 1u : 0u;
        s.prev = prev;
    }
    uint32_t mine = 0, round = 0;
    pile_tile_rescan(planes, W, tile_base, tile, s.scan, [&](uint64_t g, uint32_t depth) {
        uint32_t kinds = 0;
        if (g >= first && g - first < count) kinds = pile_call_at(planes, W, g, depth, text, rule).call.kinds;   // (first + count <= W: g < W here)
        mine += ((kinds & LRM_CALL_SNV) ? 1u : 0u) + ((kinds & LRM_CALL_INS) ? 1u : 0u);
        const unsigned long long del = __ballot((kinds & LRM_CALL_DEL) != 0u);
        if ((threadIdx.x & 63u) == 0u) {
            const uint32_t at = round * 8u + (threadIdx.x >> 6) * 2u;
            s.map[at] = (uint32_t) del;
            s.map[at + 1u] = (uint32_t) (del >> 32);
        }
        ++round;
    });
    __syncthreads();
    return mine;
}

// variants 1: one workgroup per tile that holds a requested position.  The tile's number of records -- its SNV and INS
// positions plus the deleted positions that start a run, read off the map a word per thread -- goes to tile_n[blockIdx.x];
// the tile's summary for the runs that cross tiles goes to tile_lead[blockIdx.x]: how many of its leading requested positions
// are deleted without a gap, and whether these are all of them (pile_var_lead_word).
__global__ __launch_bounds__(256) void pileup_var_count_kernel(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base,
                                                               uint64_t tile0, uint64_t first, uint64_t count, const uint8_t *__restrict__ text,
                                                               PileCallRule rule, uint32_t *__restrict__ tile_n, uint32_t *__restrict__ tile_lead) {
    __shared__ PileVarLds s;
    const uint64_t tile = tile0 + blockIdx.x;
    uint32_t mine = pile_var_map(planes, W, tile_base, tile, first, count, text, rule, s);
    if (threadIdx.x < 64u) {                                           // wavefront 0, a word of the map per lane
        const uint32_t i = threadIdx.x, w = s.map[i];
        const uint32_t carry = i ? s.map[i - 1u] >> 31 : s.prev;
        mine += (uint32_t) __popc(w & ~((w << 1) | carry));            // deleted, and the position before is not
        const uint64_t g0 = tile * LRM_PILEUP_TILE, end = first + count;
        const uint32_t a = first > g0 ? (uint32_t) (first - g0) : 0u;  // the tile's requested positions are [a, b)
        const uint32_t b = end - g0 < LRM_PILEUP_TILE ? (uint32_t) (end - g0) : (uint32_t) LRM_PILEUP_TILE;
        const uint32_t from_a = i == (a >> 5) ? ~0u << (a & 31u) : (i > (a >> 5) ? ~0u : 0u);
        const uint32_t open = ~w & from_a;                             // not deleted, at or behind a
        const uint32_t stop = open ? 32u * i + (uint32_t) __builtin_ctz(open) : (uint32_t) LRM_PILEUP_TILE;
        const uint32_t nearest = ~wave_max_u32(~stop);                 // the minimum over the 64 words
        const uint32_t until = nearest < b ? nearest : b;
        PileVarLead lead;
        lead.len = until - a;
        lead.full = until == b;
        if (i == 0) tile_lead[blockIdx.x] = pile_var_lead_word(lead);
    }
    uint32_t all;
    (void) block256_incl_scan(mine, s.scan, all);
    if (threadIdx.x == 0) tile_n[blockIdx.x] = all;
}

// variants 2 is pileup_tile_scan_kernel over the tiles' record counts.  variants 3: tile_ext[t] = the length of the deleted run
// that starts at the first position of tile t + 1, 0 for the last tile: tile_ext[t] = lead[t + 1] + (tile t + 1 wholly
// deleted ? tile_ext[t + 1] : 0).  A backward segmented scan with pile_var_lead_join by one workgroup of 1024 that loops over
// its n tiles from the last one like block1024_excl_scan: a scan over the wavefront on shuffles, the 16 wavefront summaries
// through LDS, the summary of everything done so far carried from round to round.  The work is the same whatever the runs.
__global__ __launch_bounds__(1024) void pileup_var_ext_kernel(const uint32_t *__restrict__ tile_lead, uint64_t n, uint32_t *__restrict__ tile_ext) {
    __shared__ uint32_t wave_total[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const PileVarLead none = {0u, true};
    PileVarLead running = none;                                        // of the tiles behind every tile done so far
    for (uint64_t base = 0; base < n; base += 1024u) {
        const uint64_t r = base + tid;                                 // item r is tile n - 1 - r: the scan runs from the last tile
        PileVarLead v = r < n ? pile_var_lead_of(tile_lead[n - 1u - r]) : none;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {                       // v: this tile, then the d - 1 tiles behind it
            const PileVarLead far = pile_var_lead_of((uint32_t) __shfl_up(pile_var_lead_word(v), d, 64));
            if (lane >= d) v = pile_var_lead_join(v, far);
        }
        if (lane == 63u) wave_total[wave] = pile_var_lead_word(v);
        const PileVarLead behind = pile_var_lead_of((uint32_t) __shfl_up(pile_var_lead_word(v), 1u, 64));
        PileVarLead acc = lane ? behind : none;                        // the tiles of this wavefront behind this one
        __syncthreads();
        PileVarLead chunk = none;
#pragma unroll
        for (int k = 15; k >= 0; --k) {                                // nearest first: wavefront 15 holds the tiles in front
            const PileVarLead wt = pile_var_lead_of(wave_total[k]);
            if ((uint32_t) k < wave) acc = pile_var_lead_join(acc, wt);
            chunk = pile_var_lead_join(chunk, wt);
        }
        if (r < n) tile_ext[n - 1u - r] = pile_var_lead_join(acc, running).len;
        running = pile_var_lead_join(chunk, running);
        __syncthreads();                                               // wave_total is rewritten by the next round
    }
}

// variants 4: one workgroup per tile again.  The last one writes the total as 64 bits.  A tile without a record, or whose
// first record already lies at or behind cap, leaves after its scalar loads.  Otherwise the first pass leaves the map again
// and a second one evaluates the tile once more: a round's per-thread record counts (0 .. 3) are ranked by a block scan, the
// running rank carried as the depth is, and every record goes to vars[rank] with three aligned 16-byte stores when rank <
// cap.  The thread of a run's first position finds its end in the map -- the first clear bit behind it, at most 64 words --
// and adds tile_ext when the run reaches the tile's end.  The position's 4 * K insertion words are read only where it has
// LRM_CALL_INS; the allele travels as one 64-bit word (no private segment).
__global__ __launch_bounds__(256) void pileup_var_write_kernel(const uint32_t *__restrict__ planes, uint64_t W, const uint32_t *__restrict__ tile_base,
                                                               uint64_t tile0, uint64_t first, uint64_t count, uint64_t lo,
                                                               const uint8_t *__restrict__ text, PileVarRule rule, PileIns ins,
                                                               const uint32_t *__restrict__ tile_n, const uint32_t *__restrict__ tile_rank,
                                                               const uint32_t *__restrict__ tile_ext, lrm_pileup_variant *__restrict__ vars,
                                                               uint64_t cap, uint64_t *__restrict__ n_vars) {
    __shared__ PileVarLds s;
    const uint32_t n_here = tile_n[blockIdx.x];
    uint64_t rank = tile_rank[blockIdx.x];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_vars = rank + n_here;
    if (n_here == 0 || rank >= cap) return;
    const uint64_t tile = tile0 + blockIdx.x;
    (void) pile_var_map(planes, W, tile_base, tile, first, count, text, rule.call, s);
    const uint32_t ext = tile_ext[blockIdx.x];
    uint32_t round = 0;
    pile_tile_rescan(planes, W, tile_base, tile, s.scan, [&](uint64_t g, uint32_t depth) {
        PilePos p = {};
        if (g >= first && g - first < count) p = pile_call_at(planes, W, g, depth, text, rule.call);
        const uint32_t i = round * 256u + threadIdx.x;                 // the position's place in the tile
        ++round;
        const uint32_t before = i ? (s.map[(i - 1u) >> 5] >> ((i - 1u) & 31u)) & 1u : s.prev;
        const uint32_t emits = pile_var_emits(p.call.kinds, before != 0u);
        const uint32_t c = pile_var_count(emits);
        uint32_t all;
        uint64_t at = rank + (block256_incl_scan(c, s.scan, all) - c);
        rank += all;
        if (c == 0u || at >= cap) return;
        uint32_t run = 0;
        if (emits & LRM_CALL_DEL) {
            uint32_t k = i >> 5;
            uint32_t open = ~s.map[k] & (~0u << (i & 31u));            // (bit i itself is set)
            while (!open && ++k < LRM_PILEUP_TILE / 32u) open = ~s.map[k];
            run = open ? 32u * k + (uint32_t) __builtin_ctz(open) - i : (uint32_t) LRM_PILEUP_TILE - i + ext;
        }
        PileInsAllele a = {0u, 0u, 0u, 0ull};
        if ((emits & LRM_CALL_INS) && ins.K != 0u) a = pile_ins_allele(rule.call, depth, p.n_ins, ins.planes + g, W, ins.K);
        auto put = [&](uint32_t kind) {
            if (!(emits & kind)) return;
            if (at < cap) {
                uint32_t w[12];
                pile_var_record(rule, kind, lo + g, depth, p.n_eq, p.n_del, p.n_ins, p.byte, p.call, run, a, w);
                // (each part pinned in four consecutive registers, as in pileup_sites_kernel)
                pile_u32x4 h0 = {w[0], w[1], w[2], w[3]}, h1 = {w[4], w[5], w[6], w[7]}, h2 = {w[8], w[9], w[10], w[11]};
                asm volatile("" : "+v"(h0), "+v"(h1), "+v"(h2));
                pile_u32x4 *o = reinterpret_cast<pile_u32x4 *>(vars + at);
                o[0] = h0;
                o[1] = h1;
                o[2] = h2;
            }
            ++at;
        };
        put(LRM_CALL_DEL);
        put(LRM_CALL_SNV);
        put(LRM_CALL_INS);
    });
}

// What the read-back and the call stage start with: the sums of the difference plane over the tiles up to the last requested
// position's, and their scan into `bases`.  tile0: the tile of `first`, grid: the tiles that hold a requested position.
struct PileTiles { uint64_t tile0; uint32_t grid, *bases; };
int pile_launch_tile_bases(const lrm_pileup *pl, uint64_t first, uint64_t count, const char *what, hipStream_t st, PileTiles *t) {
    const uint64_t tile_end = (first + count + LRM_PILEUP_TILE - 1) / LRM_PILEUP_TILE;
    *t = {first / LRM_PILEUP_TILE, 0u, pl->d_tiles + pl->n_tiles};
    uint32_t grid_sums;
    if (lrm_grid_1d(tile_end, what, &grid_sums) || lrm_grid_1d(tile_end - t->tile0, what, &t->grid)) return -1;
    hipLaunchKernelGGL(pileup_tile_sums_kernel, dim3(grid_sums), dim3(256), 0, st, pl->d_planes, pl->W, pl->d_tiles);
    hipLaunchKernelGGL(pileup_tile_scan_kernel, dim3(1), dim3(1024), 0, st, pl->d_tiles, tile_end, t->bases);
    return 0;
}

}  // namespace

int lrm_launch_pileup_add(const lrm_pileup *pl, const uint8_t *d_reads, uint64_t stride, const uint32_t *d_lens, const LrmOpRows &b,
                          const lrm_mapq *d_mapq, uint32_t min_mapq, void *stream) {
    if (b.rows == 0) return 0;
    uint32_t grid;
    if (op_rows_grid(b.rows, "pileup", &grid)) return -1;
    const PileWindow win = {pl->lo, pl->hi, pl->W, pl->d_planes};
    if (pl->ins_cols)                                                // the same launch also counts the insertion columns
        hipLaunchKernelGGL(pileup_add_ins_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, d_reads, stride, d_lens, b.store, b.pitch, b.n_ops,
                           b.score, b.meta_r, b.meta, b.rows, d_mapq, min_mapq, win, PileIns{pl->d_ins, pl->ins_cols});
    else
        hipLaunchKernelGGL(pileup_add_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, d_reads, stride, d_lens, b.store, b.pitch, b.n_ops,
                           b.score, b.meta_r, b.meta, b.rows, d_mapq, min_mapq, win);
    HIPCHK(hipGetLastError());
    return 0;
}

// four 16-byte groups per thread until the grid covers the chip a few times over, a grid-stride loop from there on
int lrm_launch_pileup_merge(uint32_t *d_dst, const uint32_t *d_src, uint64_t words, void *stream) {
    if (words == 0) return 0;
    const uint64_t quads = (((uintptr_t) d_dst | (uintptr_t) d_src) & 15u) ? 0u : words / 4u;
    const uint64_t items = quads ? quads : words, blocks = (items + 1023u) / 1024u;
    const uint32_t grid = (uint32_t) (blocks < 1u ? 1u : (blocks > 8192u ? 8192u : blocks));
    hipLaunchKernelGGL(pileup_merge_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, d_dst, d_src, words, quads);
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_pileup_ins_read(const lrm_pileup *pl, uint64_t first, uint64_t count, uint32_t *d_out, void *stream) {
    const uint64_t items = count * pl->ins_cols;
    uint32_t grid;
    if (lrm_grid_1d((items + 255u) / 256u, "pileup insertion read-back", &grid)) return -1;
    hipLaunchKernelGGL(pileup_ins_read_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, pl->d_ins, pl->W, pl->ins_cols, first, items,
                       reinterpret_cast<uint4 *>(d_out));
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_pileup_polish(const lrm_pileup *pl, const PileCallRule &rule, uint64_t first, uint64_t count, uint8_t *d_seq, uint64_t cap,
                             uint64_t *d_len, void *stream) {
    const hipStream_t st = (hipStream_t) stream;
    PileTiles t;
    if (pile_launch_tile_bases(pl, first, count, "pileup polish", st, &t)) return -1;
    uint32_t *n_here = pl->d_call, *rank = pl->d_call + pl->n_tiles;
    const uint8_t *text = (const uint8_t *) pl->idx->view.content + pl->lo;
    const PileIns ins = {pl->d_ins, pl->ins_cols};
    hipLaunchKernelGGL(pileup_polish_count_kernel, dim3(t.grid), dim3(256), 0, st, pl->d_planes, pl->W, t.bases, t.tile0, first, count, text, rule, ins, n_here);
    hipLaunchKernelGGL(pileup_tile_scan_kernel, dim3(1), dim3(1024), 0, st, n_here, (uint64_t) t.grid, rank);
    hipLaunchKernelGGL(pileup_polish_write_kernel, dim3(t.grid), dim3(256), 0, st, pl->d_planes, pl->W, t.bases, t.tile0, first, count, text, rule, ins,
                       n_here, rank, d_seq, cap, d_len);
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_pileup_site_alleles(const lrm_pileup *pl, const PileCallRule &rule, const lrm_pileup_site *d_sites, uint64_t n,
                                   lrm_pileup_ins_allele *d_out, void *stream) {
    uint32_t grid;
    if (lrm_grid_1d((n + 255u) / 256u, "pileup site alleles", &grid)) return -1;
    hipLaunchKernelGGL(pileup_site_alleles_kernel, dim3(grid), dim3(256), 0, (hipStream_t) stream, pl->d_ins, pl->lo, pl->hi, pl->ins_cols, rule,
                       d_sites, n, reinterpret_cast<uint4 *>(d_out));
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_pileup_read(const lrm_pileup *pl, uint64_t first, uint64_t count, lrm_pileup_col *d_out, void *stream) {
    const hipStream_t st = (hipStream_t) stream;
    PileTiles t;
    if (pile_launch_tile_bases(pl, first, count, "pileup read-back", st, &t)) return -1;
    hipLaunchKernelGGL(pileup_cols_kernel, dim3(t.grid), dim3(256), 0, st, pl->d_planes, pl->W, t.bases, t.tile0, first, count, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_pileup_sites(const lrm_pileup *pl, const PileCallRule &rule, uint64_t first, uint64_t count, lrm_pileup_site *d_sites,
                            uint64_t cap, uint64_t *d_n_sites, uint8_t *d_cons, void *stream) {
    const hipStream_t st = (hipStream_t) stream;
    PileTiles t;
    if (pile_launch_tile_bases(pl, first, count, "pileup calls", st, &t)) return -1;
    uint32_t *n_here = pl->d_call, *rank = pl->d_call + pl->n_tiles;
    const uint8_t *text = (const uint8_t *) pl->idx->view.content + pl->lo;
    hipLaunchKernelGGL(pileup_call_kernel, dim3(t.grid), dim3(256), 0, st, pl->d_planes, pl->W, t.bases, t.tile0, first, count, text, rule, d_cons, n_here);
    hipLaunchKernelGGL(pileup_tile_scan_kernel, dim3(1), dim3(1024), 0, st, n_here, (uint64_t) t.grid, rank);
    hipLaunchKernelGGL(pileup_sites_kernel, dim3(t.grid), dim3(256), 0, st, pl->d_planes, pl->W, t.bases, t.tile0, first, count, pl->lo, text, rule,
                       n_here, rank, d_sites, cap, d_n_sites);
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_pileup_variants(const lrm_pileup *pl, const PileVarRule &rule, uint64_t first, uint64_t count, lrm_pileup_variant *d_vars,
                               uint64_t cap, uint64_t *d_n_vars, void *stream) {
    const hipStream_t st = (hipStream_t) stream;
    PileTiles t;
    if (pile_launch_tile_bases(pl, first, count, "pileup variants", st, &t)) return -1;
    uint32_t *n_here = pl->d_call, *rank = pl->d_call + pl->n_tiles, *lead = pl->d_var, *ext = pl->d_var + pl->n_tiles;
    const uint8_t *text = (const uint8_t *) pl->idx->view.content + pl->lo;
    hipLaunchKernelGGL(pileup_var_count_kernel, dim3(t.grid), dim3(256), 0, st, pl->d_planes, pl->W, t.bases, t.tile0, first, count, text, rule.call, n_here, lead);
    hipLaunchKernelGGL(pileup_tile_scan_kernel, dim3(1), dim3(1024), 0, st, n_here, (uint64_t) t.grid, rank);
    hipLaunchKernelGGL(pileup_var_ext_kernel, dim3(1), dim3(1024), 0, st, lead, (uint64_t) t.grid, ext);
    hipLaunchKernelGGL(pileup_var_write_kernel, dim3(t.grid), dim3(256), 0, st, pl->d_planes, pl->W, t.bases, t.tile0, first, count, pl->lo, text, rule,
                       PileIns{pl->d_ins, pl->ins_cols}, n_here, rank, ext, d_vars, cap, d_n_vars);
    HIPCHK(hipGetLastError());
    return 0;
}
