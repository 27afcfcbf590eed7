// SPDX-License-Identifier: MIT
// Bit-sliced GACT for bands of up to 128 diagonals (the default): ONE LANE PER READ, 64 lattice points per word.
// Replaces the reference's per-read simple_gact call (mutils.c:97-103) for large batches; bit-exact
// against oracle/lrm_oracle.c:orc_gact (docs/GACT_SPEC.md).  tests/models/gact_bitslice_model.c is the
// CPU model of exactly this sequence of operations.
//
// Why: the score kernels (gact3_kernel) are bound by VALU issue at ~16 instructions per anti-diagonal
// for 128 lattice points.  The recurrence only needs DIFFERENCES of neighbouring scores, and with the
// +1/-1/-1 scheme those lie in [-1, 2]:
//     V(a,b) = R[a][b] - R[a+1][b],   H(a,b) = R[a][b] - R[a][b+1]          (2-bit code = value + 1)
//     u = H(a+1,b), w = V(a,b+1), s = +-1:   X = max(s, u-1, w-1),  V = X - u,  H = X - w
//     DIAG iff s >= u-1 and s >= w-1, else INS iff u >= w, else DEL          (the spec's tie order)
// so a whole anti-diagonal of the band -- 64 lattice points of one parity -- is four 64-bit bit-planes and
// one step is 2 x 12 boolean operations on them (gact_bs_circuit.h: ten truth tables and the two instructions of
// the base comparison per 32-bit half; two more for the decision planes), independent of the neighbouring
// lanes.  A wavefront advances 64 reads x 64 lattice points per step.
//
//   anti-diagonal s, bit t: diagonal d = 2t - 64 (+1 when s is odd), a = A0 - t, b = B0 + t,
//   A0 = (s + 64 - (s&1)) >> 1, B0 = s - A0.  even s: u = H_prev << 1, w = V_prev; odd s: u = H_prev,
//   w = V_prev >> 1.  The zero shifted in is code 0 (-1): it can never win, which is the band's -inf.
//   Free-exit points (a == tq or b == tt) are forced to V = H = 0 through one-hot "sentinel" planes that
//   travel with the sequence planes.
//
// Sequences are read as bit-planes (planar 2-bit packing, planar_pack_kernels.hip: 32 bases = {lo word, hi word}); the query
// plane of a step is a 64-bit window of the bit-reversed read that slides by one base every second
// step, the target plane a window of the reference sliding the other way -- two v_alignbit per plane,
// with wave-uniform shift amounts.
//
// Traceback without storing 2 x 64 bits per step and read: pass 1 runs the tile from its far corner
// to the anchor and keeps the four difference planes at every 32nd anti-diagonal below 2(T-O) in LDS
// (32 B per lane and checkpoint).  Pass 2 takes the 32-step blocks in walk order: recompute the block
// from its checkpoint with the decision planes kept in registers, then walk through it -- every lane
// follows its own path with the steps predicated on "my path is on this anti-diagonal" (the walk's bookkeeping:
// gact_bs_circuit.h, bs_walk_block).  The only reader of a block's decisions is the lane's own walk, which stays
// within k diagonals of where it entered after k anti-diagonals: 32 lattice points per anti-diagonal, closed under
// the recurrence.  So a block with no free-exit point near the band (and the full band, W = 128) is recomputed
// and walked on ONE 32-bit word per plane, cut out of the checkpoint and the sequence windows around the lane's
// entry point (gact_bs_circuit.h, bs_win_block / bs_walk_block_win); the other blocks keep the full-width masked step.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "lrm_hip_util.h"
#include "extend_stage.h"
#include "gact_bs_circuit.h"    // BS_K, the difference circuit, the walk's bookkeeping
#include "base_words.h"         // ops4: four CIGAR bytes per permute

#define BS_H (BS_K / 2)
#define LRM_BS_MAX_WAVES 2048ull  // 2 per SIMD on 256 CUs
#define BS_PADW LRM_BS_PADW
#define BS_NO_EXIT 0x40000000   // tq, tt of a lane without a tile: no stream word holds its free-exit point

struct __attribute__((aligned(8))) BsPair { uint64_t a, b; };

__device__ __forceinline__ uint32_t bs_alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
    return __builtin_amdgcn_alignbit(hi, lo, sh);
}
__device__ __forceinline__ uint32_t bs_onehot(int x) { return (uint32_t) x < 32u ? (1u << x) : 0u; }

// ----------------------------------------------------------------------------------------
// per-lane tile context and sequence streams
// ----------------------------------------------------------------------------------------
struct BsTile {
    const uint64_t *qpl;      // planar read, word 0
    const uint64_t *dpl;      // planar reference text, word 0
    int64_t dpos;             // loc + j: text position of the tile's anchor
    int32_t i;                // read position of the tile's anchor
    int32_t tq, tt;
};

struct BsWord { uint32_t lo, hi, sent; };

// stream word whose bit b holds read base a_hi - b (the read runs backwards through the planes):
// a 16-byte gather of two adjacent planar words, then a funnel shift by the lane's own alignment
__device__ __forceinline__ BsPair bs_q_raw(const BsTile &t, int a_hi) {
    BsPair p;
    __builtin_memcpy(&p, t.qpl + ((t.i + a_hi - 31) >> 5), sizeof(p));
    return p;
}
// SENT: with the one-hot word of the free-exit point (a == tq); a block on the window needs none
template <bool SENT = true>
__device__ __forceinline__ BsWord bs_q_conv(const BsTile &t, int a_hi, const BsPair &p) {
    const uint32_t sh = (uint32_t) (t.i + a_hi - 31) & 31u;
    BsWord w;
    w.lo = __builtin_bitreverse32(bs_alignbit((uint32_t) p.b, (uint32_t) p.a, sh));
    w.hi = __builtin_bitreverse32(bs_alignbit((uint32_t) (p.b >> 32), (uint32_t) (p.a >> 32), sh));
    w.sent = SENT ? bs_onehot(a_hi - t.tq) : 0u;
    return w;
}
__device__ __forceinline__ BsWord bs_q_word(const BsTile &t, int a_hi) { return bs_q_conv(t, a_hi, bs_q_raw(t, a_hi)); }
// word whose bit b holds text base b_lo + b
__device__ __forceinline__ BsPair bs_d_raw(const BsTile &t, int b_lo) {
    BsPair p;
    __builtin_memcpy(&p, t.dpl + ((t.dpos + b_lo) >> 5), sizeof(p));
    return p;
}
template <bool SENT = true>
__device__ __forceinline__ BsWord bs_d_conv(const BsTile &t, int b_lo, const BsPair &p) {
    const uint32_t sh = (uint32_t) (t.dpos + b_lo) & 31u;
    BsWord w;
    w.lo = bs_alignbit((uint32_t) p.b, (uint32_t) p.a, sh);
    w.hi = bs_alignbit((uint32_t) (p.b >> 32), (uint32_t) (p.a >> 32), sh);
    w.sent = SENT ? bs_onehot(t.tt - b_lo) : 0u;
    return w;
}
__device__ __forceinline__ BsWord bs_d_word(const BsTile &t, int b_lo) { return bs_d_conv(t, b_lo, bs_d_raw(t, b_lo)); }

struct BsStream {
    BsWord q0, q1, q2, d0, d1, d2;     // three consecutive stream words each
    BsPl Qlo, Qhi, Qs, Dlo, Dhi, Ds;
    BsPl bandE, bandO;                 // lattice points inside the band on even / odd anti-diagonals (all ones for W = 128)
    bool narrow;                       // W < 128: every step takes the masked (BOUND) form
    int qnext, dnext;                  // wave-uniform: a of bit 0 of the next query word / b of the next (lower) text word
};

template <bool BOUND>
__device__ __forceinline__ void bs_extract_q(BsStream &st, uint32_t shq) {
    st.Qlo.lo = bs_alignbit(st.q1.lo, st.q0.lo, shq);  st.Qlo.hi = bs_alignbit(st.q2.lo, st.q1.lo, shq);
    st.Qhi.lo = bs_alignbit(st.q1.hi, st.q0.hi, shq);  st.Qhi.hi = bs_alignbit(st.q2.hi, st.q1.hi, shq);
    if (BOUND) { st.Qs.lo = bs_alignbit(st.q1.sent, st.q0.sent, shq); st.Qs.hi = bs_alignbit(st.q2.sent, st.q1.sent, shq); }
}
template <bool BOUND>
__device__ __forceinline__ void bs_extract_d(BsStream &st, uint32_t shd) {
    st.Dlo.lo = bs_alignbit(st.d1.lo, st.d0.lo, shd);  st.Dlo.hi = bs_alignbit(st.d2.lo, st.d1.lo, shd);
    st.Dhi.lo = bs_alignbit(st.d1.hi, st.d0.hi, shd);  st.Dhi.hi = bs_alignbit(st.d2.hi, st.d1.hi, shd);
    if (BOUND) { st.Ds.lo = bs_alignbit(st.d1.sent, st.d0.sent, shd); st.Ds.hi = bs_alignbit(st.d2.sent, st.d1.sent, shd); }
}
// windows for anti-diagonal s; the text window starts room_d bases into its words
__device__ __forceinline__ void bs_stream_init(BsStream &st, const BsTile &t, int s, int room_d) {
    const int A0 = (s + 64 - (s & 1)) >> 1, B0 = s - A0;
    st.q0 = bs_q_word(t, A0);
    st.q1 = bs_q_word(t, A0 - 32);
    st.q2 = bs_q_word(t, A0 - 64);
    st.d0 = bs_d_word(t, B0 - room_d);
    st.d1 = bs_d_word(t, B0 - room_d + 32);
    st.d2 = bs_d_word(t, B0 - room_d + 64);
    st.qnext = A0 - 96;
    st.dnext = B0 - room_d - 32;
    bs_extract_q<true>(st, 0);
    bs_extract_d<true>(st, (uint32_t) room_d);
}
// does any lane hold a free-exit point in its current stream words?  (wave-uniform)
__device__ __forceinline__ bool bs_any_sentinel(const BsStream &st) {
    if (st.narrow) return true;
    return __ballot((st.q0.sent | st.q1.sent | st.q2.sent | st.d0.sent | st.d1.sent | st.d2.sent) != 0u) != 0ull;
}

struct BsState { BsPl V1, V0, H1, H0; };

// one 32-bit half of an anti-diagonal: u = H of the lower neighbour, w = V of the upper one (gact_bs_circuit.h)
template <bool BOUND, bool TRACK>
__device__ __forceinline__ void bs_half(uint32_t u1, uint32_t u0, uint32_t w1, uint32_t w0, uint32_t ql, uint32_t qh,
                                        uint32_t dl, uint32_t dh, uint32_t bm, uint32_t band, uint32_t &V1, uint32_t &V0,
                                        uint32_t &H1, uint32_t &H0, uint32_t &N, uint32_t &G) {
    const BsHalf o = bs_half_circuit(BOUND, TRACK, u1, u0, w1, w0, ql, qh, dl, dh, bm, band);
    V1 = o.V1; V0 = o.V0; H1 = o.H1; H0 = o.H0;
    if (TRACK) { N = o.N; G = o.G; }
}

// one anti-diagonal.  TRACK: also produce the decision planes
template <bool ODD, bool BOUND, bool TRACK>
__device__ __forceinline__ void bs_step(BsState &x, const BsStream &st, BsPl &N, BsPl &G) {
    BsPl u1, u0, w1, w0;
    if (!ODD) {                        // u = H << 1 (the lowest lattice point has no insertion neighbour in the band)
        u1.lo = x.H1.lo << 1; u1.hi = bs_alignbit(x.H1.hi, x.H1.lo, 31);
        u0.lo = x.H0.lo << 1; u0.hi = bs_alignbit(x.H0.hi, x.H0.lo, 31);
        w1 = x.V1; w0 = x.V0;
    } else {                           // w = V >> 1 (the highest one has no deletion neighbour)
        u1 = x.H1; u0 = x.H0;
        w1.lo = bs_alignbit(x.V1.hi, x.V1.lo, 1); w1.hi = x.V1.hi >> 1;
        w0.lo = bs_alignbit(x.V0.hi, x.V0.lo, 1); w0.hi = x.V0.hi >> 1;
    }
    const uint32_t bl = BOUND ? (st.Qs.lo | st.Ds.lo) : 0u, bh = BOUND ? (st.Qs.hi | st.Ds.hi) : 0u;
    const BsPl &band = ODD ? st.bandO : st.bandE;
    bs_half<BOUND, TRACK>(u1.lo, u0.lo, w1.lo, w0.lo, st.Qlo.lo, st.Qhi.lo, st.Dlo.lo, st.Dhi.lo, bl, band.lo,
                          x.V1.lo, x.V0.lo, x.H1.lo, x.H0.lo, N.lo, G.lo);
    bs_half<BOUND, TRACK>(u1.hi, u0.hi, w1.hi, w0.hi, st.Qlo.hi, st.Qhi.hi, st.Dlo.hi, st.Dhi.hi, bh, band.hi,
                          x.V1.hi, x.V0.hi, x.H1.hi, x.H0.hi, N.hi, G.hi);
}

__device__ __forceinline__ void bs_ckpt_store(uint32_t *ckl, int s, const BsState &x) {   // ckl: the wavefront's checkpoints + lane
    uint32_t *c_ = ckl + (size_t) (s / BS_K - 1) * 512;
    c_[0] = x.V1.lo; c_[64] = x.V1.hi; c_[128] = x.V0.lo; c_[192] = x.V0.hi;
    c_[256] = x.H1.lo; c_[320] = x.H1.hi; c_[384] = x.H0.lo; c_[448] = x.H0.hi;
}

// np step pairs of pass 1 between two events (a stream refill, the tile's last anti-diagonal): nothing but the two steps,
// the two window shifts and a checkpoint store where one is due, HB fixed, in a loop of its own -- in one loop with the
// events the compiler rotates the stream words through copies on every pair (31 v_mov of 95 instructions,
// profiles/r5/README.md)
template <bool HB>
__device__ __forceinline__ void bs_pass1_pairs(BsState &x, BsStream &st, uint32_t &shq, uint32_t &shd, int &s, int &ck_s,
                                               uint32_t *ckl, int np) {
    BsPl nN, nG;
    // the two shifts and the anti-diagonal are wave-uniform and are counted in scalar registers here, wherever the code
    // around this loop keeps them (short of scalar registers it holds them in vector ones: one v_add more per pair)
    shq = (uint32_t) __builtin_amdgcn_readfirstlane((int) shq);
    shd = (uint32_t) __builtin_amdgcn_readfirstlane((int) shd);
#pragma nounroll
    for (int k = 0; k < np; ++k) {
        bs_step<false, HB, false>(x, st, nN, nG);
        if (s == ck_s) { bs_ckpt_store(ckl, s, x); ck_s -= BS_K; }
        ++shq;
        bs_extract_q<HB>(st, shq);
        bs_step<true, HB, false>(x, st, nN, nG);
        --shd;
        bs_extract_d<HB>(st, shd);
        s -= 2;
    }
}

__device__ __forceinline__ int bs_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ uint32_t bs_wave_or(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t) __shfl_xor((int) v, o);
    return (uint32_t) __builtin_amdgcn_readfirstlane((int) v);
}

// Which traceback blocks of a tile run in full width, bit c for block c (at most 32 blocks: T - O <= 512), decided once per
// tile by the rule bs_any_sentinel applies to a block's stream words: some lane holds a free-exit point in the six words of
// block c.  Those cover a = BS_H c - 48 .. BS_H c + 47 of the read and b = BS_H c - 32 .. BS_H c + 63 of the text
// (bs_block_prefetch), so tq puts blocks ceil((tq - 47) / BS_H) .. floor((tq + 48) / BS_H) in full width and tt blocks
// ceil((tt - 63) / BS_H) .. floor((tt + 32) / BS_H).  BS_NO_EXIT gives an empty range.
__device__ __forceinline__ uint32_t bs_block_range(int lo, int hi) {      // bits max(lo, 0) .. min(hi, 31)
    lo = max(lo, 0); hi = min(hi, 31);
    return lo <= hi ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}
__device__ __forceinline__ uint32_t bs_full_blocks(int tq, int tt, bool narrow) {
    static_assert(BS_H == 16, "the block ranges below divide by BS_H as a shift by 4");
    if (narrow) return ~0u;
    return bs_wave_or(bs_block_range((tq - 32) >> 4, (tq + 48) >> 4) | bs_block_range((tt - 48) >> 4, (tt + 32) >> 4));
}

// ----------------------------------------------------------------------------------------
// the kernel: one wavefront per workgroup, lane = read
// ----------------------------------------------------------------------------------------
// everything a traceback block needs from memory, fetched one block ahead (during the previous walk).  The three stream
// words of a sequence are cut from four consecutive planar words, each fetched once: q[j] is planar word
// ((i + A0 - 31) >> 5) - 2 + j of the read, d[j] word ((dpos + b_lo) >> 5) + j of the text.
struct BsBlockRaw { uint64_t q[4], d[4]; uint32_t ck[8]; };

__device__ __forceinline__ void bs_block_prefetch(BsBlockRaw &raw, const BsTile &t, int c, const uint32_t *ckw, int lane) {
    const int A0 = BS_H * (c + 1) + 31, b_lo = BS_H * c - 32;      // anti-diagonal K(c+1)-1: A0, and B0 - K/2
    const uint64_t *qp = t.qpl + (((t.i + A0 - 31) >> 5) - 2), *dp = t.dpl + ((t.dpos + b_lo) >> 5);
#pragma unroll
    for (int e = 0; e < 4; ++e) { raw.q[e] = qp[e]; raw.d[e] = dp[e]; }
    const uint32_t *cp = ckw + (size_t) c * 512 + lane;      // checkpoint c+1 = state after anti-diagonal K(c+1)
#pragma unroll
    for (int e = 0; e < 8; ++e) raw.ck[e] = cp[64 * e];
}
// the pair of planar words that holds stream word e of the read (e = 0: the one at A0) or of the text (the one at b_lo)
__device__ __forceinline__ BsPair bs_raw_q(const BsBlockRaw &raw, int e) { return BsPair{raw.q[2 - e], raw.q[3 - e]}; }
__device__ __forceinline__ BsPair bs_raw_d(const BsBlockRaw &raw, int e) { return BsPair{raw.d[e], raw.d[e + 1]}; }

// COUNT: the counting build (lrm_workspace_set_counting; bookkeeping, never in a timed region) adds up, per wavefront,
// which path every pass-1 step pair and every pass-2 block took (LrmDevCounters::bs_count, LRM_BSC_*)
template <bool COUNT>
__global__ __launch_bounds__(64) void gact_bs_kernel(const uint64_t *__restrict__ qpl, uint64_t wpr,
                                                     const uint32_t *__restrict__ lens,
                                                     const lrm_seq_meta *__restrict__ meta,
                                                     const int32_t *__restrict__ meta_r,
                                                     const uint64_t *__restrict__ cpl,
                                                     const uint32_t *__restrict__ tlens,
                                                     const uint32_t *__restrict__ rflags, uint64_t n_reads,
                                                     int T, int O, int W, uint32_t *__restrict__ ckpt,
                                                     uint64_t *__restrict__ codes, uint64_t cw,
                                                     int32_t *__restrict__ n_codes_out,
                                                     int32_t *__restrict__ n_ops_out,
                                                     int32_t *__restrict__ score_out, LrmDevCounters *counters) {
    const int lane = threadIdx.x;
    // Lanes take reads from a queue (one atomic per wavefront and refill): reads of very different
    // lengths share a wavefront without the short ones idling behind the longest, and a grid of a few
    // resident wavefronts per SIMD serves any batch size.
    unsigned long long *queue = &counters->bs_queue;
    uint64_t r = 0;
    bool alive = false, exhausted = false;
    int n = 0, m = 0;
    int64_t loc = 0;
    uint64_t *cout = codes;                                     // 2-bit CIGAR codes, 32 per word
    BsTile t;
    t.qpl = qpl + BS_PADW;
    t.dpl = cpl;

    const int cap = T - O, lim2 = 2 * cap;
    const int nblk = (lim2 + BS_K - 1) / BS_K;
    uint32_t *ckw = ckpt + (size_t) blockIdx.x * (size_t) nblk * 512;   // this wavefront's checkpoints (L2-resident scratch)
    // band -W/2 <= b - a <= W/2 - 1 as bit ranges of the planes (even: d = 2t - 64, odd: d = 2t - 63)
    const int hw = W / 2;
    const uint64_t bandE64 = bit_range<uint64_t>((65 - hw) >> 1, ((63 + hw) >> 1) + 1);
    const uint64_t bandO64 = bit_range<uint64_t>((64 - hw) >> 1, ((62 + hw) >> 1) + 1);
    int i = 0, j = 0, cnt = 0, score = 0;
    uint64_t sb = 0;               // code stream buffer: `fill` bits used
    int fill = 0, widx = 0;
    uint64_t pend = 0;             // a full code word whose store is delayed past the next block's loads
    bool has_pend = false;
    unsigned tiles = 0;
    unsigned nc[LRM_BSC_N] = {};   // COUNT only; wave-uniform

    while (true) {
        if (alive && (score < 0 || !(i < n && j < m))) {          // this lane's read is finished: write it out
            if (has_pend) { cout[widx++] = pend; has_pend = false; }
            if (fill > 0) cout[widx] = sb;
            const int rest = score >= 0 ? n - i : 0;               // text exhausted: the expansion appends 'I's
            n_codes_out[r] = score >= 0 ? cnt : 0;
            n_ops_out[r] = score >= 0 ? cnt + rest : 0;
            score_out[r] = score >= 0 ? score + rest : score;
            alive = false;
        }
        // refill idle lanes from the queue
        while (true) {
            const bool need = !alive && !exhausted;
            const uint64_t needmask = __ballot(need);
            if (needmask == 0) break;
            if (COUNT) nc[LRM_BSC_REFILLS]++;
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(queue, (unsigned long long) __popcll(needmask));
            base = __shfl(base, 0);
            if (need) {
                r = base + (uint64_t) __popcll(needmask & ((1ull << lane) - 1ull));
                if (r >= n_reads) {
                    exhausted = true;
                } else if (meta_r[r] == 0) {                       // fenced: no extension
                    n_ops_out[r] = 0; score_out[r] = -1; n_codes_out[r] = 0;
                } else if (!(rflags && rflags[r])) {               // flagged reads belong to the byte kernel
                    n = (int) lens[r];
                    m = tlens ? (int) tlens[r] : n;
                    loc = (int64_t) meta[r].loc;
                    cout = codes + r * cw;
                    t.qpl = qpl + r * wpr + BS_PADW;
                    i = j = cnt = score = 0;
                    sb = 0; fill = 0; widx = 0;
                    alive = true;
                    if (!(n > 0 && m > 0)) {                       // nothing to align: only the 'I' tail
                        n_codes_out[r] = 0; n_ops_out[r] = n; score_out[r] = n;
                        alive = false;
                    }
                }
            }
        }
        const bool act = alive;
        const uint64_t actmask = __ballot(act);
        if (actmask == 0) break;
        tiles += (unsigned) __popcll(actmask);
        if (COUNT) nc[LRM_BSC_WAVE_TILES]++;
        t.i = i;
        t.dpos = loc + j;
        const int tq = act ? min(T, n - i) : 0, tt = act ? min(T, m - j) : 0;
        // A lane without a tile (batch exhausted, read finished, fenced or flagged) carries no free-exit point: with
        // tq = tt = 0 it would hold one in the stream words near the anchor and put its whole wavefront on the masked
        // step and on full-width blocks, for planes nobody reads.  BS_NO_EXIT is out of bs_onehot's reach for every
        // a_hi and b_lo of a tile (|a_hi|, |b_lo| < 2^12).
        t.tq = act ? tq : BS_NO_EXIT;
        t.tt = act ? tt : BS_NO_EXIT;
        const bool last = i + tq == n;
        const int S0 = ((bs_wave_max(tq + tt) + BS_K - 1) / BS_K) * BS_K;
        const int nb = min(nblk, S0 / BS_K);

        BsState x = {{0u, 0u}, {~0u, ~0u}, {0u, 0u}, {~0u, ~0u}};
        BsStream st;
        st.bandE.lo = (uint32_t) bandE64; st.bandE.hi = (uint32_t) (bandE64 >> 32);
        st.bandO.lo = (uint32_t) bandO64; st.bandO.hi = (uint32_t) (bandO64 >> 32);
        st.narrow = W < 128;
        BsPl nN, nG;
        // ---- pass 1: differences only, checkpoints at the block boundaries ----
        bs_stream_init(st, t, S0, 31);
        BsPair pq = bs_q_raw(t, st.qnext), pd = bs_d_raw(t, st.dnext);      // next stream words, one refill ahead
        uint32_t shq = 0, shd = 31;
        bool hb = bs_any_sentinel(st);
        int ck_s = nb * BS_K;                                      // next anti-diagonal whose state is kept
        for (int s = S0;;) {
            // a pair with an event: the way out after the even step, the refills around the odd one
            if (COUNT) { if (hb) nc[LRM_BSC_P1_MASKED]++; else nc[LRM_BSC_P1_PLAIN]++; }
            if (hb) bs_step<false, true, false>(x, st, nN, nG); else bs_step<false, false, false>(x, st, nN, nG);
            if (s == ck_s) { bs_ckpt_store(ckw + lane, s, x); ck_s -= BS_K; }
            if (s == BS_K) break;
            if (++shq == 32) {
                st.q0 = st.q1; st.q1 = st.q2; st.q2 = bs_q_conv(t, st.qnext, pq);
                st.qnext -= 32;
                pq = bs_q_raw(t, st.qnext);
                shq = 0;
                hb = bs_any_sentinel(st);
                if (hb) bs_extract_d<true>(st, shd);          // the text sentinel window may not be current
            }
            if (hb) {
                bs_extract_q<true>(st, shq);
                bs_step<true, true, false>(x, st, nN, nG);
            } else {
                bs_extract_q<false>(st, shq);
                bs_step<true, false, false>(x, st, nN, nG);
            }
            if (shd == 0) {
                st.d2 = st.d1; st.d1 = st.d0; st.d0 = bs_d_conv(t, st.dnext, pd);
                st.dnext -= 32;
                pd = bs_d_raw(t, st.dnext);
                shd = 32;
                hb = bs_any_sentinel(st);
                if (hb) bs_extract_q<true>(st, shq);          // the query sentinel window may not be current
            }
            --shd;
            if (hb) bs_extract_d<true>(st, shd); else bs_extract_d<false>(st, shd);
            s -= 2;
            // the pairs up to the next event: ++shq stays below 32, shd above 0, s above the last anti-diagonal
            const int np = min(min(31 - (int) shq, (int) shd), (s - BS_K) >> 1);
            if (COUNT) { if (hb) nc[LRM_BSC_P1_MASKED] += (unsigned) np; else nc[LRM_BSC_P1_PLAIN] += (unsigned) np; }
            if (hb) bs_pass1_pairs<true>(x, st, shq, shd, s, ck_s, ckw + lane, np);
            else bs_pass1_pairs<false>(x, st, shq, shd, s, ck_s, ckw + lane, np);
        }
        // ---- pass 2: per block recompute with decision planes, then walk through the block ----
        // the walk keeps at most T-O bases of either sequence; in the read's last tile it may run on to the edge
        // but not past anti-diagonal 2(T-O) (docs/GACT_SPEC.md)
        const int amax = last ? tq : min(tq, cap), bmax = last ? tt : min(tt, cap);
        BsWalk wk = {act ? -amax : 0, act ? -bmax : 0, act ? -lim2 : 0, score};
        BsBlockRaw raw;
        bs_block_prefetch(raw, t, 0, ckw, lane);
        const uint32_t fullmask = bs_full_blocks(t.tq, t.tt, st.narrow);
        for (int c = 0; c < nb; ++c) {
            if (__ballot(bs_walk_running(&wk)) == 0) { if (COUNT) nc[LRM_BSC_P2_SKIPPED] += (unsigned) (nb - c); break; }
            const int A0 = BS_H * (c + 1) + 31, b_lo = BS_H * c - 32;
            // A free-exit point near the band, or a band narrower than the planes (wave-uniform, bs_full_blocks): the block in
            // full width with the masked step.  Every other block on the 32 points per anti-diagonal that the lane's walk can
            // reach from where it stands (gact_bs_circuit.h); lanes that do not walk compute something nobody reads.
            const bool full = (fullmask >> c) & 1u;
            if (COUNT) { if (full) nc[LRM_BSC_P2_FULL]++; else nc[LRM_BSC_P2_WINDOWED]++; }
            const int32_t boff = bmax - BS_H * c + 32;
            // walk: the lane's path crosses each anti-diagonal at most once; codes 0 X, 1 =, 2 I, 3 D.
            // Branch-free: every step runs in all lanes, gated by "my path is on this anti-diagonal".
            // Either form takes what it needs out of `raw`, fetches the next block's words and checkpoint a block ahead (the
            // tile's last block fetches itself again: one fetch in either form, no path on which `raw` stays as it is) and
            // sends the previous block's full code word out behind those loads, which it must not delay.
            uint32_t e2;
            uint64_t bw;
            if (full) {
                st.q0 = bs_q_conv(t, A0, bs_raw_q(raw, 0)); st.q1 = bs_q_conv(t, A0 - 32, bs_raw_q(raw, 1)); st.q2 = bs_q_conv(t, A0 - 64, bs_raw_q(raw, 2));
                st.d0 = bs_d_conv(t, b_lo, bs_raw_d(raw, 0)); st.d1 = bs_d_conv(t, b_lo + 32, bs_raw_d(raw, 1)); st.d2 = bs_d_conv(t, b_lo + 64, bs_raw_d(raw, 2));
                x.V1.lo = raw.ck[0]; x.V1.hi = raw.ck[1]; x.V0.lo = raw.ck[2]; x.V0.hi = raw.ck[3];
                x.H1.lo = raw.ck[4]; x.H1.hi = raw.ck[5]; x.H0.lo = raw.ck[6]; x.H0.hi = raw.ck[7];
                bs_extract_q<true>(st, 0);
                bs_extract_d<true>(st, BS_H);
                BsPl N[BS_K], G[BS_K];
#pragma unroll
                for (int k = BS_K - 1; k >= 1; k -= 2) {
                    bs_step<true, true, true>(x, st, N[k], G[k]);
                    bs_extract_d<true>(st, (uint32_t) ((k - 1) >> 1));                 // K/2-1 .. 0
                    bs_step<false, true, true>(x, st, N[k - 1], G[k - 1]);
                    if (k > 1) bs_extract_q<true>(st, (uint32_t) (BS_H - ((k - 1) >> 1)));   // 1 .. K/2-1
                }
                if (has_pend) { cout[widx++] = pend; has_pend = false; }
                bw = bs_walk_block(&wk, N, G, BS_K * c, lim2, boff, &e2);
                // Beside the 128 words of the planes there is no room for the next block's 24 (256 VGPRs: two wavefronts per
                // SIMD), so here they are fetched behind the walk.  The addresses are made to depend on the walk's result
                // through an empty asm; without it the compiler moves the loads up to the block's start and the arm needs
                // 266 registers (256 VGPRs + 10 AGPRs, one wavefront per SIMD); with the fetch tied between the recompute
                // and the walk instead, 381.  If a compiler update changes `.vgpr_count` of this kernel, look here first.
                {
                    BsTile tn = t;
                    int ln = lane;
                    asm volatile("" : "+v"(tn.i), "+v"(tn.dpos), "+v"(ln) : "v"(e2));
                    bs_block_prefetch(raw, tn, min(c + 1, nb - 1), ckw, ln);
                }
            } else {
                const uint32_t o = bs_win_origin(wk.nb + boff);
                BsWinIn win;
                {
                    const BsWord q0 = bs_q_conv<false>(t, A0, bs_raw_q(raw, 0)), q1 = bs_q_conv<false>(t, A0 - 32, bs_raw_q(raw, 1)),
                                 q2 = bs_q_conv<false>(t, A0 - 64, bs_raw_q(raw, 2));
                    const BsWord d0 = bs_d_conv<false>(t, b_lo, bs_raw_d(raw, 0)), d1 = bs_d_conv<false>(t, b_lo + 32, bs_raw_d(raw, 1)),
                                 d2 = bs_d_conv<false>(t, b_lo + 64, bs_raw_d(raw, 2));
                    bs_win_cut_ck(&win, raw.ck, o);
                    bs_win_cut_seq(win.ql, q0.lo, q1.lo, q2.lo, o); bs_win_cut_seq(win.qh, q0.hi, q1.hi, q2.hi, o);
                    bs_win_cut_seq(win.dl, d0.lo, d1.lo, d2.lo, o); bs_win_cut_seq(win.dh, d0.hi, d1.hi, d2.hi, o);
                }
                bs_block_prefetch(raw, t, min(c + 1, nb - 1), ckw, lane);
                if (has_pend) { cout[widx++] = pend; has_pend = false; }
                uint32_t N[BS_K], G[BS_K];
                bs_win_block(&win, N, G);
                bw = bs_walk_block_win(&wk, N, G, BS_K * c, lim2, boff, o, &e2);
            }
            // append the block's codes (at most 32) to the lane's code stream
            sb |= bw << fill;
            cnt += (int) (e2 >> 1);
            if (fill + (int) e2 >= 64) {
                pend = sb; has_pend = true;
                sb = (bw >> 1) >> (63 - fill);
                fill -= 64;
            }
            fill += (int) e2;
        }
        if (act) {
            const int a = wk.na + amax, b = wk.nb + bmax;
            score = wk.score;
            i += a;
            j += b;
            if (a + b == 0) score = -1;                           // cannot happen (every walk moves); never spin
        }
    }
    if (lane == 0 && tiles) atomicAdd(&counters->gact_tiles, (unsigned long long) tiles);
    if (COUNT && lane < LRM_BSC_N) {
        unsigned v = 0;
#pragma unroll
        for (int e = 0; e < LRM_BSC_N; ++e) v = lane == e ? nc[e] : v;
        atomicAdd(&counters->bs_count[lane], (unsigned long long) v);
    }
}

// codes -> CIGAR bytes ('=' 'X' 'I' 'D', one per alignment column): one thread per code word -- 32 columns, the word
// loaded once -- in two halves of 16 columns (one 16-byte store each when the row is 16-byte aligned, four 4-byte stores
// otherwise, single bytes at the row's end).  Four columns per permute (ops4, base_words.h) and no compare per column: the
// one dword that holds the end of the coded columns, and the dwords behind it, take their 'I's by a byte mask.
// (One thread per 16 columns -- five workgroups per read instead of three on the bench workload, every code word loaded
// by two threads -- took 0.63 ms per Gbp against 0.50, with 85 vector instructions per wavefront as with 32: profiles/r10.)
// bs_ops4: the per-column form that ops4 and ops4_tail replaced in the kernel
__device__ __forceinline__ uint32_t bs_ops4(uint32_t c8, int o, int nc) {
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t op = o + e < nc ? __builtin_amdgcn_ubfe(0x44493d58u, ((c8 >> (2 * e)) & 3u) * 8u, 8u) : (uint32_t) 'I';
        w |= op << (8 * e);
    }
    return w;
}
// 16 columns from c32; left (> 0) columns and left_c coded columns of the row begin at out
__device__ __forceinline__ void bs_expand16(uint32_t c32, int left, int left_c, uint8_t *out) {
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = ops4((c32 >> (8 * q)) & 0xffu);
    if (left_c < 16) {                                           // the 'I' tail begins in these 16 columns or before them
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = ops4_tail(w[q], bw_keep(left_c > 4 * q ? (uint32_t) (left_c - 4 * q) : 0u));
    }
    if (left >= 16 && (((uintptr_t) out) & 15u) == 0) {
        *reinterpret_cast<uint4 *>(out) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (4 * q + 4 <= left) *reinterpret_cast<uint32_t *>(out + 4 * q) = w[q];
            else for (int e = 0; 4 * q + e < left; ++e) out[4 * q + e] = (uint8_t) (w[q] >> (8 * e));
        }
    }
}
__global__ __launch_bounds__(256) void bs_expand_kernel(const uint64_t *__restrict__ codes, uint64_t cw,
                                                        const int32_t *__restrict__ n_codes,
                                                        const int32_t *__restrict__ n_ops,
                                                        const uint32_t *__restrict__ rflags,
                                                        const int32_t *__restrict__ meta_r, uint64_t n_reads,
                                                        uint32_t blocks_per_read, uint8_t *__restrict__ store,
                                                        uint64_t store_stride) {
    const uint64_t r = blockIdx.x / blocks_per_read;
    if (r >= n_reads) return;
    if (meta_r[r] == 0 || (rflags && rflags[r])) return;         // fenced, or written by the byte kernel
    const int no = n_ops[r], nc = n_codes[r];
    const uint32_t cwi = (blockIdx.x % blocks_per_read) * 256 + threadIdx.x;      // this thread's code word
    const int o = (int) cwi * 32;
    if (o >= no) return;
    const uint64_t c64 = codes[r * cw + cwi];
    uint8_t *out = store + r * store_stride + o;
    bs_expand16((uint32_t) c64, no - o, nc - o, out);
    if (o + 16 < no) bs_expand16((uint32_t) (c64 >> 32), no - o - 16, nc - o - 16, out + 16);
}

// ----------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------
uint64_t lrm_bs_code_words(uint32_t max_len) { return (2ull * max_len + 31) / 32 + 2; }
uint64_t lrm_bs_ckpt_words(uint64_t n) {                     // T - O <= 512: at most 1024/K blocks per wavefront
    uint64_t waves = (n + 63) / 64;
    if (waves > LRM_BS_MAX_WAVES) waves = LRM_BS_MAX_WAVES;
    return waves * (uint64_t) (1024 / BS_K) * 512ull;
}

int lrm_bs_scratch_alloc(LrmBsScratch *s, uint64_t jobs, uint32_t max_len, uint32_t ops_len, uint64_t *bytes) {
    s->wpr = lrm_bs_planar_words(max_len);
    s->cw = lrm_bs_code_words(ops_len);
    const LrmDevAlloc allocs[] = {
        {(void **) &s->qpl, jobs * s->wpr * 8 + 16},
        {(void **) &s->rflags, jobs * 4},
        {(void **) &s->ckpt, lrm_bs_ckpt_words(jobs) * 4},
        {(void **) &s->codes, jobs * s->cw * 8},
        {(void **) &s->ncodes, jobs * 4},
    };
    if (lrm_dev_alloc_table(allocs, "bytes of bit-sliced extension scratch", bytes)) { lrm_bs_scratch_free(s); return -1; }
    return 0;
}

void lrm_bs_scratch_free(LrmBsScratch *s) {
    lrm_dev_free({s->qpl, s->rflags, s->ckpt, s->codes, s->ncodes});
    *s = LrmBsScratch{};
}

int lrm_bs_launch(const LrmGactJobs &j, lrm_gact_params gp, const LrmBsScratch &bs, LrmDevCounters *counters,
                  uint32_t max_waves, bool count, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    uint64_t blocks = (j.n + 63) / 64;
    if (blocks > LRM_BS_MAX_WAVES) blocks = LRM_BS_MAX_WAVES;              // resident wavefronts; lanes refill from the queue
    if (max_waves >= 1 && max_waves < blocks) blocks = max_waves;          // (tests: a small grid forces refills)
    HIPCHK(hipMemsetAsync(&counters->bs_queue, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(count ? gact_bs_kernel<true> : gact_bs_kernel<false>, dim3((uint32_t) blocks), dim3(64), 0, stream,
                       bs.qpl, bs.wpr, j.lens, j.meta, j.meta_r, j.cpl + BS_PADW, j.tlens, bs.rflags, j.n, gp.T, gp.O, gp.W,
                       bs.ckpt, bs.codes, bs.cw, bs.ncodes, j.n_ops, j.score, counters);
    const uint32_t bpr = (uint32_t) ((bs.cw + 255) / 256);                  // 256 threads x one code word per block
    uint32_t grid;
    if (lrm_grid_1d(j.n * bpr, "expand", &grid)) return -1;
    hipLaunchKernelGGL(bs_expand_kernel, dim3(grid), dim3(256), 0, stream, bs.codes, bs.cw, bs.ncodes, j.n_ops, bs.rflags,
                       j.meta_r, j.n, bpr, j.store, j.store_stride);
    return 0;
}
