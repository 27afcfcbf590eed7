// SPDX-License-Identifier: MIT
// The lane-local arithmetic of the bit-sliced GACT kernel (gact_bs_kernels.hip): the difference circuit of one
// 32-bit half of an anti-diagonal, the bookkeeping of one traceback block's walk, and the recompute and walk of a
// block on the 32 lattice points per anti-diagonal that one lane's walk can reach.  The file compiles for the
// device (hipcc: v_bitop3_b32, v_bfe_u32, v_alignbit_b32) and as plain C for the host (the same truth tables
// evaluated bit by bit), so tests/test_gact_bs_circuit.py, tests/test_gact_bs_window.py and
// tests/test_gact_bs_walk_recurrence.py check on the CPU the very source the kernel runs.
#ifndef LRM_GACT_BS_CIRCUIT_H
#define LRM_GACT_BS_CIRCUIT_H
#include <stdint.h>

// a three-input truth table is the function evaluated on A = 0xF0, B = 0xCC, C = 0xAA
enum { TA = 0xF0, TB = 0xCC, TC = 0xAA };

#if defined(__HIPCC__)
#define BS_FN __device__ __forceinline__
// gfx950 v_bitop3_b32: any boolean function of three words in one instruction
#define BS_LOP3(a, b, c, EXPR) __builtin_amdgcn_bitop3_b32((a), (b), (c), (uint32_t) (EXPR) & 0xFFu)
#define BS_BFE(x, off, width) __builtin_amdgcn_ubfe((x), (off), (width))          // offset and width mod 32
#define BS_ALIGNBIT(hi, lo, sh) __builtin_amdgcn_alignbit((hi), (lo), (sh))      // bits sh .. sh+31 of hi:lo, sh mod 32
// keeps the compiler from rewriting a value's arithmetic (it would track sums a second time, or turn a 0/1 into selects)
#define BS_OPAQUE(x) asm("" : "+v"(x))
#define BS_OPAQUE_S(x) asm("" : "+s"(x))                                          // the same for a wave-uniform value
#else
#define BS_FN static inline
static inline uint32_t bs_lop3_eval(uint32_t a, uint32_t b, uint32_t c, uint32_t table) {
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i)
        if ((table >> i) & 1u) r |= ((i & 4) ? a : ~a) & ((i & 2) ? b : ~b) & ((i & 1) ? c : ~c);
    return r;
}
#define BS_LOP3(a, b, c, EXPR) bs_lop3_eval((a), (b), (c), (uint32_t) (EXPR) & 0xFFu)
static inline uint32_t bs_bfe_eval(uint32_t x, uint32_t off, uint32_t width) {
    width &= 31u;
    return width ? (x >> (off & 31u)) & ((1u << width) - 1u) : 0u;
}
#define BS_BFE(x, off, width) bs_bfe_eval((x), (off), (width))
#define BS_ALIGNBIT(hi, lo, sh) ((uint32_t) ((((uint64_t) (hi) << 32) | (uint64_t) (lo)) >> ((sh) & 31u)))
#define BS_OPAQUE(x) (void) (x)
#define BS_OPAQUE_S(x) (void) (x)
#endif

// ----------------------------------------------------------------------------------------
// the difference circuit
// ----------------------------------------------------------------------------------------
// u = H of the insertion neighbour, w = V of the deletion neighbour as 2-bit codes (value + 1), m = bases equal:
//     m:   V = 3 - u = ~u,            H = ~w
//     !m:  V = max(1 - u, w - u, 0),  H = max(1 - w, u - w, 0)             (H is V with u and w exchanged)
// as ten truth tables, three deep from the old state to the new one:
//     t = w1 & (~u0 | w0)         V1 = ~u1 & (m | t)
//     z = w1 & ~(u1 ^ w0)         f  = u1 ? (~u0 & z) : ~(u0 ^ z)           V0 = m ? ~u0 : f
// Decision planes (the spec's tie order: DIAG iff s >= u-1 and s >= w-1, else INS iff u >= w, else DEL):
//     N = ~m & (u1 | w1)          a gap beats the mismatch diagonal
//     G = m | (w1 & ~t')          N ? deletion : match, t' = u1 & (~w0 | u0) being the t of the H side
// BOUND: free-exit points (bm) are forced to V = H = 0 (code 1); lattice points outside a band narrower than
// the 128 diagonals of the planes (~band) to code 0 (-1), the value that never wins.
struct BsHalf { uint32_t V1, V0, H1, H0, N, G; };

BS_FN struct BsHalf bs_half_circuit(int bound, int track, uint32_t u1, uint32_t u0, uint32_t w1, uint32_t w0, uint32_t ql,
                                    uint32_t qh, uint32_t dl, uint32_t dh, uint32_t bm, uint32_t band) {
    struct BsHalf o;
    const uint32_t e1 = ql ^ dl;
    const uint32_t m = BS_LOP3(e1, qh, dh, ~TA & ~(TB ^ TC));                 // bases equal
    const uint32_t tv = BS_LOP3(w1, u0, w0, TA & (~TB | TC));
    const uint32_t th = BS_LOP3(u1, w0, u0, TA & (~TB | TC));
    const uint32_t zv = BS_LOP3(w1, u1, w0, TA & ~(TB ^ TC));
    const uint32_t zh = BS_LOP3(u1, w1, u0, TA & ~(TB ^ TC));
    uint32_t v1 = BS_LOP3(u1, m, tv, ~TA & (TB | TC));
    uint32_t h1 = BS_LOP3(w1, m, th, ~TA & (TB | TC));
    const uint32_t fv = BS_LOP3(u1, u0, zv, (TA & ~TB & TC) | (~TA & ~(TB ^ TC)));
    const uint32_t fh = BS_LOP3(w1, w0, zh, (TA & ~TB & TC) | (~TA & ~(TB ^ TC)));
    uint32_t v0 = BS_LOP3(m, u0, fv, (TA & ~TB) | (~TA & TC));
    uint32_t h0 = BS_LOP3(m, w0, fh, (TA & ~TB) | (~TA & TC));
    o.N = 0; o.G = 0;
    if (track) {
        o.N = BS_LOP3(m, u1, w1, ~TA & (TB | TC));
        o.G = BS_LOP3(m, w1, th, TA | (TB & ~TC));
    }
    if (bound) {
        v1 = BS_LOP3(v1, bm, band, TA & ~TB & TC);  v0 = BS_LOP3(v0, bm, band, (TA | TB) & TC);
        h1 = BS_LOP3(h1, bm, band, TA & ~TB & TC);  h0 = BS_LOP3(h0, bm, band, (TA | TB) & TC);
    }
    o.V1 = v1; o.V0 = v0; o.H1 = h1; o.H0 = h0;
    return o;
}

// ----------------------------------------------------------------------------------------
// the walk through one traceback block
// ----------------------------------------------------------------------------------------
#ifndef BS_K
#define BS_K 32                 // anti-diagonals per traceback block (even, <= 32)
#endif

struct BsPl { uint32_t lo, hi; };                    // one bit-plane of an anti-diagonal: 64 lattice points

// A lane's place on its path, kept in the form the stop rule reads directly:
//   na = a - amax, nb = b - bmax: negative while the walk may go on;
//   ns = a + b - 2(T-O): the anti-diagonal, negative below the one no walk passes.  (Only a read's last tile has
//        amax or bmax above T-O, so the rule a + b < 2(T-O) binds there alone and can be applied to every lane.)
// "Still walking" is bit 30 of na & nb & ns; a walk that has stopped gets bit 30 of ns cleared, so ns never again
// equals an anti-diagonal's number.  A lane that never walks starts with ns = 0.
//
// Which anti-diagonals of a block a lane steps on (`on`) is a recurrence, not a comparison per step.  Blocks are
// walked in order, so a lane that is still walking stands on the block's first anti-diagonal or on its second (a
// diagonal step from the last one of the block before): on = (ns == anti-diagonal) is compared ONCE, for k = 0.
// From there a gap (n = 1) leads to the next anti-diagonal, a diagonal (n = 0) over it, and an anti-diagonal that
// was passed over is followed by one the lane is on:
//     on' = (on ? n : 1)  &  still walking after this step  &  the next anti-diagonal is below 2(T-O)
// The last term is wave-uniform (`may`, 0 or 1).  With it no lane is `on` from 2(T-O) upwards, so inside a block
// "still walking" needs na and nb only -- and the block's entry ns, whose bit 30 says whether the lane walked at
// all when the block began: ns itself is not advanced step by step.  It is brought up to date once, behind the
// block's last step, from what na and nb moved by (a + b), and loses bit 30 there if the walk has stopped.
struct BsWalk { int32_t na, nb, ns, score; };

#define BS_WALK_STOPPED_BIT 0x40000000u
#define BS_WALK_NO_STEP 0x7fffff00u        // the value `ns` is compared with when the block starts at 2(T-O) or above

BS_FN int bs_walk_running(const struct BsWalk *w) {
    return ((uint32_t) (w->na & w->nb & w->ns) & BS_WALK_STOPPED_BIT) != 0u;
}

// One anti-diagonal.  k: its number inside the block; *t: the plane bit of the lane's lattice point on it, which is
// nb + boff - ceil(k/2) with boff = bmax - (anti-diagonal of the block's first plane) / 2 + 32; it is carried from step
// to step (+1 with every column but 'I', -1 behind every even anti-diagonal) instead of being added up again from nb.
// The codes (0 X, 1 =, 2 I, 3 D) are appended to *bw at bit *e2.
// the lane's decision (n, g; both 0 where *on is 0) taken: code appended, place advanced, *on for the next anti-diagonal.
// may: 1 if that anti-diagonal is below 2(T-O), else 0.  w->ns is the block's entry value throughout.
BS_FN void bs_walk_take(struct BsWalk *w, int k, uint32_t *on, uint32_t may, uint32_t *t, uint32_t n, uint32_t g,
                        uint32_t *bw, uint32_t *e2) {
    *bw |= ((n << 1) | g) << *e2;
    *e2 += *on << 1;
    const uint32_t ia = BS_LOP3(*on, n, g, TA & ~(TB & TC));                 // every column but 'D'
    const uint32_t ib = BS_LOP3(*on, n, g, TA & ~(TB & ~TC));                // every column but 'I'
    w->na += (int32_t) ia;
    w->nb += (int32_t) ib;
    *t = (k & 1) ? *t + ib : *t + ib + 0xFFFFFFFFu;
    const uint32_t in = BS_LOP3((uint32_t) w->na, (uint32_t) w->nb, (uint32_t) w->ns, TA & TB & TC);
    const uint32_t nx = BS_LOP3(*on, n, may, (~TA | TB) & TC);               // 0 or 1: the field width that reads `in`
    *on = BS_BFE(in, 30, nx);
}

BS_FN void bs_walk_step(struct BsWalk *w, int k, uint32_t *on, uint32_t may, uint32_t *t, struct BsPl N, struct BsPl G,
                        uint32_t *bw, uint32_t *e2) {
    BS_OPAQUE(*on);
    BS_OPAQUE(*t);
    BS_OPAQUE(*e2);
    BS_OPAQUE(*bw);
    const int up = *t > 31u;
    const uint32_t n = BS_BFE(up ? N.hi : N.lo, *t, *on), g = BS_BFE(up ? G.hi : G.lo, *t, *on);   // width 0: not on this one
    bs_walk_take(w, k, on, may, t, n, g, bw, e2);
}

// The same on the block's 32-point window (below): N, G hold plane bits o .. o+31 and *t starts at nb + boff - o, always
// inside the word while the lane steps in this block.
BS_FN void bs_walk_step_win(struct BsWalk *w, int k, uint32_t *on, uint32_t may, uint32_t *t, uint32_t N, uint32_t G,
                            uint32_t *bw, uint32_t *e2) {
    BS_OPAQUE(*on);
    BS_OPAQUE(*t);
    BS_OPAQUE(*e2);
    BS_OPAQUE(*bw);
    const uint32_t n = BS_BFE(N, *t, *on), g = BS_BFE(G, *t, *on);
    bs_walk_take(w, k, on, may, t, n, g, bw, e2);
}

BS_FN uint32_t bs_popcount32(uint32_t x) {
#if defined(__HIPCC__)
    return (uint32_t) __popc(x);
#else
    return (uint32_t) __builtin_popcount(x);
#endif
}

// The whole block: anti-diagonals sbase .. sbase + BS_K - 1 (sbase a multiple of BS_K), lim2 = 2(T-O),
// boff = bmax - sbase/2 + 32.  Returns the block's codes, *e2 = twice their number.  The score (one per column
// that is not '=') is counted from the code words afterwards instead of step by step.
struct BsWalkIn { int32_t na, nb; };                 // where the block was entered
// is the lane on the block's first anti-diagonal?
BS_FN uint32_t bs_walk_enter(const struct BsWalk *w, struct BsWalkIn *in, int sbase, int lim2) {
    const uint32_t s0 = (uint32_t) (sbase - lim2);                            // negative, or past the last anti-diagonal
    in->na = w->na; in->nb = w->nb;
    return w->ns == (int32_t) (s0 > BS_WALK_NO_STEP ? s0 : BS_WALK_NO_STEP) ? 1u : 0u;
}
// 1 if anti-diagonal k of the block is below 2(T-O)
BS_FN uint32_t bs_walk_may(int sbase, int lim2, int k) {
    int32_t d = sbase + k - lim2;
    BS_OPAQUE_S(d);                                                          // the sign bit by a scalar shift, not a select per lane
    return (uint32_t) d >> 31;
}
BS_FN uint64_t bs_walk_join(struct BsWalk *w, const struct BsWalkIn *in, const uint32_t *bw, const uint32_t *e, uint32_t *e2) {
    const uint32_t eq = bs_popcount32(BS_LOP3(bw[0], bw[0] >> 1, 0x55555555u, TA & ~TB & TC)) +
                        bs_popcount32(BS_LOP3(bw[1], bw[1] >> 1, 0x55555555u, TA & ~TB & TC));
    *e2 = e[0] + e[1];
    w->score += (int32_t) ((*e2 >> 1) - eq);
    // the anti-diagonal the lane has reached, and the stop rule on it
    w->ns += (w->na - in->na) + (w->nb - in->nb);
    const uint32_t run = BS_LOP3((uint32_t) w->na, (uint32_t) w->nb, (uint32_t) w->ns, TA & TB & TC);
    w->ns = (int32_t) BS_LOP3((uint32_t) w->ns, run, BS_WALK_STOPPED_BIT, TA & (TB | ~TC));
    return (uint64_t) bw[0] | ((uint64_t) bw[1] << e[0]);                   // e[0] <= 32
}

BS_FN uint64_t bs_walk_block(struct BsWalk *w, const struct BsPl *N, const struct BsPl *G, int sbase, int lim2, int32_t boff,
                             uint32_t *e2) {
    uint32_t bw[2] = {0u, 0u}, e[2] = {0u, 0u};
    struct BsWalkIn in;
    uint32_t on = bs_walk_enter(w, &in, sbase, lim2);
    uint32_t t = (uint32_t) (w->nb + boff);
#pragma unroll
    for (int k = 0; k < BS_K; ++k)
        bs_walk_step(w, k, &on, bs_walk_may(sbase, lim2, k + 1), &t, N[k], G[k], &bw[k >= BS_K / 2], &e[k >= BS_K / 2]);
    return bs_walk_join(w, &in, bw, e, e2);
}

// on the window planes of bs_win_block, o the window's origin
BS_FN uint64_t bs_walk_block_win(struct BsWalk *w, const uint32_t *N, const uint32_t *G, int sbase, int lim2, int32_t boff,
                                 uint32_t o, uint32_t *e2) {
    uint32_t bw[2] = {0u, 0u}, e[2] = {0u, 0u};
    struct BsWalkIn in;
    uint32_t on = bs_walk_enter(w, &in, sbase, lim2);
    uint32_t t = (uint32_t) (w->nb + boff) - o;
#pragma unroll
    for (int k = 0; k < BS_K; ++k)
        bs_walk_step_win(w, k, &on, bs_walk_may(sbase, lim2, k + 1), &t, N[k], G[k], &bw[k >= BS_K / 2], &e[k >= BS_K / 2]);
    return bs_walk_join(w, &in, bw, e, e2);
}

// ----------------------------------------------------------------------------------------
// a traceback block recomputed on a 32-point window
// ----------------------------------------------------------------------------------------
// The only reader of a block's decision planes is the lane's own walk, and where it enters is known before the
// recompute: plane bit t0 = nb + boff of anti-diagonal k = 0 of the block (a walk that enters on k = 1 is on bit
// t0 - 1 of that plane, which is what a step from bit t0 of k = 0 can reach).  Crossing k anti-diagonals moves a
// walk by at most k diagonals, and in plane bits (even k: diagonal 2t - 64, odd k: 2t - 63) that is
//     even k:  t0 - k/2 <= t <= t0 + k/2          odd k:  t0 - (k+1)/2 <= t <= t0 + (k-1)/2
// so every point the walk can be on has t0 - 16 <= t <= t0 + 15 on every anti-diagonal of the block (k <= 31):
// ONE 32-bit word per plane with a fixed origin o, the same bit numbering on all anti-diagonals.  The set is closed
// under the recurrence: a point of it on anti-diagonal k reads its neighbours' bits t-1, t (even k) or t, t+1
// (odd k) of anti-diagonal k+1, which satisfy the bound of k+1.  So the step is the full-width step on one word
// (u = H << 1 on even, w = V >> 1 on odd anti-diagonals), and the zeros the shifts bring in at an inner edge of the
// window spoil one more bit every second step, exactly as fast as the reachable set draws back from that edge.
// The origin is clamped to the plane (o = min(max(t0 - 16, 0), 32)): the window then never holds a point outside
// the 64 of the plane, an edge it shares with the plane gets the zeros the full-width step gets there, and what
// the clamp cuts off is out of the band anyway.  The 33 reachable points of the checkpoint (k = BS_K) enter only
// as the inputs of the first step: u = H bits o .. o+31, w = V bits o+1 .. o+32.
// Valid for a band of all 128 diagonals and no free-exit point near it (the unmasked step).
BS_FN uint32_t bs_win_origin(int32_t t0) {
    const int32_t o = t0 - 16;
    return (uint32_t) (o < 0 ? 0 : o > 32 ? 32 : o);
}
// bits o .. o+31 of hi:lo, 0 <= o <= 33
BS_FN uint32_t bs_win32(uint32_t lo, uint32_t hi, uint32_t o) {
    return (uint32_t) ((((uint64_t) hi << 32) | (uint64_t) lo) >> o);
}

// What the block reads, cut to the window.  ck: the checkpoint as stored (V1, V0, H1, H0, each lo then hi);
// q, d: the block's three stream words of one sequence bit-plane, bit 0 of q[0] / d[0] being plane bit 0 at window
// shift 0; kept are stream bits o .. o+63, from which a step takes its word with one funnel shift by its own
// (compile-time) window shift.
struct BsWinIn {
    uint32_t u1, u0, w1, w0;                 // neighbour inputs of step BS_K - 1
    uint32_t ql[2], qh[2], dl[2], dh[2];
};
BS_FN void bs_win_cut_ck(struct BsWinIn *in, const uint32_t *ck, uint32_t o) {
    in->w1 = bs_win32(ck[0], ck[1], o + 1u); in->w0 = bs_win32(ck[2], ck[3], o + 1u);
    in->u1 = bs_win32(ck[4], ck[5], o);      in->u0 = bs_win32(ck[6], ck[7], o);
}
BS_FN void bs_win_cut_seq(uint32_t *out, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t o) {
    out[0] = bs_win32(s0, s1, o);
    out[1] = bs_win32(s1, s2, o);
}

// The block's BS_K steps, BS_K - 1 down to 0: N[k], G[k] = decision bits of plane bits o .. o+31 of anti-diagonal k.
// The query window starts at shift 0 and moves up by one after every even anti-diagonal, the text window starts
// at BS_K/2 and moves down by one after every odd one (the order of the full-width recompute).
BS_FN void bs_win_block(const struct BsWinIn *in, uint32_t *N, uint32_t *G) {
    uint32_t V1 = 0u, V0 = 0u, H1 = 0u, H0 = 0u;
    uint32_t ql = in->ql[0], qh = in->qh[0];
    uint32_t dl = BS_ALIGNBIT(in->dl[1], in->dl[0], BS_K / 2), dh = BS_ALIGNBIT(in->dh[1], in->dh[0], BS_K / 2);
#pragma unroll
    for (int k = BS_K - 1; k >= 1; k -= 2) {
        const int first = k == BS_K - 1;
        struct BsHalf x = bs_half_circuit(0, 1, first ? in->u1 : H1, first ? in->u0 : H0, first ? in->w1 : V1 >> 1,
                                          first ? in->w0 : V0 >> 1, ql, qh, dl, dh, 0u, 0u);
        N[k] = x.N; G[k] = x.G;
        const uint32_t shd = (uint32_t) ((k - 1) >> 1);                          // K/2-1 .. 0
        dl = BS_ALIGNBIT(in->dl[1], in->dl[0], shd); dh = BS_ALIGNBIT(in->dh[1], in->dh[0], shd);
        x = bs_half_circuit(0, 1, x.H1 << 1, x.H0 << 1, x.V1, x.V0, ql, qh, dl, dh, 0u, 0u);
        N[k - 1] = x.N; G[k - 1] = x.G;
        V1 = x.V1; V0 = x.V0; H1 = x.H1; H0 = x.H0;
        if (k > 1) {
            const uint32_t shq = (uint32_t) (BS_K / 2 - ((k - 1) >> 1));         // 1 .. K/2-1
            ql = BS_ALIGNBIT(in->ql[1], in->ql[0], shq); qh = BS_ALIGNBIT(in->qh[1], in->qh[0], shq);
        }
    }
}

#endif
