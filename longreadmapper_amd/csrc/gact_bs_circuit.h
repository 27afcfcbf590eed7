// SPDX-License-Identifier: MIT
// The lane-local arithmetic of the bit-sliced GACT kernel (gact_bs_kernels.hip): the difference circuit of one
// 32-bit half of an anti-diagonal, and the bookkeeping of one traceback block's walk.  The file compiles for the
// device (hipcc: v_bitop3_b32, v_bfe_u32) and as plain C for the host (the same truth tables evaluated bit by bit),
// so tests/test_gact_bs_circuit.py checks on the CPU the very source the kernel runs.
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
// keeps the compiler from rewriting a value's arithmetic (it would track sums a second time, or turn a 0/1 into selects)
#define BS_OPAQUE(x) asm("" : "+v"(x))
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
#define BS_OPAQUE(x) (void) (x)
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

// A lane's place on its path, kept in the form the stop rule and the step test read directly:
//   na = a - amax, nb = b - bmax: negative while the walk may go on;
//   ns = a + b - 2(T-O): the anti-diagonal, negative below the one no walk passes.  (Only a read's last tile has
//        amax or bmax above T-O, so the rule a + b < 2(T-O) binds there alone and can be applied to every lane.)
// "Still walking" is bit 30 of na & nb & ns; a walk that has stopped gets bit 30 of ns cleared, so ns never again
// equals a step's anti-diagonal, and `ns == anti-diagonal of this step` is the whole test for "this lane takes a
// step here".  A lane that never walks starts with ns = 0.
struct BsWalk { int32_t na, nb, ns, score; };

#define BS_WALK_STOPPED_BIT 0x40000000u
#define BS_WALK_NO_STEP 0x7fffff00u        // the value `ns` is compared with on anti-diagonals from 2(T-O) on

BS_FN int bs_walk_running(const struct BsWalk *w) {
    return ((uint32_t) (w->na & w->nb & w->ns) & BS_WALK_STOPPED_BIT) != 0u;
}

// One anti-diagonal.  k: its number inside the block; sk: that anti-diagonal minus 2(T-O), or BS_WALK_NO_STEP;
// boff: bmax - (anti-diagonal of the block's first plane) / 2 + 32, so that the lane's lattice point is bit
// nb + boff - ceil(k/2) of the 64-bit plane.  The codes (0 X, 1 =, 2 I, 3 D) are appended to *bw at bit *e2.
BS_FN void bs_walk_step(struct BsWalk *w, int k, int sk, int32_t boff, struct BsPl N, struct BsPl G, uint32_t *bw,
                        uint32_t *e2) {
    uint32_t on = w->ns == sk ? 1u : 0u;
    BS_OPAQUE(on);
    BS_OPAQUE(w->nb);
    BS_OPAQUE(*e2);
    BS_OPAQUE(*bw);
    const uint32_t t = (uint32_t) (w->nb + boff - ((k + 1) >> 1));
    const int up = t > 31u;
    const uint32_t n = BS_BFE(up ? N.hi : N.lo, t, on), g = BS_BFE(up ? G.hi : G.lo, t, on);   // width 0: not on this one
    *bw |= ((n << 1) | g) << *e2;
    *e2 += on << 1;
    const uint32_t ia = BS_LOP3(on, n, g, TA & ~(TB & TC));                  // every column but 'D'
    const uint32_t ib = BS_LOP3(on, n, g, TA & ~(TB & ~TC));                 // every column but 'I'
    w->na += (int32_t) ia;
    w->nb += (int32_t) ib;
    w->ns += (int32_t) (ia + ib);
    const uint32_t in = BS_LOP3((uint32_t) w->na, (uint32_t) w->nb, (uint32_t) w->ns, TA & TB & TC);
    w->ns = (int32_t) BS_LOP3((uint32_t) w->ns, in, BS_WALK_STOPPED_BIT, TA & (TB | ~TC));
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
BS_FN uint64_t bs_walk_block(struct BsWalk *w, const struct BsPl *N, const struct BsPl *G, int sbase, int lim2, int32_t boff,
                             uint32_t *e2) {
    uint32_t bw[2] = {0u, 0u}, e[2] = {0u, 0u};
    BS_OPAQUE(boff);
#pragma unroll
    for (int k = 0; k < BS_K; ++k) {
        const uint32_t sk = (uint32_t) (sbase - lim2 + k);                    // negative, or past the last anti-diagonal

        bs_walk_step(w, k, (int32_t) (sk > BS_WALK_NO_STEP ? sk : BS_WALK_NO_STEP), boff, N[k], G[k], &bw[k >= BS_K / 2], &e[k >= BS_K / 2]);
    }
    const uint32_t eq = bs_popcount32(BS_LOP3(bw[0], bw[0] >> 1, 0x55555555u, TA & ~TB & TC)) +
                        bs_popcount32(BS_LOP3(bw[1], bw[1] >> 1, 0x55555555u, TA & ~TB & TC));
    *e2 = e[0] + e[1];
    w->score += (int32_t) ((*e2 >> 1) - eq);
    return (uint64_t) bw[0] | ((uint64_t) bw[1] << e[0]);                   // e[0] <= 32
}

#endif
