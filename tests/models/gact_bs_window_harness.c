// SPDX-License-Identifier: MIT
// C entry points over longreadmapper_amd/csrc/gact_bs_circuit.h for tests/test_gact_bs_window.py: one traceback block
// recomputed and walked in full width (the kernel's masked path with empty masks: bs_half_circuit on both halves of the
// planes, the shifts of gact_bs_kernels.hip:bs_step, bs_walk_block) and on the lane's 32-point window (bs_win_origin,
// bs_win_cut_*, bs_win_block, bs_walk_block_win) from the same checkpoint and the same stream words.
#include "../../longreadmapper_amd/csrc/gact_bs_circuit.h"

int bsw_block_steps(void) { return BS_K; }

// bits sh .. sh+63 of the 96-bit stream s[2]:s[1]:s[0], 0 <= sh < 32
static struct BsPl plane_at(const uint32_t *s, uint32_t sh) {
    struct BsPl p = {BS_ALIGNBIT(s[1], s[0], sh), BS_ALIGNBIT(s[2], s[1], sh)};
    return p;
}

// ck: V1.lo V1.hi V0.lo V0.hi H1.lo H1.hi H0.lo H0.hi; seq: ql[3] qh[3] dl[3] dh[3];
// planes: BS_K x {N.lo, N.hi, G.lo, G.hi}
void bsw_block_full(const uint32_t *ck, const uint32_t *seq, uint32_t *planes) {
    struct BsPl V1 = {ck[0], ck[1]}, V0 = {ck[2], ck[3]}, H1 = {ck[4], ck[5]}, H0 = {ck[6], ck[7]};
    uint32_t shq = 0, shd = BS_K / 2;
    for (int k = BS_K - 1; k >= 0; --k) {
        struct BsPl u1, u0, w1, w0;
        if (k & 1) {                       // w = V >> 1
            u1 = H1; u0 = H0;
            w1.lo = (V1.lo >> 1) | (V1.hi << 31); w1.hi = V1.hi >> 1;
            w0.lo = (V0.lo >> 1) | (V0.hi << 31); w0.hi = V0.hi >> 1;
        } else {                           // u = H << 1
            u1.lo = H1.lo << 1; u1.hi = (H1.hi << 1) | (H1.lo >> 31);
            u0.lo = H0.lo << 1; u0.hi = (H0.hi << 1) | (H0.lo >> 31);
            w1 = V1; w0 = V0;
        }
        const struct BsPl ql = plane_at(seq, shq), qh = plane_at(seq + 3, shq);
        const struct BsPl dl = plane_at(seq + 6, shd), dh = plane_at(seq + 9, shd);
        const struct BsHalf lo = bs_half_circuit(1, 1, u1.lo, u0.lo, w1.lo, w0.lo, ql.lo, qh.lo, dl.lo, dh.lo, 0u, ~0u);
        const struct BsHalf hi = bs_half_circuit(1, 1, u1.hi, u0.hi, w1.hi, w0.hi, ql.hi, qh.hi, dl.hi, dh.hi, 0u, ~0u);
        V1.lo = lo.V1; V1.hi = hi.V1; V0.lo = lo.V0; V0.hi = hi.V0;
        H1.lo = lo.H1; H1.hi = hi.H1; H0.lo = lo.H0; H0.hi = hi.H0;
        planes[4 * k] = lo.N; planes[4 * k + 1] = hi.N; planes[4 * k + 2] = lo.G; planes[4 * k + 3] = hi.G;
        if (k & 1) --shd; else ++shq;      // the text window moves after an odd, the query window after an even one
    }
}

// t0 = nb + boff: the lane's plane bit on the block's first anti-diagonal.  planes: BS_K x {N, G}; returns the origin
uint32_t bsw_block_win(const uint32_t *ck, const uint32_t *seq, int32_t t0, uint32_t *planes) {
    const uint32_t o = bs_win_origin(t0);
    struct BsWinIn in;
    uint32_t N[BS_K], G[BS_K];
    bs_win_cut_ck(&in, ck, o);
    bs_win_cut_seq(in.ql, seq[0], seq[1], seq[2], o);
    bs_win_cut_seq(in.qh, seq[3], seq[4], seq[5], o);
    bs_win_cut_seq(in.dl, seq[6], seq[7], seq[8], o);
    bs_win_cut_seq(in.dh, seq[9], seq[10], seq[11], o);
    bs_win_block(&in, N, G);
    for (int k = 0; k < BS_K; ++k) { planes[2 * k] = N[k]; planes[2 * k + 1] = G[k]; }
    return o;
}

// state: na, nb, ns, score (in and out)
uint64_t bsw_walk_full(int32_t *state, const uint32_t *planes, int sbase, int lim2, int boff, uint32_t *e2, int *running) {
    struct BsWalk w = {state[0], state[1], state[2], state[3]};
    struct BsPl N[BS_K], G[BS_K];
    for (int k = 0; k < BS_K; ++k) {
        N[k].lo = planes[4 * k]; N[k].hi = planes[4 * k + 1];
        G[k].lo = planes[4 * k + 2]; G[k].hi = planes[4 * k + 3];
    }
    const uint64_t bw = bs_walk_block(&w, N, G, sbase, lim2, boff, e2);
    state[0] = w.na; state[1] = w.nb; state[2] = w.ns; state[3] = w.score;
    *running = bs_walk_running(&w);
    return bw;
}

uint64_t bsw_walk_win(int32_t *state, const uint32_t *planes, int sbase, int lim2, int boff, uint32_t o, uint32_t *e2,
                      int *running) {
    struct BsWalk w = {state[0], state[1], state[2], state[3]};
    uint32_t N[BS_K], G[BS_K];
    for (int k = 0; k < BS_K; ++k) { N[k] = planes[2 * k]; G[k] = planes[2 * k + 1]; }
    const uint64_t bw = bs_walk_block_win(&w, N, G, sbase, lim2, boff, o, e2);
    state[0] = w.na; state[1] = w.nb; state[2] = w.ns; state[3] = w.score;
    *running = bs_walk_running(&w);
    return bw;
}
