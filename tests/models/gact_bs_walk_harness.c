// SPDX-License-Identifier: MIT
// C entry points for tests/test_gact_bs_walk_recurrence.py: the walk through one traceback block as
// longreadmapper_amd/csrc/gact_bs_circuit.h does it (bs_walk_block, bs_walk_block_win: `on` by recurrence, ns brought up
// to date once per block), and beside it the form it replaced, kept here as the reference: `on` compared on every
// anti-diagonal (ns == the anti-diagonal's number, BS_WALK_NO_STEP from 2(T-O) on), ns advanced and the stop rule
// applied to it on every step.
#include "../../longreadmapper_amd/csrc/gact_bs_circuit.h"

int bswk_block_steps(void) { return BS_K; }

static void ref_take(struct BsWalk *w, uint32_t on, uint32_t n, uint32_t g, uint32_t *bw, uint32_t *e2) {
    *bw |= ((n << 1) | g) << *e2;
    *e2 += on << 1;
    const uint32_t ia = on & ~(n & g) & 1u;                                   // every column but 'D'
    const uint32_t ib = on & ~(n & ~g) & 1u;                                  // every column but 'I'
    w->na += (int32_t) ia;
    w->nb += (int32_t) ib;
    w->ns += (int32_t) (ia + ib);
    const uint32_t in = (uint32_t) w->na & (uint32_t) w->nb & (uint32_t) w->ns;
    w->ns = (int32_t) ((uint32_t) w->ns & (in | ~BS_WALK_STOPPED_BIT));
}

static uint32_t ref_bit(uint64_t plane, uint32_t t, uint32_t on) { return on ? (uint32_t) (plane >> (t & 63u)) & 1u : 0u; }

// planes: BS_K x {N.lo, N.hi, G.lo, G.hi}; state: na, nb, ns, score (in and out)
uint64_t bswk_walk_ref(int32_t *state, const uint32_t *planes, int sbase, int lim2, int boff, uint32_t *e2, int *running) {
    struct BsWalk w = {state[0], state[1], state[2], state[3]};
    uint32_t bw[2] = {0u, 0u}, e[2] = {0u, 0u};
    for (int k = 0; k < BS_K; ++k) {
        const uint32_t d = (uint32_t) (sbase - lim2 + k);
        const int32_t sk = (int32_t) (d > BS_WALK_NO_STEP ? d : BS_WALK_NO_STEP);
        const uint32_t on = w.ns == sk ? 1u : 0u;
        const uint32_t t = (uint32_t) (w.nb + boff - ((k + 1) >> 1));
        const uint64_t N = (uint64_t) planes[4 * k] | ((uint64_t) planes[4 * k + 1] << 32);
        const uint64_t G = (uint64_t) planes[4 * k + 2] | ((uint64_t) planes[4 * k + 3] << 32);
        ref_take(&w, on, ref_bit(N, t, on), ref_bit(G, t, on), &bw[k >= BS_K / 2], &e[k >= BS_K / 2]);
    }
    uint32_t eq = 0;
    for (int h = 0; h < 2; ++h)
        for (uint32_t i = 0; i < e[h]; i += 2) eq += ((bw[h] >> i) & 3u) == 1u;
    *e2 = e[0] + e[1];
    w.score += (int32_t) ((*e2 >> 1) - eq);
    state[0] = w.na; state[1] = w.nb; state[2] = w.ns; state[3] = w.score;
    *running = ((uint32_t) (w.na & w.nb & w.ns) & BS_WALK_STOPPED_BIT) != 0u;
    return (uint64_t) bw[0] | (e[0] < 64u ? (uint64_t) bw[1] << e[0] : 0u);
}

uint64_t bswk_walk_full(int32_t *state, const uint32_t *planes, int sbase, int lim2, int boff, uint32_t *e2, int *running) {
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

// the same planes cut to bits o .. o+31, o = bs_win_origin(nb + boff) of the entry state; *o_out: that origin
uint64_t bswk_walk_win(int32_t *state, const uint32_t *planes, int sbase, int lim2, int boff, uint32_t *e2, int *running,
                       uint32_t *o_out) {
    struct BsWalk w = {state[0], state[1], state[2], state[3]};
    const uint32_t o = bs_win_origin(w.nb + boff);
    uint32_t N[BS_K], G[BS_K];
    for (int k = 0; k < BS_K; ++k) {
        N[k] = (uint32_t) (((uint64_t) planes[4 * k] | ((uint64_t) planes[4 * k + 1] << 32)) >> o);
        G[k] = (uint32_t) (((uint64_t) planes[4 * k + 2] | ((uint64_t) planes[4 * k + 3] << 32)) >> o);
    }
    const uint64_t bw = bs_walk_block_win(&w, N, G, sbase, lim2, boff, o, e2);
    state[0] = w.na; state[1] = w.nb; state[2] = w.ns; state[3] = w.score;
    *running = bs_walk_running(&w);
    *o_out = o;
    return bw;
}
