// SPDX-License-Identifier: MIT
// C entry points over longreadmapper_amd/csrc/gact_bs_circuit.h for tests/test_gact_bs_circuit.py: the header is the
// source the kernel compiles, evaluated here with its host definitions of the truth-table and bit-field instructions.
#include "../../longreadmapper_amd/csrc/gact_bs_circuit.h"

void bsc_half(int bound, int track, const uint32_t *in, uint32_t *out) {
    const struct BsHalf o = bs_half_circuit(bound, track, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9]);
    out[0] = o.V1; out[1] = o.V0; out[2] = o.H1; out[3] = o.H0; out[4] = o.N; out[5] = o.G;
}

int bsc_block_steps(void) { return BS_K; }

// state: na, nb, ns, score (in and out); planes: BS_K x {N.lo, N.hi, G.lo, G.hi}
uint64_t bsc_walk_block(int32_t *state, const uint32_t *planes, int sbase, int lim2, int boff, uint32_t *e2, int *running) {
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
