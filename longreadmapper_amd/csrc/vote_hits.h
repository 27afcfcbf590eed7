// vote_hits.h -- from a survivor list to its hits: the one staging step and the one hit walk of the vote kernels (vote_kernels.hip); the mapping-quality vote (mapq_kernels.hip) calls find_seed
#pragma once
#include "lrm_hip_util.h"

// Survivors come in two kinds.  UNIQUE seeds (rr == 1: the read's true locus, ~3/4 of the survivors of a noisy
// read) are voted by the lane that loaded them: one SA gather, no staging.  REPEAT seeds (rr > 1) are compacted
// into LDS with the prefix sums of their hit counts and their hits are expanded flat: hit h finds its seed by a
// binary search over the (few) staged repeat seeds.

// survivor s of the hit h: off[s] <= h < off[s + 1]  (off: exclusive prefix of the staged survivors' hit counts,
// strictly increasing because every survivor has at least one hit; cnt >= 1)
// (Measured alternative for the wavefront tier [r2]: a marker byte where the hits of each staged seed begin + a DPP
//  prefix maximum over the 64 consecutive hits of the lanes, i.e. one LDS read instead of seven dependent ones:
//  9.80 vs 9.76 ms per Gbp -- the search is not what the tier waits for.)
__device__ __forceinline__ uint32_t find_seed(const uint32_t *off, uint32_t cnt, uint32_t h) {
    uint32_t lo = 0, hi = cnt;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= h) lo = mid; else hi = mid;
    }
    return lo;
}

// The hits [0, total) of the staged survivors (off / srec / sq; geometry of the item: iter, P, tbits), expanded by NT
// threads (tid of NT): all gathers of a step first (U per lane in flight), then sink(live, h, key, order key) for each of
// them.  The loop bounds are uniform, so EVERY lane calls the sink in every step -- a sink may hold a ballot -- with
// live == false (and zeros) past the last hit; a sink that only wants hits returns at once on !live.
struct Staged { const uint32_t *off; const uint64_t *srec; const uint32_t *sq; uint32_t cnt, total, iter, P, tbits; };

template <int NT, int U, typename Sink>
__device__ __forceinline__ void for_each_hit(const LrmIndexView &ix, const Staged &g, uint32_t tid, Sink sink) {
    for (uint32_t hb = 0; hb < g.total; hb += NT * U) {
        uint64_t v[U];
        uint32_t ss[U], tt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t h = hb + (uint32_t) u * NT + tid;
            v[u] = 0; ss[u] = 0; tt[u] = 0;
            if (h < g.total) {
                const uint32_t s = find_seed(g.off, g.cnt, h);
                ss[u] = s;
                tt[u] = h - g.off[s];
                v[u] = sa_locate(ix, (g.srec[s] & ((1ull << 40) - 1ull)) + tt[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t h = hb + (uint32_t) u * NT + tid;
            const bool live = h < g.total;
            uint64_t key = 0;
            uint32_t order = 0;
            if (live) {
                const uint32_t q = g.sq[ss[u]];
                key = v[u] - (uint64_t) (g.iter + q * g.P);                    // alnmain.c:363-365 (u64 wrap kept); j < 2^32
                order = (q << g.tbits) | tt[u];
            }
            sink(live, h, key, order);
        }
    }
}

// One chunk of up to 64 survivors of a wavefront, one per lane (record e, seed ordinal q; zeros past the chunk): its repeat
// seeds are appended to the staging arrays behind the `at.n` seeds with `at.hits` hits staged before it (zeros, unless the
// caller accumulates chunks), with the exclusive prefix of their hit counts and the terminator off[n] = hits.  Returns the
// new totals.  Ends with a wavefront fence and a wave barrier: on return every lane may read the staging.  (The fence is
// acquire-release at both sites; vote_item_wave had a release fence there.  At wavefront scope it emits no instruction and
// only binds the compiler.)
struct WaveStage { uint32_t n, hits; };                     // repeat seeds staged, their hits
__device__ __forceinline__ WaveStage stage_repeats_wave(uint32_t *off, uint64_t *srec, uint32_t *sq, uint64_t e, uint32_t q, WaveStage at,
                                                        uint32_t lane) {
    const uint32_t rr = (uint32_t) (e >> 40);
    const bool big = rr > 1;
    const unsigned long long bm = __ballot(big);
    const uint32_t incl = wave_incl_scan(big ? rr : 0u);
    if (big) {
        const uint32_t idx = at.n + mask_rank(bm);
        off[idx] = at.hits + incl - rr; srec[idx] = e; sq[idx] = q;
    }
    at.hits += (uint32_t) __builtin_amdgcn_readlane((int) incl, 63);
    at.n += (uint32_t) __popcll(bm);
    if (lane == 0) off[at.n] = at.hits;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return at;
}

// One chunk of up to 256 survivors of a workgroup, one per thread (record e0, seed ordinal q0, hit count r0; zeros past the
// chunk): the repeat seeds are compacted into the staging arrays with the exclusive prefix of their hit counts -- a wave scan,
// the four wave totals through s_wsum, the rank inside the wave by mask_rank.  Ends with a barrier: the staging is complete.
// EXACT (the exact tier): the previous chunk or pass may still be reading the staging, so a barrier comes first; and the
// unique seeds are counted too (s_wsum[8..11]): their keys go to the key scratch in front of the chunk's repeat hits.
struct BlockStage { uint32_t nbig, total, nuni, urank; };      // repeat seeds, their hits, unique seeds, this thread's rank among those
template <bool EXACT>
__device__ __forceinline__ BlockStage stage_repeats_block(uint32_t *off, uint64_t *srec, uint32_t *sq, uint32_t *s_wsum, uint64_t e0,
                                                          uint32_t q0, uint32_t r0) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const bool b0 = r0 > 1;
    const uint32_t h0 = b0 ? r0 : 0u;
    const unsigned long long bm = __ballot(b0), um = EXACT ? __ballot(r0 == 1) : 0ull;
    const uint32_t incl_h = wave_incl_scan(h0);
    if (EXACT) __syncthreads();
    if (lane == 63) {
        s_wsum[wave] = incl_h; s_wsum[4 + wave] = (uint32_t) __popcll(bm);
        if (EXACT) s_wsum[8 + wave] = (uint32_t) __popcll(um);
    }
    __syncthreads();
    BlockStage r = {0, 0, 0, 0};
    uint32_t woff_h = 0, woff_n = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t x = s_wsum[w], y = s_wsum[4 + w], z = EXACT ? s_wsum[8 + w] : 0u;
        r.total += x; r.nbig += y; r.nuni += z;
        if (w < wave) { woff_h += x; woff_n += y; r.urank += z; }
    }
    r.urank += mask_rank(um);
    if (b0) {
        const uint32_t idx = woff_n + mask_rank(bm);
        off[idx] = woff_h + incl_h - h0; srec[idx] = e0; sq[idx] = q0;
    }
    if (tid == 0) off[r.nbig] = r.total;
    __syncthreads();
    return r;
}
