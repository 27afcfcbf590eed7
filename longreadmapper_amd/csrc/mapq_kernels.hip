// mapq_kernels.hip -- mapping quality (docs/GACT_SPEC.md, "Mapping quality"): a second, much simpler vote over the seed
// hits of a read.  The reference prints MAPQ 255 for every mapped read (alnmain.c:460-474); this stage is a choice of
// THIS implementation and runs only when a caller asks for the records.
//
// The vote kernels of vote_kernels.hip keep the two largest 16-diagonal buckets of a phase, which on a noisy read are
// neighbours of the same locus and say nothing about a RIVAL locus.  The survivor lists the seed kernel wrote (rec =
// k | rr << 40, recq = seed ordinal, cnt, per (read, phase)) are still in the workspace when decide_kernel has run, so
// this kernel goes over them once more: every hit of the phases 0 .. d (d: the deciding phase) is either within R
// diagonals of the chosen locus (n1) or counted in two staggered histograms of bucket width 2 R whose fullest bucket
// is the rival (n2).  The arithmetic is mapq_rule.h.
//
// One workgroup of 256 per read.  A wavefront takes chunks of 64 survivors (phase by phase, chunks dealt round-robin
// to the four wavefronts): a unique seed (rr == 1) is voted by the lane that loaded it, repeat seeds are staged in the
// wavefront's own LDS lists and their rows expanded flat, MQ_U gathers in flight per lane, as vote_item_wave does.  The
// staging and the walk are this kernel's own copies of stage_repeats_wave and for_each_hit (vote_hits.h, whose find_seed it
// calls): through the shared ones it measured 0.4 % (staging alone) and 1.8 % (both) slower (profiles/r7/README.md, section 5) --
// the walk here reads the seed ordinal before the gathers are issued, which in the vote kernels costs scratch.
// The histograms are ONE open-addressing table in LDS, {tag, count} per slot, tag = bucket << 1 | histogram, claimed by
// compare-and-swap like the slots of the exact vote kernel.  Then one sweep for the largest count.
#include <hip/hip_runtime.h>
#include "vote_hits.h"
#include "mapq_rule.h"
#include "mapq_table.h"

// a hit: the winner's window, or the two histograms
__device__ __forceinline__ void mq_hit(MqLds &L, uint64_t key, uint64_t best_key, uint32_t r, uint32_t slots, uint32_t &n1) {
    if (mq_inside(key, best_key, r)) { ++n1; return; }
    if (*(volatile uint32_t *) &L.overflow) return;          // the read's answer is fixed (n2 = n1): no more probing of a full table
    if (!mq_insert(L, mq_tag(key, r, 0u), slots) || !mq_insert(L, mq_tag(key, r, 1u), slots)) L.overflow = 1u;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
void mapq_vote_kernel(LrmIndexView ix, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ recq,
                      const uint32_t *__restrict__ g_cnt, const uint32_t *__restrict__ lens,
                      const uint8_t *__restrict__ phase_d, const lrm_entry *__restrict__ best, uint64_t n, uint32_t P,
                      uint32_t cap_q, uint32_t slots, lrm_mapq *__restrict__ out) {
    __shared__ MqLds L;
    const uint64_t read = blockIdx.x;
    if (read >= n) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (tid >> 6));
    const lrm_entry b = best[read];
    if (b.val == 0) {                                         // no locus: the record is all zeros
        if (tid == 0) *reinterpret_cast<uint4 *>(out + read) = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint32_t r = mq_radius_log2(lens[read]);
    const uint32_t d = phase_d[read] < P ? phase_d[read] : P - 1u;
    for (uint32_t s = tid; s < slots; s += 256) { L.tag[s] = MQ_TAG_EMPTY; L.count[s] = 0u; }
    if (tid == 0) { L.n1 = 0u; L.overflow = 0u; }
    __syncthreads();

    MqWaveLds &W = L.w[wave];
    uint32_t n1 = 0, item = 0;
    for (uint32_t ph = 0; ph <= d; ++ph) {
        const uint64_t id = read * (uint64_t) P + ph;
        const uint32_t cnt = g_cnt[id];
        const uint64_t *prec = rec + id * cap_q;
        const uint32_t *pq = recq + id * cap_q;
        for (uint32_t c0 = 0; c0 < cnt; c0 += 64, ++item) {
            if ((item & (MQ_WAVES - 1u)) != wave) continue;
            const uint32_t s = c0 + lane;
            const uint64_t e = s < cnt ? prec[s] : 0ull;
            const uint32_t q = s < cnt ? pq[s] : 0u;
            const uint32_t rr = (uint32_t) (e >> 40);
            const uint64_t sv = rr == 1 ? sa_of_unique(ix, e) : 0ull;       // unique seeds: gather at once (or nothing to gather)
            const bool big = rr > 1;
            const unsigned long long bm = __ballot(big);
            const uint32_t incl = wave_incl_scan(big ? rr : 0u);
            if (big) {
                const uint32_t k = mask_rank(bm);
                W.off[k] = incl - rr; W.srec[k] = e; W.sq[k] = q;
            }
            const uint32_t total = (uint32_t) __builtin_amdgcn_readlane((int) incl, 63);
            const uint32_t nbig = (uint32_t) __popcll(bm);
            if (lane == 0) W.off[nbig] = total;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (rr == 1) mq_hit(L, sv - (uint64_t) (ph + q * P), b.key, r, slots, n1);
            for (uint32_t hb = 0; hb < total; hb += 64 * MQ_U) {             // the rows of the repeat seeds, flat
                uint64_t v[MQ_U];
                uint32_t jj[MQ_U];
#pragma unroll
                for (int u = 0; u < MQ_U; ++u) {
                    const uint32_t h = hb + (uint32_t) u * 64 + lane;
                    v[u] = 0; jj[u] = 0;
                    if (h < total) {
                        const uint32_t k = find_seed(W.off, nbig, h);
                        jj[u] = ph + W.sq[k] * P;
                        v[u] = sa_locate(ix, (W.srec[k] & ((1ull << 40) - 1ull)) + (h - W.off[k]));
                    }
                }
#pragma unroll
                for (int u = 0; u < MQ_U; ++u)
                    if (hb + (uint32_t) u * 64 + lane < total) mq_hit(L, v[u] - (uint64_t) jj[u], b.key, r, slots, n1);   // alnmain.c:363-365 (u64 wrap kept)
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();                                  // the lists are free for the next chunk
        }
    }
    {
        const uint32_t sum = (uint32_t) __builtin_amdgcn_readlane((int) wave_incl_scan(n1), 63);
        if (lane == 0 && sum) atomicAdd(&L.n1, sum);
    }
    __syncthreads();

    uint64_t m = 0;                                                           // one sweep for the fullest bucket of either histogram
    for (uint32_t s = tid; s < slots; s += 256) { const uint32_t c = L.count[s]; m = c > m ? c : m; }
    m = wave_max_u64(m);
    if (lane == 0) L.wmax[wave] = (uint32_t) m;
    __syncthreads();
    if (tid == 0) {
        uint32_t n2 = 0;
        for (int w = 0; w < MQ_WAVES; ++w) n2 = L.wmax[w] > n2 ? L.wmax[w] : n2;
        const uint32_t s1 = L.n1;
        uint32_t flags = 0;
        if (L.overflow) { flags |= LRM_MAPQ_OVERFLOW; n2 = s1; }
        const uint32_t q = mq_value(s1, n2);
        *reinterpret_cast<uint4 *>(out + read) = make_uint4(s1, n2, 1u << r, q | (d << 8) | (flags << 16));   // one 16-byte vector store
    }
}

uint8_t *lrm_mapq_phase_buf(lrm_workspace *ws) {
    if (ws->d_mq_phase) return ws->d_mq_phase;
    if (hipMalloc((void **) &ws->d_mq_phase, ws->n_max) != hipSuccess) {
        (void) hipGetLastError();
        ws->d_mq_phase = nullptr;
        lrm_set_error("hipMalloc of %llu bytes for the deciding phases failed", (unsigned long long) ws->n_max);
        return nullptr;
    }
    ws->bytes += ws->n_max;
    return ws->d_mq_phase;
}

int lrm_launch_mapq(lrm_index *idx, lrm_workspace *ws, const uint32_t *d_lens, uint64_t n, uint32_t seed_len, uint32_t thres,
                    const lrm_entry *d_best, lrm_mapq *d_mapq, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    (void) thres;                                        // (the lists hold the survivors 0 < rr < thres already)
    if (n == 0) return 0;
    if (!ws->d_mq_phase || !ws->d_rec || seed_len != ws->seed_len || n > ws->n_max || !lrm_seed_stamp_is(ws, d_best, n)) {
        lrm_set_error("mapping quality: the workspace did not run the seed stage of this batch with the phase output");
        return -1;
    }
    const uint32_t slots = idx->dbg_mapq_slots ? idx->dbg_mapq_slots : (uint32_t) LRM_MAPQ_SLOTS;     // (lrm_debug_set_mapq_slots checked it)
    uint32_t grid;
    if (lrm_grid_1d(n, "mapq_vote", &grid)) return -1;
    lrm_time_begin(ws, LRM_K_DECIDE, stream);
    hipLaunchKernelGGL(mapq_vote_kernel, dim3(grid), dim3(256), 0, stream, idx->view, (const uint64_t *) ws->d_rec,
                       (const uint32_t *) ws->d_recq, (const uint32_t *) ws->d_cnt, d_lens, (const uint8_t *) ws->d_mq_phase, d_best, n,
                       ws->P, ws->cap_q, slots, d_mapq);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());
    return 0;
}
