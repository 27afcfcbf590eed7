// vote_kernels.hip -- K2 of PART 1: the LDS vote over the survivor lists seed_search leaves (seed_kernels.hip); staging and hit walk: vote_hits.h
#include <hip/hip_runtime.h>
#include "vote_hits.h"
#include "vote_hash.h"              // bucket_hash, bucket_pass, sketch_counter

// ----------------------------------------------------------------------------------------
// K2 vote.
// histo_add / histo_find_2_max (histo.c:42-56, 84-96) order entries by insertion; the stable top-2 is "val
// descending, first-seen ascending".  First-seen order of a bucket is the order of (seed ordinal q, SA offset t)
// of its first hit, which is intrinsic to the hit -- so the table can be filled in any order: every slot keeps the
// count, the low 4 bits of the minimum key and the minimum order key (q << tbits) | t.
//
// (Measured and not kept [r2]: a second kernel with a 4096-slot table (70 KB of LDS) for items that need three or more
//  passes -- ultra-long reads, ~3500 hits per item: 45.0 vs 46.1 ms per 2 Gbp, 10.9 vs 11.2 on the bench workload.)
// The vote table always lives in LDS.  ONE kernel votes every (read, phase) item; a 256-thread workgroup owns
// VG consecutive items and routes each by its hit count H (an upper bound on its distinct buckets, left by
// seed_search next to the survivor list):
//   H == 0            the zero result
//   H <= T1_LIMIT     one WAVEFRONT per item (the four wavefronts work on different items), 256-slot table
//   H >  T1_LIMIT     the whole WORKGROUP on one item after the other, T3_SLOTS-slot table, ceil(H / T3_LIMIT)
//                     passes: pass p admits only buckets with hash % passes == p and the per-pass top-2 are merged
//                     (buckets of different passes are disjoint, so the merge is exact)
// Hits are expanded FLAT: the survivors' hit counts are prefix-summed into LDS, and hit h of the item finds its
// seed by a binary search over the prefix -- every lane gathers one SA row per step whatever the shape of the
// item, and all gathers of a step (up to 4 per lane) are in flight before the first vote is cast.  (The first
// version walked repeat seeds two at a time, one memory latency per pair: an item with 24 repeat seeds took 12
// dependent round trips, now 1-2.)
// In front of that kernel run the FAST kernels (further down: "fast path"), which settle nearly every item of a real batch:
// their table only counts -- a slot is {u32 identity of the bucket, u32 count}, an insert one 32-bit compare-and-swap and
// one add -- and holds the unique seeds' buckets only; repeat seeds' hits are looked up in it and otherwise go to a sketch.
// The top two, their minimum keys and their first-seen order are taken from the HITS once the table is final (the rank
// step: 32-bit wave reductions, no table scan).  What they cannot settle goes to the exact kernel above by item number.
// ----------------------------------------------------------------------------------------
#define VG 16                // items per workgroup (default; LRM_VOTE_VG)
#define VG_MAX 64
#define T1_SLOTS 256
#define T1_LIMIT LRM_VOTE_T1_LIMIT
#define T3_SLOTS LRM_VOTE_T3_SLOTS
#define T3_LIMIT LRM_VOTE_T3_LIMIT
#define T3_CHUNK 256                  // survivors per prefix chunk of the workgroup tier: one per thread

// never a vote key: keys are SA - j (u64 wrap) with SA < 2^40 and j < 2^32, i.e. in [0, 2^40) or [2^64 - 2^32, 2^64)
#define EMPTY_KEY 0x8000000000000000ull

// One slot = {min key of the bucket, count, min order key}: the bucket is key >> 4 (histo.c:26-28) and the entry's
// key is the minimum key added to it (histo.c:45-49), so the smallest key IS the slot's identity and its payload.
// Count and order key share one 8-byte word, `count << 32 | ~first` -- the slot's rank in the stable top-2 as it
// stands: the count is a 32-bit atomic add on the high dword, the first-seen order a 32-bit atomic max on the low
// one, and clearing or scanning a slot is one 8-byte LDS access instead of two 4-byte ones.
struct VoteTable {
    uint64_t *key;
    uint64_t *cf;
    uint32_t slots;
};

template <int NT>
__device__ __forceinline__ void table_clear(const VoteTable &t, uint32_t tid) {
    for (uint32_t s = tid; s < t.slots; s += NT) { t.key[s] = EMPTY_KEY; t.cf[s] = 0; }
}

// a hit lands in its bucket's slot: the smaller key (when the caller saw a larger one there), the count, the first-seen order
__device__ __forceinline__ void slot_count(const VoteTable &t, uint32_t slot, bool lower, uint64_t key, uint32_t order, uint32_t n) {
    if (lower) atomicMin((unsigned long long *) &t.key[slot], (unsigned long long) key);
    uint32_t *cf = reinterpret_cast<uint32_t *>(&t.cf[slot]);
    atomicAdd(cf + 1, n);                              // count
    atomicMax(cf, 0xFFFFFFFFu - order);                // ~(min order key)
}

// Returns false only if the table is full (never in the wavefront tier, where H <= 0.75*slots; in the multi-pass
// tier only under a pathological hash skew) -- the probe loop is bounded so a wave can never spin.
__device__ __forceinline__ bool vote_insert(const VoteTable &t, uint64_t key, uint32_t order, uint32_t hash, uint32_t n = 1u) {
    const uint64_t bucket = key >> 4;
    uint32_t slot = (uint32_t) (((uint64_t) hash * t.slots) >> 32);
    for (uint32_t probe = 0; probe < t.slots; ++probe) {
        // (a plain read before the compare-and-swap, to step over occupied slots cheaply, measured SLOWER: 15.5 vs
        //  13.4 ms per Gbp [r2] -- the extra dependent LDS round trip costs more than the CAS it saves)
        const unsigned long long prev = atomicCAS((unsigned long long *) &t.key[slot], EMPTY_KEY, key);
        if (prev == EMPTY_KEY || (prev >> 4) == bucket) {
            slot_count(t, slot, prev != EMPTY_KEY && key < prev, key, order, n);
            return true;
        }
        slot = slot + 1 == t.slots ? 0 : slot + 1;
    }
    return false;
}

__device__ __forceinline__ bool vote_admit(const VoteTable &t, uint64_t key, uint32_t order, uint32_t passes, uint32_t pass) {
    const uint32_t hash = bucket_hash(key >> 4);
    if (passes == 1 || bucket_pass(hash, passes) == pass) return vote_insert(t, key, order, hash);
    return true;
}

struct TopEntry { uint64_t key, bucket; uint32_t val, first; };          // val == 0: none
struct PhaseTop { TopEntry a, b; };

__device__ __forceinline__ void write_phase(LrmPhaseRes *out, const PhaseTop &p) {
    LrmPhaseRes res = {0, 0, 0, 0, 0, 0};
    if (p.a.val) { res.key1 = p.a.key; res.val1 = p.a.val; res.bucket1 = p.a.bucket; }
    if (p.b.val) { res.key2 = p.b.key; res.val2 = p.b.val; res.bucket2 = p.b.bucket; }
    *out = res;
}

// Top-2 of a vote table, "count descending, first-seen ascending" (histo.c:84-96 with the insertion order carried
// by the order key): one u64 per slot, count << 32 | ~first, is unique among the filled slots (every hit has its own
// order key), so the stable top-2 is the two largest keys.  Every lane scans its slots, then two max-reductions.
struct Top2 { uint64_t k1, k2; uint32_t s1, s2; };

// GLOBAL: a table in global memory (the one-pass path of very large items): the counts were written by atomics through
// L2, and a slice of the pool is reused by later items, so the scan reads past the L1 (agent-scope loads)
template <int NT, bool GLOBAL = false>
__device__ __forceinline__ Top2 table_top2(const VoteTable &t, uint32_t tid) {
    uint64_t k1 = 0, k2 = 0;
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t s = tid; s < t.slots; s += NT) {
        const uint64_t k = GLOBAL ? __hip_atomic_load(&t.cf[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : t.cf[s];
        if (k > k1) { k2 = k1; s2 = s1; k1 = k; s1 = s; }
        else if (k > k2) { k2 = k; s2 = s; }
    }
    // wave-level: the largest key, then the largest of what is left
    const uint64_t m1 = wave_max_u64(k1);
    const bool win = k1 == m1 && (m1 >> 32) != 0;
    const uint64_t m2 = wave_max_u64(win ? k2 : k1);
    Top2 r;
    r.k1 = (m1 >> 32) ? m1 : 0; r.k2 = (m2 >> 32) ? m2 : 0; r.s1 = 0; r.s2 = 0;
    if (r.k1) {
        const unsigned long long b = __ballot(k1 == m1);
        r.s1 = (uint32_t) __builtin_amdgcn_readlane((int) s1, (int) __builtin_ctzll(b));
    }
    if (r.k2) {
        const bool has = (win ? k2 : k1) == m2;
        const unsigned long long b = __ballot(has);
        const int src = (int) __builtin_ctzll(b);
        r.s2 = (uint32_t) __builtin_amdgcn_readlane((int) (win ? s2 : s1), src);
    }
    return r;
}

// slot s of a table, found by table_top2 with rank k = count << 32 | ~first (0: none), as an entry of its item's result, and
// the two best slots as that result; global: see table_top2
__device__ __forceinline__ TopEntry entry_of(const VoteTable &t, uint64_t k, uint32_t s, bool global = false) {
    TopEntry e = {0, 0, 0, 0};
    if (k) {
        e.key = global ? __hip_atomic_load(&t.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : t.key[s];
        e.bucket = e.key >> 4; e.val = (uint32_t) (k >> 32); e.first = 0xFFFFFFFFu - (uint32_t) k;
    }
    return e;
}
__device__ __forceinline__ PhaseTop phase_of(const VoteTable &t, uint64_t k1, uint32_t s1, uint64_t k2, uint32_t s2, bool global = false) {
    return PhaseTop{entry_of(t, k1, s1, global), entry_of(t, k2, s2, global)};
}

// the workgroup's top-2 = the two largest of the four wavefronts' pairs (thread 0, after a barrier behind s_top)
__device__ __forceinline__ Top2 block_top2(const Top2 *s_top) {
    Top2 r = {0, 0, 0, 0};
    for (int x = 0; x < 4; ++x) {
        const Top2 c = s_top[x];
        const uint64_t ks[2] = {c.k1, c.k2};
        const uint32_t ss[2] = {c.s1, c.s2};
        for (int y = 0; y < 2; ++y) {
            if (ks[y] > r.k1) { r.k2 = r.k1; r.s2 = r.s1; r.k1 = ks[y]; r.s1 = ss[y]; }
            else if (ks[y] > r.k2) { r.k2 = ks[y]; r.s2 = ss[y]; }
        }
    }
    return r;
}

// clear / scan only as much of a table as x entries can fill at `load` percent
__device__ __forceinline__ uint32_t table_slots_for(uint32_t x, uint32_t load, uint32_t cap) {
    const uint32_t eff = x * 100u / load + 64;
    return eff < cap ? eff : cap;
}

// What every vote kernel is given by value (the launcher fills it once): the items' geometry -- n reads x np phases from
// phase_lo, P = seed_len + 1, cap_q survivor records per (read, phase) --, the order key's shift, the table load in percent,
// and where the results go.  The survivor lists seed_search left (rec, recq, their counts gcnt and hit counts ghits, the
// reads already decided) stay kernel arguments of their own: only there does __restrict__ reach the compiler, and without
// it the per-item loads of ghits / gcnt are vector loads instead of scalar ones (vote slot 3.47 -> 3.68 ms: profiles/r7/README.md, section 5).
struct VoteItems {
    uint64_t n;
    uint32_t P, np, phase_lo, cap_q, tbits, load;
    LrmPhaseRes *phase_res;
};
// one of them: survivor list, survivor and hit count, phase, result
struct Item { const uint64_t *rec; const uint32_t *recq; uint32_t cnt, H, iter; LrmPhaseRes *out; };

// item number -> read, phase and id = read * P + phase (a 64-bit division: ~150 instructions, so once per item at most)
struct ItemId { uint64_t read, id; uint32_t iter; };
__device__ __forceinline__ ItemId item_decode(uint64_t item, const VoteItems &v) {
    ItemId r;
    r.read = item / v.np;
    r.iter = v.phase_lo + (uint32_t) (item - r.read * v.np);
    r.id = r.read * (uint64_t) v.P + r.iter;
    return r;
}

// exact vote of the staged hits; kc_key / kc_ord (multi-pass items): keys kept for the later passes
template <int NT, int VOTE_U>
__device__ __forceinline__ bool vote_hits(const LrmIndexView &ix, const VoteTable &t, const Staged &g, uint32_t tid, uint32_t passes,
                                          uint32_t pass, uint64_t *kc_key = nullptr, uint32_t *kc_ord = nullptr) {
    bool ok = true;
    for_each_hit<NT, VOTE_U>(ix, g, tid, [&](bool live, uint32_t h, uint64_t key, uint32_t order) __attribute__((always_inline)) {
        if (!live) return;
        if (kc_key) { kc_key[h] = key; kc_ord[h] = order; }
        ok &= vote_admit(t, key, order, passes, pass);
    });
    return ok;
}

// ---- wavefront tier: H <= T1_LIMIT, so at most T1_LIMIT survivors -------------------------------------------
struct WaveLds {
    uint64_t key[T1_SLOTS];
    uint64_t srec[T1_LIMIT / 2];             // repeat seeds have >= 2 hits each
    uint64_t cf[T1_SLOTS];
    uint32_t off[T1_LIMIT / 2 + 4];
    uint32_t sq[T1_LIMIT / 2];
};

template <int VOTE_U>
__device__ __forceinline__ void vote_item_wave(const LrmIndexView &ix, const VoteItems &v, const Item &it, uint32_t lane, WaveLds &L) {
    const VoteTable t = {L.key, L.cf, table_slots_for(it.H, v.load, T1_SLOTS)};
    constexpr int NU = (T1_LIMIT + 63) / 64;
    uint64_t e[NU], sv[NU];
    uint32_t qq[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {                                   // survivor loads first, table clear behind them
        const uint32_t s = (uint32_t) u * 64 + lane;
        e[u] = s < it.cnt ? it.rec[s] : 0ull;
        qq[u] = s < it.cnt ? it.recq[s] : 0u;
    }
    table_clear<64>(t, lane);
#pragma unroll
    for (int u = 0; u < NU; ++u) sv[u] = (uint32_t) (e[u] >> 40) == 1 ? sa_of_unique(ix, e[u]) : 0ull;       // unique seeds: gather at once (or nothing to gather)
    WaveStage st = {0, 0};                                           // one staging of all chunks: each goes behind the ones before it
#pragma unroll
    for (int u = 0; u < NU; ++u) st = stage_repeats_wave(L.off, L.srec, L.sq, e[u], qq[u], st, lane);
    // (peeling the most frequent buckets of a batch off with ballots + wave reductions, so that one lane adds a whole
    //  group of equal votes, measured SLOWER: 18.8 vs 13.4 ms per Gbp [r2] -- same-slot contention is not the cost)
#pragma unroll
    for (int u = 0; u < NU; ++u)
        if ((uint32_t) (e[u] >> 40) == 1) vote_admit(t, sv[u] - (uint64_t) (it.iter + qq[u] * v.P), qq[u] << v.tbits, 1u, 0u);
    if (st.n) vote_hits<64, VOTE_U>(ix, t, Staged{L.off, L.srec, L.sq, st.n, st.hits, it.iter, v.P, v.tbits}, lane, 1u, 0u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const Top2 w = table_top2<64>(t, lane);
    if (lane == 0) write_phase(it.out, phase_of(t, w.k1, w.s1, w.k2, w.s2));
    __builtin_amdgcn_wave_barrier();
}

// ---- workgroup tier -------------------------------------------------------------------------------------------
struct BlockLds {
    uint64_t key[T3_SLOTS];
    uint64_t srec[T3_CHUNK];
    uint64_t cf[T3_SLOTS];
    uint32_t off[T3_CHUNK + 4];
    uint32_t sq[T3_CHUNK];
};
union VoteLds { WaveLds w[4]; BlockLds b; };

struct KeyScratch { uint64_t *key; uint32_t *ord; uint32_t cap; };       // this workgroup's slice of the key scratch, in hits
struct GlobalPool { uint64_t *tab; uint32_t *lock; uint32_t slices, slots; uint32_t *s_slice; };   // global-memory tables; s_slice: LDS word

template <int VOTE_U>
__device__ __forceinline__ void vote_item_block(const LrmIndexView &ix, const VoteItems &v, const Item &it, uint32_t slots, uint32_t limit,
                                                BlockLds &L, uint32_t *s_wsum, Top2 *s_top, uint32_t *err_word, const KeyScratch &kc,
                                                const GlobalPool &gp) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t H = it.H, cnt = it.cnt;
    VoteTable t = {L.key, L.cf, slots};
    uint32_t passes = (H + limit - 1) / limit;
    // Items with more hits than the key scratch holds (a read made of a 100-299-copy repeat family: up to
    // cap_q * (thres - 1) hits per phase, 142 k for a 10 kbp read) would take H / 768 passes of H gathers each over
    // the 1024-slot LDS table -- quadratic, minutes for a batch of such reads.  They vote in ONE pass into a table in
    // global memory instead: the workgroup takes one of a few slices of a pool (a spin on a lock word: holders never
    // wait for anyone, so it always comes free), clears 2^k >= 2 H slots, inserts with the same compare-and-swap
    // protocol through L2, scans, gives the slice back.
    const bool big = gp.tab != nullptr && H > kc.cap && 2ull * H <= (uint64_t) gp.slots;
    if (big) {
        if (tid == 0) {
            uint32_t got = 0xFFFFFFFFu;
            for (uint32_t spin = 0; got == 0xFFFFFFFFu; ++spin) {
                const uint32_t sl = (blockIdx.x + spin) % gp.slices;
                if (atomicCAS(&gp.lock[sl], 0u, 1u) == 0u) got = sl;
                else __builtin_amdgcn_s_sleep(32);
            }
            *gp.s_slice = got;
        }
        __syncthreads();
        uint32_t gs = 1024;
        while (gs < 2 * H) gs <<= 1;
        uint64_t *base = gp.tab + (uint64_t) (*gp.s_slice) * 2ull * gp.slots;
        t.key = base; t.cf = base + gp.slots; t.slots = gs;
        passes = 1;
    }
    // Items that need several passes (ultra-long reads: ~3500 hits, five passes): the first pass writes every hit's
    // {key, order key} to this workgroup's slice of a global scratch, and the later passes stream them back
    // (12 coalesced bytes per hit) instead of searching, gathering and subtracting again.
    // (from three passes on: with two, writing and re-reading 12 B per hit costs as much traffic as it saves)
    const bool cache = passes > 2 && H <= kc.cap;
    if (!big) t.slots = table_slots_for(passes > 1 ? limit : H, v.load, slots);
    PhaseTop best = {};
    for (uint32_t pass = 0; pass < passes; ++pass) {
        table_clear<256>(t, tid);
        if (big) { __threadfence(); __syncthreads(); }             // the cleared slots are in L2 before the first atomic of another thread
        bool ok = true;
        if (cache && pass > 0) {
            __syncthreads();                                   // table cleared
            for (uint32_t i = tid; i < H; i += 256) ok &= vote_admit(t, kc.key[i], kc.ord[i], passes, pass);
        } else {
        uint32_t kbase = 0;                                    // hits of the chunks before this one
        for (uint32_t c0 = 0; c0 < cnt; c0 += T3_CHUNK) {
            const uint32_t nc = cnt - c0 < (uint32_t) T3_CHUNK ? cnt - c0 : (uint32_t) T3_CHUNK;
            // one survivor per thread; unique seeds gather at once, repeat seeds are compacted into LDS
            const uint64_t e0 = tid < nc ? it.rec[c0 + tid] : 0ull;
            const uint32_t q0 = tid < nc ? it.recq[c0 + tid] : 0u;
            const uint32_t r0 = (uint32_t) (e0 >> 40);
            const uint64_t v0 = r0 == 1 ? sa_of_unique(ix, e0) : 0ull;
            const BlockStage st = stage_repeats_block<true>(L.off, L.srec, L.sq, s_wsum, e0, q0, r0);
            if (r0 == 1) {
                const uint64_t key = v0 - (uint64_t) (it.iter + q0 * v.P);
                if (cache) { const uint32_t i = kbase + st.urank; kc.key[i] = key; kc.ord[i] = q0 << v.tbits; }
                ok &= vote_admit(t, key, q0 << v.tbits, passes, pass);
            }
            if (st.nbig) ok &= vote_hits<256, VOTE_U>(ix, t, Staged{L.off, L.srec, L.sq, st.nbig, st.total, it.iter, v.P, v.tbits}, tid, passes, pass,
                                                      cache ? kc.key + kbase + st.nuni : nullptr, cache ? kc.ord + kbase + st.nuni : nullptr);
            kbase += st.nuni + st.total;
        }
        if (cache) __threadfence_block();                      // the scratch is read back by other threads of the workgroup
        }
        if (!ok) *(volatile uint32_t *) err_word = LRM_ERR_VOTE_OVERFLOW;   // host-coherent, sticky
        if (big) __threadfence();
        __syncthreads();
        const Top2 w = big ? table_top2<256, true>(t, tid) : table_top2<256>(t, tid);                       // this wavefront's share of the table
        if (lane == 0) s_top[wave] = w;
        __syncthreads();
        if (tid == 0) {
            // the pass's top-2, merged into the running top-2 of the earlier passes (disjoint bucket sets).  Entries compare
            // as (count, first-seen) pairs.  (Merged in a copy: merging into `best` in place costs vote_kernel<8> scratch.)
            const Top2 c = block_top2(s_top);
            auto rank = [](const TopEntry &e) { return e.val ? ((uint64_t) e.val << 32) | (0xFFFFFFFFu - e.first) : 0ull; };
            const uint64_t cks[2] = {c.k1, c.k2};
            const uint32_t css[2] = {c.s1, c.s2};
            PhaseTop nb = best;
            uint64_t r1 = rank(best.a), r2 = rank(best.b);
            for (int x = 0; x < 2; ++x) {
                const uint64_t ck = cks[x];
                if (!ck) continue;
                const TopEntry e = entry_of(t, ck, css[x], big);
                if (ck > r1) { nb.b = nb.a; r2 = r1; nb.a = e; r1 = ck; }
                else if (ck > r2) { nb.b = e; r2 = ck; }
            }
            best = nb;
        }
        __syncthreads();
    }
    if (tid == 0) write_phase(it.out, best);
    if (big) {                                                     // the slice goes back to the pool
        __syncthreads();
        if (tid == 0) { __threadfence(); atomicExch(&gp.lock[*gp.s_slice], 0u); }
    }
}

// ---- fast path: one wavefront per item, repeat-only buckets never enter the table ------------------------------------------
// On a text with interspersed repeats most hits of an item come from a few REPEAT seeds (rr up to thres - 1 hits each)
// and land in buckets of their own, one or two votes each: on the bench workload 85 % of all hits, and what pushes an
// item from the 256-slot wavefront table into the workgroup tier and its passes.  They cannot win.  The vote's output is
// the top entry and the COUNT of the second (alnmain.c:374-388 reads cand[0] and cand[1].val only), so:
//   A  the hits of the UNIQUE seeds (rr == 1; at most one per survivor) are inserted as before -- table T;
//   B  a hit of a repeat seed is looked up in T with plain reads: present -> counted, and noted on a short LDS list (it may
//      hold its bucket's smallest key or earliest order); absent -> it belongs to a bucket made of repeat hits only, and
//      only a 16-bit counter of a small SKETCH (indexed by a hash of the bucket) is incremented -- no compare-and-swap,
//      no probe chain, no table space;
//   C  with t2 = the second-highest count in T and M = the largest sketch counter (>= the count of every repeat-only
//      bucket): if M < t2 no repeat-only bucket reaches the top two, and the top two of T are the item's result, bit for
//      bit.  Otherwise (few true hits, a read made of repeats, more step-B entries than the list holds) the item goes
//      on a list for the exact kernel above.
// The table only ever holds buckets of unique seeds (<= survivors <= T1_LIMIT), so an item needs one pass whatever its
// hit count, and a wavefront stages its repeat seeds 64 survivors at a time.  Items with more than T1_LIMIT survivors go
// to the exact kernel as well.
#define FAST_SK_WORDS 512                    // 1024 16-bit counters per wavefront
#define FB_LIMIT 1536                        // survivors up to which the workgroup form takes an item (75 % of its 2048 slots)

// The table of the fast kernels counts and nothing else: a slot is {u32 identity, u32 count} in two arrays.  A vote key is
// SA - j (u64 wrap): on a text of fewer than 2^35 rows it lies in [0, 2^35) or in [2^64 - 2^32, 2^64), so the low 32 bits
// of its bucket key >> 4 -- [0, 2^31) or [2^32 - 2^28, 2^32) -- name the bucket, and the bucket comes back from them
// (bucket_of_ident).  The launcher takes the fast kernels only on such a text (every text the project handles; the exact
// kernel has no such limit), and an item with a key outside the two ranges all the same (key_wide) is left to the exact
// kernel: exactness does not rest on the row count.  An insert is one 32-bit compare-and-swap and one 32-bit add; the min key and the first-seen
// order of a bucket are NOT kept current: only the top two buckets' are ever used, and they are properties of the HITS,
// which the lanes still hold when the table is final (the rank step below).
// (The exact kernel's slot is {u64 min key, u64 count << 32 | ~first}: a 64-bit compare-and-swap, sometimes a 64-bit min, an
//  add and a max per hit, and twice the LDS.)
#define EMPTY_ID 0x80000000u                 // in neither range
#define FAST_NONE 0xFFFFFFFFu                // no slot / no hit
struct FastTable { uint32_t *ident, *count; uint32_t slots; };
template <int NT>
__device__ __forceinline__ void table_clear(const FastTable &t, uint32_t tid) {
    for (uint32_t s = tid; s < t.slots; s += NT) { t.ident[s] = EMPTY_ID; t.count[s] = 0; }
}

// a key outside the two ranges (an index whose suffix-array values reach 2^35: the ui40 format holds 2^40): its bucket has
// no 32-bit name, and the item it belongs to goes to the exact kernel
__device__ __forceinline__ bool key_wide(uint64_t key) { return (uint32_t) (key >> 32) + 1u > 8u; }
__device__ __forceinline__ uint64_t bucket_of_ident(uint32_t id) {
    return id < 0x80000000u ? (uint64_t) id : (0x0FFFFFFF00000000ull | id);
}

// A: the slot of the bucket, claimed or found, with the hit counted; FAST_NONE if the table is full (never: both forms size
// the table above their survivor limit) -- the probe loop is bounded so a wave can never spin
__device__ __forceinline__ uint32_t fast_insert(const FastTable &t, uint32_t id, uint32_t hash) {
    uint32_t slot = (uint32_t) (((uint64_t) hash * t.slots) >> 32);
    for (uint32_t probe = 0; probe < t.slots; ++probe) {
        const uint32_t prev = atomicCAS(&t.ident[slot], EMPTY_ID, id);
        if (prev == EMPTY_ID || prev == id) { atomicAdd(&t.count[slot], 1u); return slot; }
        slot = slot + 1 == t.slots ? 0 : slot + 1;
    }
    return FAST_NONE;
}
// B: the slot of the bucket if the table has it (plain reads; no deletions: an empty slot ends the chain)
__device__ __forceinline__ uint32_t fast_find(const FastTable &t, uint32_t id, uint32_t hash) {
    uint32_t slot = (uint32_t) (((uint64_t) hash * t.slots) >> 32);
    for (uint32_t probe = 0; probe < t.slots; ++probe) {
        const uint32_t prev = t.ident[slot];
        if (prev == EMPTY_ID) return FAST_NONE;
        if (prev == id) return slot;
        slot = slot + 1 == t.slots ? 0 : slot + 1;
    }
    return FAST_NONE;
}

// A hit that counted in the table, as its lane keeps it: the word slot << 4 | (key & 15) -- the key is the bucket's
// identity and these four bits -- and its order key.  A repeat seed's hit that lands in a table bucket (step B) can lower
// that bucket's min key or its first-seen order, so it goes on a small LDS list as ~order << 32 | word and takes part in
// the rank step like the unique seeds' hits.  An item with more of them than the list holds goes to the exact kernel:
// exactness never depends on the capacity.
// Capacity of the wavefront form, 64 entries: on the bench batch (100 k x 10 kbp ONT reads, E. coli sized text with 5 %
// planted repeats, 2.1 M items) NO item has more than 32 -- a build with 32 entries and one with 64 leave the same 20 527
// items to the exact kernel as the kernels before them, which had no list (profiles/r4/README.md) -- and vote takes the
// same time with either (3.447 / 3.445 ms); 64 is one entry per lane of the rank step and 512 bytes.
#ifndef LRM_VOTE_FAST_LIST
#define LRM_VOTE_FAST_LIST 64
#endif
#define FAST_LIST LRM_VOTE_FAST_LIST
#define FB_LIST 512                          // workgroup form: items of up to FB_LIMIT survivors
__device__ __forceinline__ uint32_t hit_word(uint32_t slot, uint64_t key) { return (slot << 4) | ((uint32_t) key & 15u); }

// B over the staged repeat seeds, a sink of for_each_hit that every lane enters (it holds a ballot).  n_list: entries so far,
// a wave-uniform register in the wavefront form (NT == 64); the workgroup form counts in the LDS word list_n instead.
template <int NT, int VOTE_U>
__device__ __forceinline__ void fast_hits(const LrmIndexView &ix, const FastTable &t, const Staged &g, uint32_t *sketch, uint32_t sk_mask,
                                          uint32_t tid, uint64_t *list, uint32_t cap, uint32_t &n_list, uint32_t *list_n, bool &wide) {
    for_each_hit<NT, VOTE_U>(ix, g, tid, [&](bool live, uint32_t, uint64_t key, uint32_t order) __attribute__((always_inline)) {
        uint32_t hw = FAST_NONE, oinv = 0;
        if (live) {
            const uint32_t hash = bucket_hash(key >> 4);
            wide |= key_wide(key);
            const uint32_t slot = fast_find(t, (uint32_t) (key >> 4), hash);
            if (slot != FAST_NONE) {
                atomicAdd(&t.count[slot], 1u);
                hw = hit_word(slot, key);
                oinv = 0xFFFFFFFFu - order;
            } else {
                const uint32_t c = sketch_counter(hash, sk_mask);
                atomicAdd(&sketch[c >> 1], 1u << (16 * (c & 1)));          // < 2^16 hits per bucket: 16 per seed at most
            }
        }
        const unsigned long long bm = __ballot(hw != FAST_NONE);
        if (bm) {
            uint32_t base;
            if (NT == 64) { base = n_list; n_list += (uint32_t) __popcll(bm); }
            else {
                uint32_t b0 = 0;
                if ((tid & 63u) == 0) b0 = atomicAdd(list_n, (uint32_t) __popcll(bm));
                base = (uint32_t) __builtin_amdgcn_readfirstlane((int) b0);
            }
            if (hw != FAST_NONE) {
                const uint32_t i = base + mask_rank(bm);
                if (i < cap) list[i] = ((uint64_t) oinv << 32) | hw;
            }
        }
    });
}

// ---- the rank step: the stable top two from the hits ------------------------------------------------------------------
// "count descending, first-seen ascending" is a property of the hits: with the table final, hit h in slot s has
// r(h) = count[s] << 32 | ~order(h) (a plain LDS read), the winner is the slot of the hit with the largest r, the second the
// slot of the largest r among the hits outside the winner's slot, and their keys are the smallest keys among their hits --
// the bucket's identity and the smallest low four bits.  No table scan.  A 64-bit maximum is taken as two 32-bit ones (the
// count, then ~order among the lanes that hold it); the two minima of four bits come out of ONE 32-bit OR reduction of
// 0x8000 >> low4 (the winner's in the high half).
struct RankTop { uint64_t r; uint32_t s; };              // r == 0: none
__device__ __forceinline__ RankTop wave_top_rank(const RankTop &x) {
    const uint32_t hi = (uint32_t) (x.r >> 32), lo = (uint32_t) x.r;
    const uint32_t mh = wave_max_u32(hi);
    const uint32_t ml = wave_max_u32(hi == mh ? lo : 0u);
    RankTop w = {0, 0};
    if (mh) {
        const unsigned long long b = __ballot(hi == mh && lo == ml);       // order keys are unique per hit: one lane
        w.r = ((uint64_t) mh << 32) | ml;
        w.s = (uint32_t) __builtin_amdgcn_readlane((int) x.s, (int) __builtin_ctzll(b));
    }
    return w;
}
template <int N>
__device__ __forceinline__ RankTop lane_top_rank(const uint64_t (&hr)[N], const uint32_t (&hw)[N], uint32_t skip) {
    RankTop b = {0, 0};
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t s = hw[k] >> 4;
        if (hr[k] > b.r && s != skip) { b.r = hr[k]; b.s = s; }
    }
    return b;
}
template <int N>
__device__ __forceinline__ uint32_t lane_low4_mask(const uint64_t (&hr)[N], const uint32_t (&hw)[N], const RankTop &a, const RankTop &b) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t s = hw[k] >> 4, bit = 0x8000u >> (hw[k] & 15u);
        if (hr[k] && s == a.s) m |= bit << 16;
        else if (hr[k] && b.r && s == b.s) m |= bit;
    }
    return m;
}
__device__ __forceinline__ TopEntry fast_entry(const FastTable &t, const RankTop &w, uint32_t mask16) {
    TopEntry e = {0, 0, 0, 0};
    if (w.r) {
        e.bucket = bucket_of_ident(t.ident[w.s]);
        e.key = (e.bucket << 4) | (uint32_t) (__clz((int) mask16) - 16);
        e.val = (uint32_t) (w.r >> 32); e.first = 0xFFFFFFFFu - (uint32_t) w.r;
    }
    return e;
}

// the list entries (step B) of this thread of NT, i = l * NT + tid of the n_list entries (at most cap), as inputs of the rank
// step behind the thread's own hits: hw = the entry's word, hr = count << 32 | ~order with the table final
template <int NT, int NL, int N>
__device__ __forceinline__ void list_ranks(const FastTable &t, const uint64_t *list, uint32_t n_list, uint32_t cap, uint32_t tid,
                                           uint64_t (&hr)[N], uint32_t (&hw)[N]) {
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const uint32_t i = (uint32_t) l * NT + tid;
        hr[N - NL + l] = 0; hw[N - NL + l] = FAST_NONE;
        if (i < n_list && i < cap) {
            const uint64_t x = list[i];
            hw[N - NL + l] = (uint32_t) x;
            hr[N - NL + l] = ((uint64_t) t.count[(uint32_t) x >> 4] << 32) | (x >> 32);
        }
    }
}
// the largest 16-bit counter of a sketch of WORDS words, scanned by NT threads: this wavefront's maximum, in every lane
template <int NT, int WORDS>
__device__ __forceinline__ uint32_t sketch_max(const uint32_t *sketch, uint32_t tid) {
    static_assert(WORDS % NT == 0, "every thread scans WORDS / NT words");
    uint32_t m = 0;
#pragma unroll
    for (uint32_t s = 0; s < WORDS / NT; ++s) {
        const uint32_t x = sketch[s * NT + tid];
        const uint32_t lo = x & 0xffffu, hi = x >> 16;
        m = lo > m ? lo : m;
        m = hi > m ? hi : m;
    }
    return wave_max_u32(m);
}

// ---- fast path, wavefront form ------------------------------------------------------------------------------------------
struct FastLds {
    uint32_t ident[T1_SLOTS];
    uint32_t count[T1_SLOTS];
    uint64_t srec[64];
    uint64_t list[FAST_LIST];
    uint32_t off[64 + 4];
    uint32_t sq[64];
    uint32_t sketch[FAST_SK_WORDS];
};

// 64 VGPRs and 22.6 KB of LDS per workgroup: seven workgroups per CU (the 16-byte slots' 28.7 KB allowed five).  vote per
// 1-Gbp step, each kernel alone on the chip: 3.88 ms with five, 3.57 with six, 3.44 with seven [r4]
// (builds without the per-hit key_wide test, which adds about 0.05 ms to each)
#ifndef LRM_VOTE_FAST_WAVES
#define LRM_VOTE_FAST_WAVES (LRM_VOTE_FAST_GRID / 256)      // workgroups per CU == waves per SIMD
#endif
#define FAST_CH 16                           // items per ticket of a wavefront
template <int VOTE_U>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LRM_VOTE_FAST_WAVES, LRM_VOTE_FAST_WAVES)))
void vote_fast_kernel(LrmIndexView ix, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ recq, const uint32_t *__restrict__ gcnt,
                      const uint32_t *__restrict__ ghits, const uint8_t *__restrict__ decided, VoteItems v, unsigned long long *ticket, uint64_t *__restrict__ redo, unsigned long long *redo_n,
                      uint64_t *__restrict__ big, unsigned long long *big_n) {
    __shared__ FastLds lds[4];
    const uint32_t lane = threadIdx.x & 63u;
    FastLds &L = lds[threadIdx.x >> 6];
    const uint64_t n_items = v.n * (uint64_t) v.np;
    constexpr int NU = (T1_LIMIT + 63) / 64;
    constexpr int NL = (FAST_LIST + 63) / 64;
    for (;;) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(ticket, (unsigned long long) FAST_CH);
        base = ((unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) (base >> 32)) << 32) |
               (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) base);
        if (base >= n_items) break;
        ItemId ii = item_decode(base, v);                                      // once per ticket: its items follow by increments
        for (uint32_t it = 0; it < FAST_CH && base + it < n_items; ++it, ++ii.iter) {
            if (ii.iter == v.phase_lo + v.np) { ii.iter = v.phase_lo; ++ii.read; }
            const uint64_t item = base + it;
            const uint32_t iter = ii.iter;
            const uint64_t id = ii.read * (uint64_t) v.P + iter;
            if (decided && decided[ii.read]) continue;
            const uint32_t H = ghits[id], cnt = gcnt[id];
            if (H == 0) {
                if (lane == 0) { LrmPhaseRes z = {0, 0, 0, 0, 0, 0}; v.phase_res[id] = z; }
                continue;
            }
            if (cnt > (uint32_t) T1_LIMIT) {                                   // more survivors than the wavefront table is sized for:
                if (lane == 0) {                                               // the workgroup form of this kernel, or the exact kernel
                    if (cnt <= (uint32_t) FB_LIMIT) big[atomicAdd(big_n, 1ull)] = item;
                    else redo[atomicAdd(redo_n, 1ull)] = item;
                }
                continue;
            }
            const FastTable t = {L.ident, L.count, table_slots_for(cnt, v.load, T1_SLOTS)};
            uint64_t e[NU], sv[NU];
            uint32_t qq[NU];
            const uint64_t *irec = rec + id * v.cap_q;
            const uint32_t *iq = recq + id * v.cap_q;
#pragma unroll
            for (int u = 0; u < NU; ++u) {                                   // survivor loads first, clears behind them
                const uint32_t s = (uint32_t) u * 64 + lane;
                e[u] = s < cnt ? irec[s] : 0ull;
                qq[u] = s < cnt ? iq[s] : 0u;
            }
            table_clear<64>(t, lane);
            unsigned long long any_big = 0;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const uint32_t rr = (uint32_t) (e[u] >> 40);
                sv[u] = rr == 1 ? sa_of_unique(ix, e[u]) : 0ull;       // unique seeds: gather at once (or nothing to gather)
                any_big |= __ballot(rr > 1);
            }
            if (any_big) {                                             // the sketch is cleared and scanned only for items with a repeat seed
#pragma unroll
                for (uint32_t s = 0; s < FAST_SK_WORDS / 64; ++s) L.sketch[s * 64 + lane] = 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // A: the unique seeds' hits make the table; every lane keeps its hits (slot, low key bits; the order key is qq << tbits)
            uint64_t hr[NU + NL];
            uint32_t hw[NU + NL];
            bool wide = false;                                         // a key without a 32-bit bucket name
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                hw[u] = FAST_NONE;
                if ((uint32_t) (e[u] >> 40) == 1) {
                    const uint64_t key = sv[u] - (uint64_t) (iter + qq[u] * v.P);
                    wide |= key_wide(key);
                    const uint32_t slot = fast_insert(t, (uint32_t) (key >> 4), bucket_hash(key >> 4));
                    if (slot != FAST_NONE) hw[u] = hit_word(slot, key);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // B: the repeat seeds' hits, 64 survivors at a time
            uint32_t n_list = 0;
            if (any_big) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    if (__ballot((uint32_t) (e[u] >> 40) > 1) == 0) continue;             // a chunk without a repeat seed stages nothing
                    const WaveStage st = stage_repeats_wave(L.off, L.srec, L.sq, e[u], qq[u], WaveStage{0, 0}, lane);
                    fast_hits<64, VOTE_U>(ix, t, Staged{L.off, L.srec, L.sq, st.n, st.hits, iter, v.P, v.tbits}, L.sketch, 2 * FAST_SK_WORDS - 1, lane,
                                          L.list, (uint32_t) FAST_LIST, n_list, nullptr, wide);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            // rank: the top two from the hits (the table is final)
            bool lost = wide;                                          // ... or a hit without a slot: never (see fast_insert)
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const bool uniq = (uint32_t) (e[u] >> 40) == 1;
                lost |= uniq && hw[u] == FAST_NONE;
                hr[u] = uniq && hw[u] != FAST_NONE ? ((uint64_t) t.count[hw[u] >> 4] << 32) | (0xFFFFFFFFu - (qq[u] << v.tbits)) : 0ull;
            }
            list_ranks<64, NL>(t, L.list, n_list, (uint32_t) FAST_LIST, lane, hr, hw);
            const RankTop a = wave_top_rank(lane_top_rank(hr, hw, FAST_NONE));
            const RankTop b = wave_top_rank(lane_top_rank(hr, hw, a.r ? a.s : FAST_NONE));
            const uint32_t lowm = wave_or_u32(lane_low4_mask(hr, hw, a, b));
            // C
            bool settled = n_list <= (uint32_t) FAST_LIST && __ballot(lost) == 0;
            if (any_big) settled = settled && sketch_max<64, FAST_SK_WORDS>(L.sketch, lane) < (uint32_t) (b.r >> 32);
            if (lane == 0) {
                if (settled) write_phase(&v.phase_res[id], PhaseTop{fast_entry(t, a, lowm >> 16), fast_entry(t, b, lowm & 0xffffu)});
                else redo[atomicAdd(redo_n, 1ull)] = item;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// The same for items with up to FB_LIMIT survivors (reads of 100 kbp: ~1200 per item), one WORKGROUP per item: a
// 2048-slot table for the unique seeds' buckets, a 4096-counter sketch, repeat seeds staged 256 survivors at a time.
// One pass whatever the hit count (the exact kernel takes ceil(hits / 768) passes over its 1024-slot table: five on
// such reads).  Works through the list the wavefront kernel leaves (`big`).  A thread keeps up to FB_LIMIT / 256 hits.
#define FB_SLOTS 2048
#define FB_SK_WORDS 2048
struct FastBlockLds {
    uint32_t ident[FB_SLOTS];
    uint32_t count[FB_SLOTS];
    uint64_t srec[T3_CHUNK];
    uint64_t list[FB_LIST];
    uint32_t off[T3_CHUNK + 4];
    uint32_t sq[T3_CHUNK];
    uint32_t sketch[FB_SK_WORDS];
};
__device__ __forceinline__ RankTop block_top_rank(const RankTop *s_rk) {
    RankTop r = {0, 0};
    for (int x = 0; x < 4; ++x) if (s_rk[x].r > r.r) r = s_rk[x];
    return r;
}
template <int VOTE_U>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
void vote_fast_block_kernel(LrmIndexView ix, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ recq,
                            const uint32_t *__restrict__ gcnt, VoteItems v, unsigned long long *ticket, const uint64_t *__restrict__ big,
                            const unsigned long long *__restrict__ big_n, uint64_t *__restrict__ redo, unsigned long long *redo_n) {
    __shared__ FastBlockLds L;
    __shared__ uint32_t s_wsum[8], s_m[4], s_or[4], s_list_n;
    __shared__ RankTop s_rk[2][4];
    __shared__ unsigned long long s_at;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t n_big = (uint64_t) *big_n;
    constexpr int NU = FB_LIMIT / 256;
    constexpr int NL = FB_LIST / 256;
    for (;;) {
        if (tid == 0) { s_at = atomicAdd(ticket, 1ull); s_list_n = 0; }
        __syncthreads();
        const uint64_t at = s_at;
        if (at >= n_big) break;
        const uint64_t item = big[at];
        const ItemId ii = item_decode(item, v);
        const uint64_t id = ii.id;
        const uint32_t iter = ii.iter, cnt = gcnt[id];
        const uint64_t *irec = rec + id * v.cap_q;
        const uint32_t *iq = recq + id * v.cap_q;
        const FastTable t = {L.ident, L.count, table_slots_for(cnt, v.load, FB_SLOTS)};
        table_clear<256>(t, tid);
        __syncthreads();
        // A: the unique seeds' hits make the table; every thread keeps its hits
        bool ok = true;
        uint32_t any_big = 0;
        uint64_t hr[NU + NL];
        uint32_t hw[NU + NL], ho[NU];
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            const uint32_t s = (uint32_t) k * 256 + tid;
            hw[k] = FAST_NONE; ho[k] = 0;
            const uint64_t e0 = s < cnt ? irec[s] : 0ull;
            const uint32_t r0 = (uint32_t) (e0 >> 40);
            any_big |= r0 > 1 ? 1u : 0u;
            if (r0 == 1) {
                const uint32_t q0 = iq[s];
                const uint64_t key = sa_of_unique(ix, e0) - (uint64_t) (iter + q0 * v.P);
                const uint32_t slot = fast_insert(t, (uint32_t) (key >> 4), bucket_hash(key >> 4));
                ok &= slot != FAST_NONE && !key_wide(key);
                if (slot != FAST_NONE) { hw[k] = hit_word(slot, key); ho[k] = 0xFFFFFFFFu - (q0 << v.tbits); }
            }
        }
        const bool block_big = __syncthreads_or((int) any_big) != 0;
        // B: the repeat seeds' hits, 256 survivors at a time (the sketch is cleared and scanned only for items with a repeat seed)
        if (block_big) {
            for (uint32_t s = tid; s < FB_SK_WORDS; s += 256) L.sketch[s] = 0;       // (stage_repeats_block ends with a barrier)
            uint32_t unused = 0;
            bool wide = false;
            for (uint32_t c0 = 0; c0 < cnt; c0 += 256) {
                const uint64_t e0 = c0 + tid < cnt ? irec[c0 + tid] : 0ull;
                const uint32_t q0 = c0 + tid < cnt ? iq[c0 + tid] : 0u;
                const uint32_t r0 = (uint32_t) (e0 >> 40);
                const BlockStage st = stage_repeats_block<false>(L.off, L.srec, L.sq, s_wsum, e0, q0, r0);
                if (st.nbig) fast_hits<256, VOTE_U>(ix, t, Staged{L.off, L.srec, L.sq, st.nbig, st.total, iter, v.P, v.tbits}, L.sketch, 2 * FB_SK_WORDS - 1, tid,
                                                    L.list, (uint32_t) FB_LIST, unused, &s_list_n, wide);
                __syncthreads();                                   // the staging is rewritten by the next chunk
            }
            ok &= !wide;
        }
        // rank: the top two from the hits (the table is final: a barrier lies behind A and behind every chunk of B)
        const uint32_t n_list = s_list_n;
#pragma unroll
        for (int k = 0; k < NU; ++k)
            hr[k] = hw[k] != FAST_NONE ? ((uint64_t) t.count[hw[k] >> 4] << 32) | ho[k] : 0ull;
        list_ranks<256, NL>(t, L.list, n_list, (uint32_t) FB_LIST, tid, hr, hw);
        const RankTop wa = wave_top_rank(lane_top_rank(hr, hw, FAST_NONE));
        if (lane == 0) s_rk[0][wave] = wa;
        __syncthreads();
        const RankTop a = block_top_rank(s_rk[0]);
        const RankTop wb = wave_top_rank(lane_top_rank(hr, hw, a.r ? a.s : FAST_NONE));
        if (lane == 0) s_rk[1][wave] = wb;
        __syncthreads();
        const RankTop b = block_top_rank(s_rk[1]);
        const uint32_t lowm = wave_or_u32(lane_low4_mask(hr, hw, a, b));
        // C
        const uint32_t m = block_big ? sketch_max<256, FB_SK_WORDS>(L.sketch, tid) : 0u;
        if (lane == 0) { s_or[wave] = lowm; s_m[wave] = m; }
        const bool all_ok = __syncthreads_and((int) ok) != 0;
        if (tid == 0) {
            uint32_t M = 0, lm = 0;
            for (int x = 0; x < 4; ++x) { M = s_m[x] > M ? s_m[x] : M; lm |= s_or[x]; }
            const bool settled = all_ok && n_list <= (uint32_t) FB_LIST && (!block_big || M < (uint32_t) (b.r >> 32));
            if (settled) write_phase(&v.phase_res[id], PhaseTop{fast_entry(t, a, lm >> 16), fast_entry(t, b, lm & 0xffffu)});
            else redo[atomicAdd(redo_n, 1ull)] = item;
        }
        __syncthreads();                                           // s_at, s_list_n, the table and s_rk are rewritten by the next item
    }
}

#ifndef LRM_VOTE_WAVES_PER_EU
#define LRM_VOTE_WAVES_PER_EU 6     // 80 VGPRs (and a spill: DESIGN.md, "vote") and 23.5 KB of LDS per workgroup: six workgroups per CU
#endif
template <int VOTE_U>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LRM_VOTE_WAVES_PER_EU, LRM_VOTE_WAVES_PER_EU)))
void vote_kernel(LrmIndexView ix, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ recq, const uint32_t *__restrict__ gcnt,
                 const uint32_t *__restrict__ ghits, const uint8_t *__restrict__ decided, VoteItems v, uint32_t slots3, uint32_t limit3, uint32_t vg, uint32_t limit1, unsigned long long *ticket,
                 uint64_t *__restrict__ kc_key_all, uint32_t *__restrict__ kc_ord_all, uint32_t kc_cap, uint32_t *err_word,
                 const uint64_t *__restrict__ list, const unsigned long long *__restrict__ list_n, uint64_t *gtab, uint32_t *glock,
                 uint32_t g_slices, uint32_t g_slots) {
    __shared__ VoteLds lds;
    __shared__ uint32_t g_H[VG_MAX], g_cnt[VG_MAX], g_ph[VG_MAX];
    __shared__ uint64_t g_id[VG_MAX];
    __shared__ uint32_t s_wsum[12];
    __shared__ Top2 s_top[4];
    __shared__ unsigned long long s_grp;
    __shared__ uint32_t s_slice;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    // list mode: the items the fast kernel could not settle (vote_fast_kernel), by their item numbers
    const uint64_t n_items = list ? (uint64_t) *list_n : v.n * (uint64_t) v.np;
    const uint64_t n_groups = (n_items + vg - 1) / vg;
    const KeyScratch kc = {kc_key_all + (uint64_t) blockIdx.x * kc_cap, kc_ord_all + (uint64_t) blockIdx.x * kc_cap, kc_cap};
    const GlobalPool gp = {gtab, glock, g_slices, g_slots, &s_slice};
    // A fixed grid of resident workgroups takes groups of items from a ticket counter (dynamic balance, and one
    // scratch slice per workgroup); every workgroup ends with a ticket beyond the last group.
    for (;;) {
    if (tid == 0) s_grp = atomicAdd(ticket, 1ull);
    __syncthreads();
    const uint64_t grp = s_grp;
    if (grp >= n_groups) break;
    if (tid < vg) {
        const uint64_t li = grp * vg + tid;
        const uint64_t item = list && li < n_items ? list[li] : li;
        uint32_t H = 0, c = 0, ph = 0;
        uint64_t id = 0;
        if (li < n_items) {
            const ItemId ii = item_decode(item, v);
            ph = ii.iter; id = ii.id;                                        // (kept in LDS: decoding again per wavefront costs a 64-bit division)
            if (!(decided && decided[ii.read])) {
                H = ghits[id];
                c = gcnt[id];
                if (H == 0) { LrmPhaseRes z = {0, 0, 0, 0, 0, 0}; v.phase_res[id] = z; }
            }
        }
        g_H[tid] = H; g_cnt[tid] = c; g_id[tid] = id; g_ph[tid] = ph;
    }
    __syncthreads();
    for (uint32_t g = wave; g < vg; g += 4) {                 // wavefront tier: four items at a time
        const uint32_t H = g_H[g];
        if (H == 0 || H > limit1) continue;
        const uint64_t id = g_id[g];
        vote_item_wave<VOTE_U>(ix, v, Item{rec + id * v.cap_q, recq + id * v.cap_q, g_cnt[g], H, g_ph[g], &v.phase_res[id]}, lane, lds.w[wave]);
    }
    __syncthreads();
    for (uint32_t g = 0; g < vg; ++g) {                       // workgroup tier: one item after the other
        const uint32_t H = g_H[g];
        if (H <= limit1) continue;
        const uint64_t id = g_id[g];
        vote_item_block<VOTE_U>(ix, v, Item{rec + id * v.cap_q, recq + id * v.cap_q, g_cnt[g], H, g_ph[g], &v.phase_res[id]}, slots3, limit3, lds.b,
                                s_wsum, s_top, err_word, kc, gp);
        __syncthreads();
    }
    __syncthreads();                                          // s_grp, g_* are rewritten by the next round
    }
}

// ----------------------------------------------------------------------------------------
// host launcher
// ----------------------------------------------------------------------------------------
struct VoteKnobs { uint32_t t3_limit, t3_slots, vg, t1_limit, load; uint64_t *big_tab; };

// the launches of one round: the fast pair over all items and the exact kernel over the items they could not settle (their
// list), or the exact kernel over all items
template <int U>
static void launch_vote_u(lrm_index *idx, lrm_workspace *ws, const LrmVoteLaunch &v, const VoteKnobs &k, hipStream_t stream) {
    LrmDevCounters *c = ws->d_counters;
    const int r = v.round;
    const uint32_t np = (uint32_t) (v.phase_hi - v.phase_lo + 1);
    const uint64_t items = v.n * (uint64_t) np;
    const VoteItems vi = {v.n, (uint32_t) v.seed_len + 1, np, (uint32_t) v.phase_lo, ws->cap_q, v.tbits, k.load, ws->d_phase};
    const uint64_t *list = nullptr;
    const unsigned long long *list_n = nullptr;
    // the fast kernels name a bucket by 32 bits of it (FastTable): exact on a text of fewer than 2^35 rows, and only taken there
    const bool ident32 = idx->view.length < (1ull << 35);
    if (v.mt->vote_fast && ident32) {
        uint64_t fblocks = (items + 4 * FAST_CH - 1) / (4 * FAST_CH);
        if (fblocks > LRM_VOTE_FAST_GRID) fblocks = LRM_VOTE_FAST_GRID;
        hipLaunchKernelGGL(vote_fast_kernel<U>, dim3((uint32_t) fblocks), dim3(256), 0, stream, idx->view, ws->d_rec, ws->d_recq, ws->d_cnt, ws->d_hcount,
                           v.decided, vi, &c->vote_fast_ticket[r], ws->d_redo,
                           &c->vote_redo_n[r], ws->d_big, &c->vote_big_n[r]);
        const uint64_t bblocks = items < 768 ? items : 768;                     // three workgroups per CU
        hipLaunchKernelGGL(vote_fast_block_kernel<U>, dim3((uint32_t) bblocks), dim3(256), 0, stream, idx->view, ws->d_rec, ws->d_recq, ws->d_cnt, vi,
                           &c->vote_big_ticket[r],
                           (const uint64_t *) ws->d_big, (const unsigned long long *) &c->vote_big_n[r], ws->d_redo, &c->vote_redo_n[r]);
        list = ws->d_redo; list_n = &c->vote_redo_n[r];
    }
    uint64_t vblocks = (items + k.vg - 1) / k.vg;
    if (vblocks > LRM_VOTE_GRID) vblocks = LRM_VOTE_GRID;              // resident workgroups; groups of items go by ticket
    hipLaunchKernelGGL(vote_kernel<U>, dim3((uint32_t) vblocks), dim3(256), 0, stream, idx->view, ws->d_rec, ws->d_recq, ws->d_cnt,
                       ws->d_hcount, v.decided, vi, k.t3_slots, k.t3_limit, k.vg, k.t1_limit,
                       &c->vote_ticket[r], ws->d_kc_key, ws->d_kc_ord, (uint32_t) LRM_VOTE_KC_CAP, ws->d_err, list, list_n, k.big_tab, ws->d_glock,
                       ws->g_slices, ws->g_slots);
}

int lrm_launch_vote(lrm_index *idx, lrm_workspace *ws, const LrmVoteLaunch &v, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const LrmMapTune &mt = *v.mt;
    VoteKnobs k;
    // (tests force overflows of the multi-pass tier with a pass limit above the table size and a small table:
    //  lrm_debug_set_vote_limits)
    k.t3_limit = mt.t3_limit ? mt.t3_limit : (uint32_t) T3_LIMIT;
    k.t3_slots = mt.t3_slots >= 8 && mt.t3_slots <= T3_SLOTS ? mt.t3_slots : (uint32_t) T3_SLOTS;
    // tuning knobs (measured defaults; tools/seed_probe.py sweeps them through the environment, read at handle creation)
    k.vg = mt.vote_vg >= 1 && mt.vote_vg <= VG_MAX ? mt.vote_vg : VG;
    k.t1_limit = mt.vote_t1 <= T1_LIMIT ? mt.vote_t1 : (uint32_t) T1_LIMIT;
    k.load = mt.vote_load;          // percent of the table slots an item is sized for (when the table allows): at 75 % the
                                    // linear probes of the slowest lane cost +1.7 ms per Gbp [r2], at 90 % +4.4 ms
    k.big_tab = mt.t3_limit ? nullptr : ws->d_gtab;      // (the overflow-forcing test knobs keep the LDS passes)
    lrm_time_begin(ws, LRM_K_VOTE, stream);
    switch ((int) mt.vote_u) {
        case 2: launch_vote_u<2>(idx, ws, v, k, stream); break;
        case 8: launch_vote_u<8>(idx, ws, v, k, stream); break;
        default: launch_vote_u<4>(idx, ws, v, k, stream); break;
    }
    lrm_time_end(ws, stream);
    return 0;
}
