// secondary_kernels.hip -- gfx950 kernels of the SECONDARY ALIGNMENTS stage (docs/GACT_SPEC.md, "Secondary alignments"):
// where the rival locus of the mapping-quality vote is, and the read extended there
//
//   rival_locus     one workgroup per read: the fullest (histogram, bucket) pair of the rival vote, its fullest sub-bucket,
//                   the smallest hit of that -- an lrm_entry the extension can start from (zeros: not a candidate)
//   compact_count / compact_scan / (host) / compact_mark<SecRule>   the candidate table in its order (compact_rows.h):
//                   a candidate's lrm_secondary record, its length and its rival entry
//   compact_gather<SecRule>   the read AS SEQUENCED into row s of the candidate batch (the primary extension
//                   reverse-complemented reverse-strand reads in place: those are read mirrored and complemented), zeros
//                   from the read's end to the end of the row
//   (extension)     lrm_launch_extend / lrm_launch_extend_anchored, unchanged, over the rows with best = the rival entries
//   sec_flag        LRM_SEC_DUPLICATE and LRM_SEC_ALIGNED
//
// rival_locus goes over the survivor lists the seed kernel left in the workspace, as mapq_vote_kernel did (mapq_kernels.hip),
// TWICE.  Pass 1 rebuilds that kernel's pair table -- the same LDS table, the same mq_insert, the same number of slots -- and
// finds the fullest pair with one 64-bit maximum of count << 32 | ~tag: the largest count, then the smallest tag.  Pass 2
// counts the hits of that pair in direct-indexed sub-buckets (2048 x {count, smallest offset}, in the memory of the pair table)
// with one LDS atomicAdd and one LDS atomicMin per hit; one sweep for count << 32 | ~index ends it.  Counts are sums and keys
// are minima: nothing depends on the scheduling.  A read that is not a candidate (rival_rule.h: arithmetic on its 16-byte
// lrm_mapq record) leaves after reading that record.
// The walk is the shared one of the vote kernels (vote_hits.h: stage_repeats_wave, for_each_hit), a wavefront per chunk of 64
// survivors; mapq_vote_kernel keeps its own copy for the 1.8 % it measured (mapq_kernels.hip) and is not touched.
//
// Order of the table: exclusive prefix sums without atomics, as in split_kernels.hip (compact_rows.h: the one copy of it).
#include <hip/hip_runtime.h>
#include "vote_hits.h"
#include "rival_rule.h"
#include "mapq_table.h"
#include "compact_rows.h"
#include "extend_stage.h"
#include "seq_bytes.h"

struct LrmSecScratch {
    lrm_entry *rival; uint64_t rival_cap;     // the rival entry of every read of the batch
    LrmCompactScratch c;                      // the candidate table's order
};

// every hit SA[row] - j of the phases 0 .. d of one read, chunks of 64 survivors dealt round-robin to the four wavefronts:
// sink(key) in the lane that holds the hit
template <typename Sink>
__device__ __forceinline__ void rv_walk(const LrmIndexView &ix, MqWaveLds &W, const uint64_t *__restrict__ rec,
                                        const uint32_t *__restrict__ recq, const uint32_t *__restrict__ g_cnt, uint64_t read,
                                        uint32_t P, uint32_t cap_q, uint32_t d, uint32_t wave, uint32_t lane, Sink sink) {
    uint32_t item = 0;
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
            const bool uniq = (uint32_t) (e >> 40) == 1;
            const uint64_t sv = uniq ? sa_of_unique(ix, e) : 0ull;
            const WaveStage st = stage_repeats_wave(W.off, W.srec, W.sq, e, q, WaveStage{0, 0}, lane);
            if (uniq) sink(sv - (uint64_t) (ph + q * P));
            const Staged g = {W.off, W.srec, W.sq, st.n, st.hits, ph, P, 0};
            for_each_hit<64, MQ_U>(ix, g, lane, [&](bool live, uint32_t, uint64_t key, uint32_t) { if (live) sink(key); });
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();                                  // the lists are free for the next chunk
        }
    }
}

// the maximum of v over the workgroup, in every thread (s_m: four words of LDS; two barriers)
__device__ __forceinline__ uint64_t rv_block_max(uint64_t v, uint64_t *s_m, uint32_t wave, uint32_t lane) {
    v = wave_max_u64(v);
    __syncthreads();                                                          // s_m of an earlier call has been read
    if (lane == 0) s_m[wave] = v;
    __syncthreads();
    uint64_t m = 0;
#pragma unroll
    for (int w = 0; w < MQ_WAVES; ++w) m = s_m[w] > m ? s_m[w] : m;
    return m;
}

__device__ __forceinline__ void rv_store_entry(lrm_entry *out, uint64_t key, uint64_t val, uint64_t bucket) {
    const uint64_t kv[2] = {key, val};
    __builtin_memcpy(out, kv, 16);                                            // (entries are 8-byte aligned)
    out->bucket = bucket;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
void rival_locus_kernel(LrmIndexView ix, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ recq,
                        const uint32_t *__restrict__ g_cnt, const uint32_t *__restrict__ lens,
                        const uint8_t *__restrict__ phase_d, const lrm_entry *__restrict__ best,
                        const lrm_mapq *__restrict__ mapq, uint64_t n, uint32_t P, uint32_t cap_q, uint32_t slots, uint32_t H,
                        uint32_t pct, lrm_entry *__restrict__ out) {
    __shared__ MqLds L;
    __shared__ uint64_t s_m[MQ_WAVES];
    const uint64_t read = blockIdx.x;
    if (read >= n) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (tid >> 6));
    const uint4 q = *reinterpret_cast<const uint4 *>(mapq + read);            // n1, n2, radius, mapq | phase << 8 | flags << 16
    if (!rv_candidate(q.x, q.y, (q.w >> 16) & 0xFFu, H, pct)) {               // uniform: the whole workgroup leaves
        if (tid == 0) rv_store_entry(out + read, 0ull, 0ull, 0ull);
        return;
    }
    const uint64_t best_key = best[read].key;
    const uint32_t r = mq_radius_log2(lens[read]);
    const uint32_t d = phase_d[read] < P ? phase_d[read] : P - 1u;
    for (uint32_t s = tid; s < slots; s += 256) { L.tag[s] = MQ_TAG_EMPTY; L.count[s] = 0u; }
    if (tid == 0) L.overflow = 0u;
    __syncthreads();

    // pass 1: the pair table of mapq_vote_kernel
    MqWaveLds &W = L.w[wave];
    rv_walk(ix, W, rec, recq, g_cnt, read, P, cap_q, d, wave, lane, [&](uint64_t key) {
        if (mq_inside(key, best_key, r)) return;
        if (!mq_insert(L, mq_tag(key, r, 0u), slots) || !mq_insert(L, mq_tag(key, r, 1u), slots)) L.overflow = 1u;
    });
    __syncthreads();
    uint64_t m = 0;                                                           // the fullest pair; ties: the smallest tag
    for (uint32_t s = tid; s < slots; s += 256) {
        const uint32_t c = L.count[s];
        const uint64_t v = ((uint64_t) c << 32) | (uint32_t) ~L.tag[s];
        m = c && v > m ? v : m;
    }
    m = rv_block_max(m, s_m, wave, lane);
    // (a candidate's record has no overflow flag and the table has the slots it had then: the switch never fires; a full
    //  table would leave some hits uncounted, so such a read gets the zero entry)
    if (L.overflow || m == 0) {
        if (tid == 0) rv_store_entry(out + read, 0ull, 0ull, 0ull);
        return;
    }
    const uint32_t wtag = ~(uint32_t) m, h = wtag & 1u;
    const uint32_t sub_shift = rv_sub_shift(r);
    const uint32_t n_sub = (2u << r) >> sub_shift;                            // <= RV_SUB_BUCKETS
    uint32_t *sub_cnt = L.count, *sub_min = L.tag;                            // the pair table has been read (barriers of rv_block_max)
    for (uint32_t s = tid; s < n_sub; s += 256) { sub_cnt[s] = 0u; sub_min[s] = 0xFFFFFFFFu; }
    __syncthreads();

    // pass 2: the hits of the winning pair into its sub-buckets
    rv_walk(ix, W, rec, recq, g_cnt, read, P, cap_q, d, wave, lane, [&](uint64_t key) {
        if (mq_inside(key, best_key, r) || mq_tag(key, r, h) != wtag) return;
        const uint32_t off = rv_off(key, r, h);
        atomicAdd(&sub_cnt[off >> sub_shift], 1u);
        atomicMin(&sub_min[off >> sub_shift], off);
    });
    __syncthreads();
    uint64_t b = 0;                                                           // the fullest sub-bucket; ties: the smallest index
    for (uint32_t s = tid; s < n_sub; s += 256) {
        const uint32_t c = sub_cnt[s];
        const uint64_t v = ((uint64_t) c << 32) | (uint32_t) ~s;
        b = c && v > b ? v : b;
    }
    b = rv_block_max(b, s_m, wave, lane);
    if (tid == 0) {
        const uint32_t at = ~(uint32_t) b;
        const uint64_t key = b ? rv_key_of(wtag, r, sub_min[at]) : 0ull;
        rv_store_entry(out + read, key, b >> 32, b ? key >> 4 : 0ull);
    }
}
static_assert(RV_SUB_BUCKETS <= LRM_MAPQ_SLOTS, "the sub-buckets live in the pair table's memory");

// ---- the candidate table -----------------------------------------------------------------------------------------------------
// the stage's rule: a candidate read is one row, as long as the read
struct SecRule {
    const char *__restrict__ reads; uint64_t stride; const lrm_seq_meta *__restrict__ meta; const int32_t *__restrict__ meta_r;
    const lrm_mapq *__restrict__ mapq; const uint32_t *__restrict__ lens; const lrm_entry *__restrict__ rival; uint32_t H, pct;
    lrm_secondary *__restrict__ table; uint32_t *__restrict__ sec_lens; lrm_entry *__restrict__ sec_rival;
    struct Item {};                                                           // (the record is made of r alone)
    __device__ uint32_t items(uint64_t n, uint64_t r, Item &, uint32_t &longest) const {
        if (r >= n) return 0;
        const uint4 q = *reinterpret_cast<const uint4 *>(mapq + r);
        if (!rv_candidate(q.x, q.y, (q.w >> 16) & 0xFFu, H, pct)) return 0;
        longest = lens[r];
        return 1;
    }
    __device__ void write(uint64_t r, const Item &, uint32_t, uint64_t at, uint64_t cap) const {
        if (at >= cap) return;
        const lrm_entry e = rival[r];
        *reinterpret_cast<uint4 *>(table + at) = make_uint4((uint32_t) r, (uint32_t) e.val, 0u, 0u);
        sec_lens[at] = lens[r];
        rv_store_entry(sec_rival + at, e.key, e.val, e.bucket);
    }
    // the gather: the whole read; mirrored when the primary extension turned it round
    static constexpr bool MIRRORS = true;
    __device__ CompactSpan span(uint64_t s) const { return CompactSpan{reads + (uint64_t) table[s].read * stride, sec_lens[s]}; }
    __device__ bool mirrored(uint64_t s) const {
        const uint32_t read = table[s].read;
        return meta && meta_r[read] != 0 && meta[read].strand == 1;
    }
    __device__ static uint64_t zeros_to(uint32_t, uint64_t row_stride) { return row_stride; }
};

// one lane per candidate.  anchored: LRM_SEC_ALIGNED needs an anchor of the candidate's own
__global__ __launch_bounds__(256) void sec_flag_kernel(lrm_secondary *__restrict__ table, const uint32_t *__restrict__ sec_lens,
                                                       const lrm_seq_meta *__restrict__ meta_p, const int32_t *__restrict__ meta_r_p,
                                                       const lrm_seq_meta *__restrict__ meta, const int32_t *__restrict__ meta_r,
                                                       const int32_t *__restrict__ score, const lrm_anchor *__restrict__ anchor,
                                                       uint64_t n_sec) {
    const uint64_t s = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (s >= n_sec) return;
    const uint32_t read = table[s].read;
    const lrm_seq_meta none = {0, 0, -1, 0};
    table[s].flags = lrm_sec_flags(meta_p != nullptr, meta_p ? meta_r_p[read] : 0, meta_p ? meta_p[read] : none, meta_r[s], meta[s],
                                   score[s], sec_lens[s], anchor != nullptr, anchor ? anchor[s].flags : 0u);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
void lrm_sec_scratch_free(lrm_workspace *ws) {
    LrmSecScratch *s = ws ? ws->sec : nullptr;
    if (!s) return;
    lrm_dev_free({s->rival});
    lrm_compact_scratch_free(&s->c);
    free(s);
    ws->sec = nullptr;
}

// the stage's own scratch, sized once from the workspace: a rival entry per read, the order's 8 bytes per 256 reads
// (what a failed call did allocate stays, booked, for the next call and for lrm_sec_scratch_free)
static int sec_scratch(lrm_workspace *ws) {
    if (!ws->sec && !(ws->sec = (LrmSecScratch *) calloc(1, sizeof(LrmSecScratch)))) { lrm_set_error("out of memory"); return -1; }
    LrmSecScratch *s = ws->sec;
    if (lrm_compact_scratch(ws, &s->c, (ws->n_max + SP_BLOCK - 1) / SP_BLOCK, "secondary")) return -1;
    if (s->rival) return 0;
    if (hipMalloc((void **) &s->rival, ws->n_max * sizeof(lrm_entry)) != hipSuccess) {
        (void) hipGetLastError();
        lrm_set_error("hipMalloc of %llu bytes of secondary-stage scratch failed", (unsigned long long) (ws->n_max * sizeof(lrm_entry)));
        return -1;
    }
    s->rival_cap = ws->n_max;
    ws->bytes += ws->n_max * sizeof(lrm_entry);
    return 0;
}

int lrm_launch_rival(lrm_index *idx, lrm_workspace *ws, const uint32_t *d_lens, uint64_t n, uint32_t seed_len, const lrm_entry *d_best,
                     const lrm_mapq *d_mapq, uint32_t min_hits, uint32_t ratio_pct, lrm_entry *d_rival, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    uint32_t H, pct;
    if (lrm_rival_options(min_hits, ratio_pct, &H, &pct)) return -1;
    if (n == 0) return 0;
    if (!ws->d_mq_phase || !ws->d_rec || seed_len != ws->seed_len || n > ws->n_max || !lrm_seed_stamp_is(ws, d_best, n)) {
        lrm_set_error("rival locus: the workspace did not run the seed stage of this batch with the phase output");
        return -1;
    }
    const uint32_t slots = idx->dbg_mapq_slots ? idx->dbg_mapq_slots : (uint32_t) LRM_MAPQ_SLOTS;     // as the records were made
    uint32_t grid;
    if (lrm_grid_1d(n, "rival_locus", &grid)) return -1;
    lrm_time_begin(ws, LRM_K_DECIDE, stream);
    hipLaunchKernelGGL(rival_locus_kernel, dim3(grid), dim3(256), 0, stream, idx->view, (const uint64_t *) ws->d_rec,
                       (const uint32_t *) ws->d_recq, (const uint32_t *) ws->d_cnt, d_lens, (const uint8_t *) ws->d_mq_phase, d_best,
                       d_mapq, n, ws->P, ws->cap_q, slots, H, pct, d_rival);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int lrm_launch_secondary(lrm_index *idx, lrm_workspace *ws, const LrmSecArgs &a, const lrm_secondary_dev &out, uint64_t *n_sec_out,
                         void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const uint64_t n = a.n;
    uint32_t H, pct;
    if (n > ws->n_max) { lrm_set_error("secondary: %llu reads, the workspace holds %llu", (unsigned long long) n, (unsigned long long) ws->n_max); return -1; }
    if (lrm_rival_options(a.min_hits, a.ratio_pct, &H, &pct) || sec_scratch(ws)) return -1;
    LrmSecScratch &s = *ws->sec;
    if (int rc = lrm_launch_rival(idx, ws, a.lens, n, a.seed_len, a.best, a.mapq, a.min_hits, a.ratio_pct, s.rival, stream_)) return rc;
    const uint32_t n_blk = (uint32_t) ((n + SP_BLOCK - 1) / SP_BLOCK);

    const SecRule rule = {a.reads, a.stride, a.meta, a.meta_r, a.mapq, a.lens, s.rival, H, pct, out.table, out.lens, out.rival};
    uint64_t n_sec;
    uint32_t longest;
    if (lrm_compact_count(ws, s.c, rule, n, n_blk, stream, &n_sec, &longest)) return -1;
    *n_sec_out = n_sec;
    dim3 grid;                                                       // (chunks over the whole row: the gather fills it with zeros to its end)
    const int room = lrm_compact_room(ws, LrmCompactNouns{"secondary", "secondary candidates", "candidate"}, n_sec, longest, out.cap, out.row_stride,
                                      out.store_stride, a.anchored ? lrm_anchored_store_stride(longest) : 2ull * longest, out.row_stride, &grid);
    if (room || n_sec == 0) return room;
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(compact_mark_kernel<SecRule>, dim3(n_blk), dim3(SP_BLOCK), 0, stream, rule, n, (const uint2 *) s.c.blk, out.cap);
    hipLaunchKernelGGL(compact_gather_kernel<SecRule>, grid, dim3(256), 0, stream, rule, n_sec, out.rows, out.row_stride);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());

    // the candidate batch through the unchanged extension stage (n_sec <= n <= ws->n_max: one call)
    const LrmMapTune &mt = idx->mtune;
    const LrmExtendBatch b = {out.rows, out.row_stride, out.lens, n_sec, longest, out.rival, out.store, out.store_stride, out.n_ops,
                              out.score, out.meta, out.meta_r};
    if (a.anchored) {
        const LrmClipOpt clip = a.clip ? LrmClipOpt{1, a.clip_penalty, a.clip_end_bonus, out.clip} : LrmClipOpt{};
        if (int rc = lrm_launch_extend_anchored(idx, ws, b, a.gp, out.anchor, a.anchor_min_len, clip, mt, stream_)) return rc;
    } else if (int rc = lrm_launch_extend(idx, ws, b, a.gp, mt, stream_)) return rc;
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(sec_flag_kernel, dim3((uint32_t) ((n_sec + 255) / 256)), dim3(256), 0, stream, out.table, (const uint32_t *) out.lens,
                       a.meta, a.meta_r, (const lrm_seq_meta *) out.meta, (const int32_t *) out.meta_r, (const int32_t *) out.score,
                       a.anchored ? (const lrm_anchor *) out.anchor : (const lrm_anchor *) nullptr, n_sec);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());
    return 0;
}
