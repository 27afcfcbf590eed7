// anchor_kernels.hip -- gfx950 kernels of the ANCHORED extension mode (docs/GACT_SPEC.md, "Anchored extension")
//
//   anchor_scan     the longest exact match of a read on the LRM_ANCHOR_DIAGS diagonals around its voted locus
//   anchor_jobs     the job table (2 rows per read: right job, left job) and the job read rows
//   (extension)     ONE launch of the unchanged extension kernels over the job table (lrm_gact_run_jobs, extend_launch.hip)
//   anchor_clip     (lrm_map_options.clip) per job: the best-scoring prefix of its op bytes and what that prefix holds
//   anchor_stitch   reverse(left ops) ++ right ops into the caller's store, sums, moved meta, lrm_anchor records; with
//                   the clip records: the kept prefixes between runs of 'S'
//
// Scan: a wavefront takes one SEGMENT of one read and its 64 lanes take the 64 diagonals.  Per 32 read bases a lane
// builds one 32-bit mismatch word -- from the bit-planar images the bit-sliced extension already keeps (reads:
// bs_pack_reads, text: the index's planar copy), two 64-bit words of text funnel-shifted to the lane's diagonal and
// XORed with the read's word -- and carries the length of the run of equal bases that is open at the word's end.
// A run is counted by the segment it STARTS in: a lane first looks at the base before its segment (a run already open
// there belongs to the segment before), and after its last word it goes on, word by word, until the run still open
// has ended.  Runs that lie inside one word (no longer than 30 bases) are only looked for when a shift-and-AND test
// says the word holds 12 equal bases in a row (12 is the shortest anchor the option allows).  Reads or texts with a
// byte other than ACGT build the same mismatch words from bytes.  The best (length, |delta|, delta, j) of the lanes
// is reduced as one 64-bit key and merged into the read's key with one atomicMax per segment.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "lrm_hip_util.h"
#include "extend_stage.h"
#include "seq_bytes.h"
#include "anchor_clip.h"
#include "anchor_plan.h"                      // the key, AnPlan, the lrm_anchor record

#define AN_SEG_WORDS 64                       // words (of 32 bases) per scan segment: 2048 bases
#define AN_CHUNK 4096                         // bytes of a row one workgroup of the job / stitch kernels moves
static_assert(LRM_ANCHOR_DIAGS == 64, "one lane per diagonal");

struct LrmAnchorScratch {
    uint64_t n_max;
    uint32_t max_len;
    uint64_t *keys;                           // per read: best (length, |delta|, delta, j) as one word, 0 = none
    char *job_reads; uint64_t job_stride;     // 2 rows per read
    uint32_t *job_lens, *job_tlens;
    lrm_seq_meta *job_meta;
    int32_t *job_meta_r, *job_nops, *job_score;
    uint8_t *job_store; uint64_t job_store_stride;
    lrm_anchor *anchors;                      // used when the caller passes none
    uint4 *clip_recs;                         // end clipping, per job {keep, non_eq, non_I, non_D}: allocated by its first call
    LrmBsScratch bs;                          // bit-sliced extension over the job table
};

// ---- scan ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool an_is_acgt(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

struct AnScan {
    const uint64_t *qw;          // planar read words (null: bytes)
    const uint64_t *cpl;         // planar text, word 0 = bases 0..31
    const uint8_t *q, *text;     // bytes
    int64_t P0;                  // text position of read base 0 on this lane's diagonal
    int64_t S, E;                // the sequence [S, E)
    int n;

    // bit k set <=> read base 32w + k does NOT match the text on this diagonal (or lies outside the read / the sequence)
    __device__ __forceinline__ uint32_t mismatch(int w) const {
        const int b0 = 32 * w;
        const int64_t P = P0 + b0;
        const int64_t lo64 = S - P, hi64 = E - P;
        const int lo = lo64 > 0 ? (lo64 < 32 ? (int) lo64 : 32) : 0;
        int hi = hi64 < 32 ? (hi64 > 0 ? (int) hi64 : 0) : 32;
        hi = min(hi, n - b0);
        if (hi <= lo) return 0xFFFFFFFFu;
        uint32_t x;
        if (qw) {
            const uint64_t qv = qw[w];
            const int64_t wi = P >> 5;                 // >= -1 here: the planar text has padding words in front
            const uint32_t sh = (uint32_t) P & 31u;
            const uint64_t t0 = cpl[wi], t1 = cpl[wi + 1];
            const uint32_t tlo = __builtin_amdgcn_alignbit((uint32_t) t1, (uint32_t) t0, sh);
            const uint32_t thi = __builtin_amdgcn_alignbit((uint32_t) (t1 >> 32), (uint32_t) (t0 >> 32), sh);
            x = ((uint32_t) qv ^ tlo) | ((uint32_t) (qv >> 32) ^ thi);
        } else {
            x = 0;
            for (int k = lo; k < hi; ++k) {
                const uint32_t a = q[b0 + k], b = text[P + k];
                x |= (uint32_t) !(a == b && an_is_acgt(a)) << k;
            }
        }
        return x | ~bit_range<uint32_t>(lo, hi);
    }
};

__global__ __launch_bounds__(256) void anchor_scan_kernel(const char *__restrict__ reads, uint64_t stride,
                                                          const uint32_t *__restrict__ lens,
                                                          const lrm_seq_meta *__restrict__ meta,
                                                          const int32_t *__restrict__ meta_r, uint64_t n_reads,
                                                          const LrmMtaDev *__restrict__ mta, const char *__restrict__ content,
                                                          const uint64_t *__restrict__ qpl, uint64_t wpr,
                                                          const uint32_t *__restrict__ rflags,
                                                          const uint64_t *__restrict__ cpl, uint32_t min_len,
                                                          uint32_t segs_per_read, unsigned long long *__restrict__ keys) {
    const uint64_t wave_id = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint64_t r = wave_id / segs_per_read;
    if (r >= n_reads || !meta_r[r]) return;
    const int n = (int) lens[r];
    const int nw = (n + 31) >> 5;
    const int w0 = (int) (wave_id % segs_per_read) * AN_SEG_WORDS;
    if (w0 >= nw) return;
    const int w1 = min(w0 + AN_SEG_WORDS, nw);
    const lrm_seq_meta m = meta[r];
    const int delta = lane - AN_HALF;
    AnScan sc;
    const bool planar = qpl && cpl && !rflags[r];
    sc.qw = planar ? qpl + r * wpr + LRM_BS_PADW : nullptr;
    sc.cpl = cpl;
    sc.q = reinterpret_cast<const uint8_t *>(reads) + r * stride;
    sc.text = reinterpret_cast<const uint8_t *>(content);
    sc.P0 = (int64_t) m.loc + delta;
    sc.S = (int64_t) mta[m.seq_id].offset;
    sc.E = sc.S + (int64_t) mta[m.seq_id].seq_len;
    sc.n = n;

    uint32_t run = 0, best_len = 0, best_j = 0;
    bool own = true;                                 // the open run started in this segment
    if (w0 > 0 && !(sc.mismatch(w0 - 1) >> 31)) { run = 1; own = false; }
    int w = w0;
    for (;; ++w) {
        const bool in_seg = w < w1;
        const bool live = in_seg || (own && run > 0);    // past the segment only a run that is still open goes on
        if (!in_seg && (w >= nw || !__any(live))) break;
        if (live) {
            const uint32_t x = sc.mismatch(w);
            if (x == 0) {
                run += 32;
            } else {
                const uint32_t f = (uint32_t) __builtin_ctz(x), len = run + f;
                if (own && len >= min_len && len > best_len) { best_len = len; best_j = (uint32_t) (32 * w) + f - len; }
                run = 0;
                own = true;
                if (in_seg) {
                    const uint32_t h = (uint32_t) __builtin_clz(x);
                    // runs between the first and the last mismatch of the word
                    uint32_t z = ~x & ~((2u << f) - 1u) & (0x7FFFFFFFu >> h);
                    const uint32_t r2 = z & (z >> 1), r4 = r2 & (r2 >> 2), r8 = r4 & (r4 >> 4);
                    if (r8 & (r4 >> 8)) {
                        while (z) {
                            const uint32_t s = (uint32_t) __builtin_ctz(z);
                            const uint32_t l = (uint32_t) __builtin_ctz(~(z >> s));
                            if (l >= min_len && l > best_len) { best_len = l; best_j = (uint32_t) (32 * w) + s; }
                            z &= ~(((1u << l) - 1u) << s);
                        }
                    }
                    run = h;
                }
            }
        }
    }
    if (own && run >= min_len && run > best_len) { best_len = run; best_j = (uint32_t) (32 * w) - run; }

    const uint64_t key = wave_max_u64(best_len ? an_key(best_len, delta, best_j) : 0);     // 0 = none: the identity of the maximum
    if (lane == 0 && key) atomicMax(keys + r, (unsigned long long) key);
}

// ---- jobs ------------------------------------------------------------------------------------------------------------
// dst[k] = src[k] (right job) or comp(src[cnt - 1 - k]) (left job), k in [c0, c1): 16 bytes per thread, aligned stores
// (job rows are 16-byte aligned), the source at any byte (seq_bytes.h: the row steps of the gathers, with the one unaligned
// load that measured faster here).  The row's last bytes go one by one: nothing is written behind a job's length
template <bool REV>
__device__ __forceinline__ void an_fill_row(char *__restrict__ dst, const char *__restrict__ src, uint32_t cnt, uint32_t c0,
                                            uint32_t c1, uint32_t tid) {
    for (uint32_t k = c0 + 16 * tid; k < c1; k += 16 * 256) {
        if (k + 16 <= cnt) {
            *reinterpret_cast<uint4 *>(dst + k) = REV ? sp_row16_mirrored<true>(src + (cnt - k), 16u) : sp_row16<true>(src + k, 16u);
        } else {
            for (uint32_t e = k; e < cnt; ++e) dst[e] = REV ? comp_base(src[cnt - 1 - e]) : src[e];
        }
    }
}

__global__ __launch_bounds__(256) void anchor_jobs_kernel(const char *__restrict__ reads, uint64_t stride,
                                                          const uint32_t *__restrict__ lens,
                                                          const lrm_seq_meta *__restrict__ meta,
                                                          const int32_t *__restrict__ meta_r, uint64_t n_reads,
                                                          const LrmMtaDev *__restrict__ mta, uint64_t con_len,
                                                          unsigned long long *__restrict__ keys, uint32_t chunks_per_read,
                                                          char *__restrict__ job_reads, uint64_t job_stride,
                                                          uint32_t *__restrict__ job_lens, uint32_t *__restrict__ job_tlens,
                                                          lrm_seq_meta *__restrict__ job_meta, int32_t *__restrict__ job_meta_r) {
    const uint64_t r = blockIdx.x / chunks_per_read;
    const uint32_t chunk = blockIdx.x % chunks_per_read, tid = threadIdx.x;
    if (r >= n_reads) return;
    const bool mapped = meta_r[r] != 0;
    const uint32_t n = mapped ? lens[r] : 0;
    const lrm_seq_meta m = meta[r];
    AnPlan a = {};
    if (mapped) {
        const uint64_t S = mta[m.seq_id].offset, len_s = mta[m.seq_id].seq_len;
        // (a text that does not hold the reverse-complement half of the sequence cannot serve a left job)
        const uint64_t key = S + 2 * len_s <= con_len ? keys[r] : 0;
        a = an_plan(key, m.loc, n, S, len_s);
    }
    const bool anchored = a.flags & LRM_ANCHOR_ANCHORED;
    if (chunk == 0 && tid == 0) {
        lrm_seq_meta mr = m, ml = m;
        mr.loc = a.p;
        ml.loc = a.left_loc;
        job_meta[2 * r] = mr; job_meta[2 * r + 1] = ml;
        job_lens[2 * r] = anchored ? n - a.j : n;
        job_tlens[2 * r] = anchored ? a.right_tlen : n;
        job_meta_r[2 * r] = mapped;
        job_lens[2 * r + 1] = anchored ? a.j : 0;
        job_tlens[2 * r + 1] = a.left_tlen;
        job_meta_r[2 * r + 1] = anchored && a.j > 0;
        if (mapped && !anchored) keys[r] = 0;      // (only differs for the text without a reverse half)
    }
    if (!mapped) return;
    const char *src = reads + r * stride;
    const uint32_t j = anchored ? a.j : 0;
    const uint32_t c0 = chunk * AN_CHUNK;
    char *right = job_reads + 2 * r * job_stride, *left = right + job_stride;
    if (c0 < n - j) an_fill_row<false>(right, src + j, n - j, c0, min(c0 + AN_CHUNK, n - j), tid);
    if (c0 < j) an_fill_row<true>(left, src, j, c0, min(c0 + AN_CHUNK, j), tid);
}

// ---- clip ------------------------------------------------------------------------------------------------------------
// One wavefront per job.  Per step the wavefront takes 1024 op bytes of the job's row, 16 per lane with one aligned load
// (job rows are 16-byte aligned); a lane folds its columns into (sum, key) (anchor_clip.h), an inclusive scan of the sums
// places the lanes' keys in the step, their maximum is merged into the carried summary of the row.  With `keep` known, a
// second sweep over the kept prefix counts its columns other than '=', other than 'I' and other than 'D'.
__device__ __forceinline__ void an_clip_load(const uint8_t *row, uint32_t off, uint32_t m, uint32_t w[4]) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (off < m) v = *reinterpret_cast<const uint4 *>(row + off);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
__global__ __launch_bounds__(256) void anchor_clip_kernel(uint64_t n_jobs, const int32_t *__restrict__ job_meta_r,
                                                          const unsigned long long *__restrict__ keys,
                                                          const uint8_t *__restrict__ job_store, uint64_t job_store_stride,
                                                          const int32_t *__restrict__ job_nops, uint32_t P, uint32_t B,
                                                          uint4 *__restrict__ recs) {
    const uint64_t job = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (job >= n_jobs) return;
    const bool live = job_meta_r[job] != 0;
    const uint32_t m = live ? min((uint32_t) job_nops[job], (uint32_t) job_store_stride) : 0;
    if (!live || keys[job >> 1] == 0) {               // no job, or the single job of an unanchored read: kept whole
        if (lane == 0) recs[job] = make_uint4(m, 0, 0, 0);
        return;
    }
    const uint8_t *row = job_store + job * job_store_stride;
    AcSeg acc = ac_empty();
    for (uint32_t base = 0; base < m; base += 64 * AC_LANE_COLS) {
        const uint32_t off = base + AC_LANE_COLS * lane;
        uint32_t w[4];
        an_clip_load(row, off, m, w);
        const AcSeg l = ac_fold16(w, off < m ? m - off : 0, P);
        const uint32_t incl = wave_incl_scan((uint32_t) l.sum);
        const uint64_t placed = ac_key_move(l.key, (int32_t) (incl - (uint32_t) l.sum), AC_LANE_COLS * lane);
        AcSeg step;
        step.key = wave_max_u64(placed);
        step.sum = __builtin_amdgcn_readlane((int) incl, 63);
        acc = ac_merge(acc, base, step);
    }
    const uint32_t keep = ac_keep(acc, m, B);
    uint32_t non_eq = 0, non_i = 0, non_d = 0;
    for (uint32_t base = 0; base < keep; base += 64 * AC_LANE_COLS) {
        const uint32_t off = base + AC_LANE_COLS * lane;
        uint32_t w[4];
        an_clip_load(row, off, keep, w);
        const uint32_t nv = off < keep ? keep - off : 0;
        non_eq += ac_count_not(w, nv, '=');
        non_i += ac_count_not(w, nv, 'I');
        non_d += ac_count_not(w, nv, 'D');
    }
    non_eq = wave_incl_scan(non_eq); non_i = wave_incl_scan(non_i); non_d = wave_incl_scan(non_d);
    if (lane == 63) recs[job] = make_uint4(keep, non_eq, non_i, non_d);       // the last lane holds the totals
}

// ---- stitch ----------------------------------------------------------------------------------------------------------
// the whole 24-byte record, padding included: the mode's meta is the same bytes whatever the buffer held before
__device__ __forceinline__ void an_store_meta(lrm_seq_meta *dst, uint64_t loc, uint64_t off, int32_t seq_id, uint8_t strand) {
    static_assert(sizeof(lrm_seq_meta) == 24, "three words");
    uint64_t *w = reinterpret_cast<uint64_t *>(dst);
    w[0] = loc; w[1] = off; w[2] = (uint64_t) (uint32_t) seq_id | ((uint64_t) strand << 32);
}
struct __attribute__((packed, aligned(1))) An16 { uint32_t x, y, z, w; };     // 16 op bytes at any address, loaded or stored
__global__ __launch_bounds__(256) void anchor_stitch_kernel(const uint32_t *__restrict__ lens,
                                                            lrm_seq_meta *__restrict__ meta,
                                                            const int32_t *__restrict__ meta_r, uint64_t n_reads,
                                                            const LrmMtaDev *__restrict__ mta,
                                                            const unsigned long long *__restrict__ keys,
                                                            uint32_t chunks_per_read,
                                                            const uint8_t *__restrict__ job_store, uint64_t job_store_stride,
                                                            const int32_t *__restrict__ job_nops,
                                                            const int32_t *__restrict__ job_score,
                                                            uint8_t *__restrict__ store, uint64_t store_stride,
                                                            int32_t *__restrict__ n_ops, int32_t *__restrict__ score,
                                                            lrm_anchor *__restrict__ anchors,
                                                            const uint4 *__restrict__ clip_recs, lrm_clip *__restrict__ clip_out) {
    __shared__ uint32_t s_cnt[4];
    const uint64_t r = blockIdx.x / chunks_per_read;
    const uint32_t chunk = blockIdx.x % chunks_per_read, tid = threadIdx.x;
    if (r >= n_reads) return;
    if (!meta_r[r]) {
        if (chunk == 0 && tid == 0) {
            n_ops[r] = 0; score[r] = -1;
            an_store_meta(meta + r, 0, 0, -1, 0);
            lrm_anchor z = {};
            anchors[r] = z;
            if (clip_out) clip_out[r] = lrm_clip{0, 0};
        }
        return;
    }
    const lrm_seq_meta m = meta[r];
    const uint64_t S = mta[m.seq_id].offset, len_s = mta[m.seq_id].seq_len;
    const AnPlan a = an_plan(keys[r], m.loc, lens[r], S, len_s);
    const bool left = (a.flags & LRM_ANCHOR_ANCHORED) && a.j > 0;
    // end clipping (anchored reads only): the jobs' kept prefixes stand for the jobs, cl / cr query bases become 'S'
    const bool clip = clip_recs && (a.flags & LRM_ANCHOR_ANCHORED);
    const uint4 rec_r = clip ? clip_recs[2 * r] : make_uint4(0, 0, 0, 0);
    const uint4 rec_l = clip && left ? clip_recs[2 * r + 1] : make_uint4(0, 0, 0, 0);
    const uint32_t nr = clip ? rec_r.x : (uint32_t) job_nops[2 * r];
    const uint32_t nl = clip ? rec_l.x : left ? (uint32_t) job_nops[2 * r + 1] : 0;
    const uint32_t cl = clip ? a.j - rec_l.w : 0, cr = clip ? (lens[r] - a.j) - rec_r.w : 0;
    const uint32_t b0 = cl, b1 = cl + nl, b2 = b1 + nr, total = b2 + cr;      // 'S' | reversed left | right | 'S'
    const uint8_t *rrow = job_store + 2 * r * job_store_stride, *lrow = rrow + job_store_stride;
    uint8_t *out = store + r * store_stride;
    const uint32_t c1 = min((chunk + 1) * AN_CHUNK, total);
    for (uint32_t o = chunk * AN_CHUNK + 16 * tid; o < c1; o += 16 * 256) {
        An16 v;
        if (o >= b0 && o + 16 <= b1) {             // reversed left ops
            const An16 s = *reinterpret_cast<const An16 *>(lrow + (b1 - 16 - o));
            v.x = __builtin_bswap32(s.w); v.y = __builtin_bswap32(s.z); v.z = __builtin_bswap32(s.y); v.w = __builtin_bswap32(s.x);
            *reinterpret_cast<An16 *>(out + o) = v;
        } else if (o >= b1 && o + 16 <= b2) {      // right ops
            *reinterpret_cast<An16 *>(out + o) = *reinterpret_cast<const An16 *>(rrow + (o - b1));
        } else if (o + 16 <= b0 || (o >= b2 && o + 16 <= total)) {
            v.x = v.y = v.z = v.w = 0x53535353u;   // 'S'
            *reinterpret_cast<An16 *>(out + o) = v;
        } else {                                   // a group that straddles a seam, or the tail
            for (uint32_t e = o; e < o + 16 && e < total; ++e)
                out[e] = e < b0 || e >= b2 ? (uint8_t) 'S' : e < b1 ? lrow[b1 - 1 - e] : rrow[e - b1];
        }
    }
    if (chunk != 0) return;
    // target bases the left job consumed: its columns other than 'I' (with the clip records: counted there)
    uint32_t cnt = 0;
    for (uint32_t o = tid; o < (clip ? 0u : nl); o += 256) cnt += lrow[o] != (uint8_t) 'I';
    cnt = wave_incl_scan(cnt);
    if ((tid & 63) == 63) s_cnt[tid >> 6] = cnt;               // the last lane holds the wavefront's total
    __syncthreads();
    if (tid != 0) return;
    const uint32_t consumed = clip ? rec_l.z : s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    n_ops[r] = (int32_t) total;
    score[r] = clip ? (int32_t) (rec_l.y + rec_r.y) : job_score[2 * r] + (left ? job_score[2 * r + 1] : 0);
    anchors[r] = an_record(a, b1, (cl ? LRM_ANCHOR_SOFT_LEFT : 0u) | (cr ? LRM_ANCHOR_SOFT_RIGHT : 0u));
    if (clip_out) clip_out[r] = lrm_clip{cl, cr};
    if (a.flags & LRM_ANCHOR_ANCHORED) {           // meta moves to the alignment's first text base
        an_store_meta(meta + r, a.p - consumed, a.p - consumed - S, m.seq_id, m.strand);
    } else {
        an_store_meta(meta + r, m.loc, m.off, m.seq_id, m.strand);
    }
}

// ----------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------
void lrm_anchor_scratch_free(lrm_workspace *ws) {
    LrmAnchorScratch *s = ws ? ws->an : nullptr;
    if (!s) return;
    lrm_dev_free({s->keys, s->job_reads, s->job_lens, s->job_tlens, s->job_meta, s->job_meta_r, s->job_nops, s->job_score,
                  s->job_store, s->anchors, s->clip_recs});
    lrm_bs_scratch_free(&s->bs);
    delete s;
    ws->an = nullptr;
}

// Scratch of the mode, sized once from the workspace's batch shape: 2 n_max jobs, job reads of up to max_len bases,
// targets of up to len + ceil(len / 8) bases (so up to lrm_anchored_store_stride(max_len) op bytes and 2-bit codes per job).
static int anchor_scratch(lrm_workspace *ws, bool planar) {
    if (ws->an) return 0;
    LrmAnchorScratch *s = new (std::nothrow) LrmAnchorScratch();
    if (!s) { lrm_set_error("out of memory"); return -1; }
    ws->an = s;
    const uint64_t n = ws->n_max, jobs = 2 * n;
    s->n_max = n; s->max_len = ws->max_len;
    s->job_stride = ((uint64_t) ws->max_len + 31) & ~15ull;
    s->job_store_stride = (lrm_anchored_store_stride(ws->max_len) + 15) & ~15ull;
    const LrmDevAlloc allocs[] = {
        {(void **) &s->keys, n * 8},
        {(void **) &s->job_reads, jobs * s->job_stride},
        {(void **) &s->job_lens, jobs * 4},
        {(void **) &s->job_tlens, jobs * 4},
        {(void **) &s->job_meta, jobs * sizeof(lrm_seq_meta)},
        {(void **) &s->job_meta_r, jobs * 4},
        {(void **) &s->job_nops, jobs * 4},
        {(void **) &s->job_score, jobs * 4},
        {(void **) &s->job_store, jobs * s->job_store_stride},
        {(void **) &s->anchors, n * sizeof(lrm_anchor)},
    };
    if (lrm_dev_alloc_table(allocs, "bytes of anchored-mode scratch", &ws->bytes) ||
        (planar && lrm_bs_scratch_alloc(&s->bs, jobs, ws->max_len, ws->max_len + ws->max_len / 16 + 2, &ws->bytes))) {
        lrm_anchor_scratch_free(ws);
        return -1;
    }
    return 0;
}

// the records of the clip step: with the first call that has the step on
static int anchor_clip_scratch(lrm_workspace *ws) {
    LrmAnchorScratch *s = ws->an;
    if (s->clip_recs) return 0;
    const uint64_t bytes = 2 * s->n_max * sizeof(uint4);
    if (hipMalloc((void **) &s->clip_recs, bytes) != hipSuccess) {
        s->clip_recs = nullptr;
        lrm_set_error("hipMalloc of %llu bytes of end-clipping scratch failed", (unsigned long long) bytes);
        return -1;
    }
    ws->bytes += bytes;
    return 0;
}

// P and B of the clip step: 0 selects the default
static int anchor_clip_params(LrmClipOpt *c) {
    if (!c->on) return 0;
    if (c->penalty == 0) c->penalty = LRM_CLIP_PENALTY_DEFAULT;
    if (c->end_bonus == 0) c->end_bonus = LRM_CLIP_END_BONUS_DEFAULT;
    if (c->penalty > 15) { lrm_set_error("clip_penalty %u outside [1, 15]", c->penalty); return -1; }
    if (c->end_bonus > 255) { lrm_set_error("clip_end_bonus %u outside [1, 255]", c->end_bonus); return -1; }
    return 0;
}

int lrm_anchor_min_len(uint32_t min_len, uint32_t *out) {
    if (min_len == 0) min_len = LRM_ANCHOR_MIN_DEFAULT;
    if (min_len < 12 || min_len > 64) { lrm_set_error("anchor_min_len %u outside [12, 64]", min_len); return -1; }
    *out = min_len;
    return 0;
}

int lrm_anchor_scan(const LrmExtendBatch &b, const LrmIndexView &ix, const LrmBsScratch &pl, const uint64_t *cpl,
                    uint32_t min_len, uint64_t *keys, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const uint32_t nw = (b.max_len + 31) / 32;
    const uint32_t segs = nw ? (nw + AN_SEG_WORDS - 1) / AN_SEG_WORDS : 1;
    uint32_t grid;
    if (lrm_grid_1d((b.n * segs + 3) / 4, "anchor scan", &grid)) return -1;
    HIPCHK(hipMemsetAsync(keys, 0, b.n * 8, stream));
    hipLaunchKernelGGL(anchor_scan_kernel, dim3(grid), dim3(256), 0, stream, b.reads, b.stride, b.lens, b.meta, b.meta_r, b.n,
                       ix.mta, ix.content, cpl ? pl.qpl : nullptr, pl.wpr, pl.rflags, cpl ? cpl + LRM_BS_PADW : nullptr,
                       min_len, segs, (unsigned long long *) keys);
    return 0;
}

int lrm_launch_extend_anchored(lrm_index *idx, lrm_workspace *ws, const LrmExtendBatch &b, lrm_gact_params gp,
                               lrm_anchor *d_anchor, uint32_t min_len, const LrmClipOpt &clip_, const LrmMapTune &mt,
                               void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const uint64_t n = b.n;
    if (n == 0) return 0;
    LrmClipOpt clip = clip_;
    if (lrm_gact_resolve_params(&gp) || lrm_anchor_min_len(min_len, &min_len) || anchor_clip_params(&clip)) return -1;
    if (b.store_stride < lrm_anchored_store_stride(b.max_len)) {
        lrm_set_error("anchored extension: store_stride %llu < 2*max_len + max_len/8 + 2 = %llu",
                      (unsigned long long) b.store_stride, (unsigned long long) lrm_anchored_store_stride(b.max_len));
        return -1;
    }
    if (!(ws->parts & LRM_WS_EXTEND) || n > ws->n_max || b.max_len > ws->max_len) {
        lrm_set_error("anchored extension: workspace too small (have n=%llu len=%u with%s extension scratch, need n=%llu len=%u)",
                      (unsigned long long) ws->n_max, ws->max_len, (ws->parts & LRM_WS_EXTEND) ? "" : "out",
                      (unsigned long long) n, b.max_len);
        return -1;
    }
    const bool planar = lrm_planar_ready(idx, ws);
    if (anchor_scratch(ws, planar) || (clip.on && anchor_clip_scratch(ws))) return -1;
    LrmAnchorScratch &s = *ws->an;
    const LrmGactJobs jobs = {s.job_reads, s.job_stride, s.job_lens, s.job_tlens, s.job_meta, s.job_meta_r, idx->view.content,
                              idx->d_cpl, 2 * n, s.job_store, s.job_store_stride, s.job_nops, s.job_score};
    LrmGactPlan plan;
    if (lrm_gact_plan(jobs, gp, mt.gact_impl, planar, &plan)) return -1;
    if (lrm_launch_locus_revcomp(idx, ws, b, stream_)) return -1;

    // anchor: planar image of the oriented reads, then the scan
    lrm_time_begin(ws, LRM_K_LOCUS, stream);
    if (planar && lrm_bs_pack_reads(b.reads, b.stride, b.lens, n, b.max_len, ws->bs, stream)) return -1;
    if (lrm_anchor_scan(b, idx->view, ws->bs, planar ? idx->d_cpl : nullptr, min_len, s.keys, stream)) return -1;
    lrm_time_end(ws, stream);

    // jobs
    const uint32_t chunks_rd = b.max_len ? (b.max_len + AN_CHUNK - 1) / AN_CHUNK : 1;
    uint32_t grid;
    if (lrm_grid_1d(n * chunks_rd, "anchor jobs", &grid)) return -1;
    lrm_time_begin(ws, LRM_K_REVCOMP, stream);
    hipLaunchKernelGGL(anchor_jobs_kernel, dim3(grid), dim3(256), 0, stream, b.reads, b.stride, b.lens, b.meta, b.meta_r, n,
                       idx->view.mta, idx->view.con_len, (unsigned long long *) s.keys, chunks_rd, s.job_reads, s.job_stride,
                       s.job_lens, s.job_tlens, s.job_meta, s.job_meta_r);
    lrm_time_end(ws, stream);

    // one extension launch over the job table
    if (lrm_gact_run_jobs(ws, jobs, b.max_len, gp, plan, s.bs, ws->d_counters, mt.bs_waves, stream)) return -1;

    // clip: one wavefront per job
    if (clip.on) {
        if (lrm_grid_1d((2 * n + 3) / 4, "anchor clip", &grid)) return -1;
        lrm_time_begin(ws, plan.slot, stream);
        hipLaunchKernelGGL(anchor_clip_kernel, dim3(grid), dim3(256), 0, stream, 2 * n, s.job_meta_r,
                           (const unsigned long long *) s.keys, s.job_store, s.job_store_stride, s.job_nops, clip.penalty,
                           clip.end_bonus, s.clip_recs);
        lrm_time_end(ws, stream);
    }

    // stitch
    const uint64_t ops_max = lrm_anchored_store_stride(b.max_len);
    const uint32_t chunks_op = (uint32_t) ((ops_max + AN_CHUNK - 1) / AN_CHUNK);
    if (lrm_grid_1d(n * chunks_op, "anchor stitch", &grid)) return -1;
    lrm_time_begin(ws, plan.slot, stream);
    hipLaunchKernelGGL(anchor_stitch_kernel, dim3(grid), dim3(256), 0, stream, b.lens, b.meta, b.meta_r, n, idx->view.mta,
                       (const unsigned long long *) s.keys, chunks_op, s.job_store, s.job_store_stride, s.job_nops,
                       s.job_score, b.store, b.store_stride, b.n_ops, b.score, d_anchor ? d_anchor : s.anchors,
                       clip.on ? s.clip_recs : nullptr, clip.on ? clip.d_clip : nullptr);
    lrm_time_end(ws, stream);
    HIPCHK(hipGetLastError());
    return 0;
}
