// lrm_host.hip -- the host-buffer entry points of liblrm_accel.so (the drop-in boundary):
//   lrm_map_batch          PART 1 + PART 2 of single_end() for one batch in ONE device pass (alnmain.c:333-451)
//   lrm_map_batch_submit   the same, asynchronous: up to two batches per device in flight (the batch loop
//   lrm_map_batch_wait       alnmain.c:302-330 with the copy clauses the reference planned at :420-424)
//   lrm_seed_batch         PART 1 alone (alnmain.c:333-405)
//   lrm_extend_batch       PART 2 alone (alnmain.c:408-451)
// on one device or on a multi-GPU group handle (reads partitioned by bases, every replica writes its slice of the
// caller's arrays in place -- SURVEY 8(b)/(e)).
// The pipeline that runs a submitted batch (slots, issuer and collector threads, staging) is host_pipeline.hip; here a
// batch is checked, cut into slices per replica and queued, and its ticket awaited.
#include <cstring>
#include <exception>
#include "host_pipeline.h"
#include "pileup_step.h"                       // LRM_PILEUP_MAX_STRIDE
#include "../../include/lrm_io_host.h"     // lrm_parse_cigar: the CIGAR text of the secondary pass

namespace {

uint32_t max_of(const uint32_t *lens, uint64_t n) {
    uint32_t m = 0;
    for (uint64_t i = 0; i < n; ++i) m = lens[i] > m ? lens[i] : m;
    return m;
}

// Reads per device pass: the per-batch scratch is ~13 bytes per read base (seed records, op bytes, codes, packed
// copies), so very large caller batches (the reference's sweeps use up to 1 M reads, gen-sbatch-scripts.py:74) go
// through the device in slices of ~32 GB of scratch, two of them in flight.  Results do not depend on the slicing:
// there is no cross-read state.
uint64_t host_slice_reads(uint32_t max_len, const LrmMapTune &mt) {
    if (mt.slice_reads >= 1) return mt.slice_reads;
    const uint64_t per_read = 13ull * (max_len ? max_len : 1) + 4096;
    uint64_t r = (32ull << 30) / per_read;
    return r < 16384 ? 16384 : r;
}
// contiguous slices balanced by cumulative bases, not by read count (100 kbp reads next to 1 kbp ones)
void partition_by_bases(const uint32_t *lens, uint64_t n, int parts, std::vector<uint64_t> &cuts) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) total += lens[i];
    cuts.assign((size_t) parts + 1, n);
    cuts[0] = 0;
    uint64_t acc = 0, i = 0;
    for (int r = 1; r < parts; ++r) {
        const uint64_t target = (uint64_t) ((__uint128_t) total * (uint64_t) r / (uint64_t) parts);
        while (i < n && acc < target) acc += lens[i++];
        cuts[r] = i;
    }
}

// queue the slices of one replica's share of the batch
int submit_replica(lrm_index *ix, const MapJob &j, const LrmMapTune &mt, lrm_ticket *t, int group_size) {
    if (j.n == 0) return 0;
    if (lrm_host_ensure_ctx(ix, group_size)) return -1;
    LrmHostCtx &c = *ix->host;
    const uint32_t max_len = max_of(j.lens, j.n);
    const uint64_t slice = host_slice_reads(max_len, mt);
    std::vector<std::unique_ptr<SliceJob>> jobs;
    for (uint64_t o = 0; o < j.n; o += slice) {
        std::unique_ptr<SliceJob> sj(new SliceJob);
        sj->j = j.slice(o, j.n - o < slice ? j.n - o : slice);
        sj->mt = mt;
        sj->ticket = t;
        sj->max_len = max_len;
        jobs.push_back(std::move(sj));
    }
    { std::lock_guard<std::mutex> g(t->m); t->pending += (int) jobs.size(); }
    {
        std::lock_guard<std::mutex> lk(c.mu);
        for (auto &sj : jobs) { c.q_issue.push_back(std::move(sj)); ++c.n_active; }
    }
    c.cv.notify_all();
    return 0;
}

// piles: one accumulator per replica (lrm_batch_pileup, checked by the entry point), or null
int submit_impl(lrm_index *idx, const MapJob &j, const lrm_map_options *opt, lrm_ticket **out, uint64_t *diff_needed_out = nullptr,
                lrm_pileup *const *piles = nullptr) {
    LrmMapTune mt = idx->mtune;
    if (opt) lrm_call_map_tune(idx, opt, &mt);
    const uint32_t max_len = max_of(j.lens, j.n);
    if (j.stride < max_len) { lrm_set_error("stride < longest read"); return -1; }
    if ((j.mode & DO_EXTEND) && j.store_stride < 2ull * max_len) { lrm_set_error("store_stride < 2 * longest read (alnmain.c:316-320)"); return -1; }
    if ((j.mode & DO_EXTEND) && mt.clip && !mt.anchored) { lrm_set_error("lrm_map_options.clip needs lrm_map_options.anchored"); return -1; }
    if ((j.mode & DO_EXTEND) && mt.anchored && j.store_stride < lrm_anchored_store_stride(max_len)) {
        lrm_set_error("anchored extension: store_stride %llu < 2 * longest read + longest read / 8 + 2 = %llu",
                      (unsigned long long) j.store_stride, (unsigned long long) lrm_anchored_store_stride(max_len));
        return -1;
    }
    if ((j.mode & DO_EXTEND) && mt.dense && (j.store_stride & 15u)) { lrm_set_error("dense results need store_stride to be a multiple of 16"); return -1; }
    if (j.diff_off && ((j.store_stride + 3) & ~3ull) > (1ull << 22)) {
        lrm_set_error("difference events: store_stride %llu above 2^22 (the '=' count of an event has 22 bits)", (unsigned long long) j.store_stride);
        return -1;
    }
    std::unique_ptr<lrm_ticket> t(new lrm_ticket);
    t->diff_needed_out = diff_needed_out;
    if (j.n) {
        if (idx->n_peers <= 1 || !idx->peers) {
            if (submit_replica(idx, j, mt, t.get(), 1)) return -1;
        } else {
            const int np = idx->n_peers;
            std::vector<uint64_t> cuts;
            partition_by_bases(j.lens, j.n, np, cuts);
            for (int r = 0; r < np; ++r) {
                const uint64_t lo = cuts[r], hi = cuts[r + 1];
                if (hi <= lo) continue;
                MapJob jr = j.slice(lo, hi - lo);
                jr.pile = piles ? piles[r] : nullptr;
                if (submit_replica(idx->peers[r], jr, mt, t.get(), np)) {
                    // the replicas queued so far run to completion before the caller gets its buffers back
                    const std::string msg = lrm_last_error();
                    { std::unique_lock<std::mutex> lk(t->m); t->cv.wait(lk, [&] { return t->pending == 0; }); }
                    lrm_set_error("replica %d (device %d): %s", r, idx->peers[r]->device, msg.c_str());
                    return -1;
                }
            }
        }
    }
    *out = t.release();
    return 0;
}

int wait_impl(lrm_ticket *t) {
    int rc;
    {
        std::unique_lock<std::mutex> lk(t->m);
        t->cv.wait(lk, [&] { return t->pending == 0; });
        rc = t->rc;
        if (rc) lrm_set_error("%s", t->err.c_str());
        if (t->diff_needed_out) *t->diff_needed_out = t->diff_total.load();
    }
    delete t;
    return rc;
}

// C ABI: no C++ exception may leave the library (allocation failures of the host-side bookkeeping, thread creation)
int run_job(lrm_index *idx, const MapJob &j, const lrm_map_options *opt, lrm_ticket **ticket_out, uint64_t *diff_needed_out = nullptr,
            lrm_pileup *const *piles = nullptr) {
    try {
        lrm_ticket *t = nullptr;
        if (submit_impl(idx, j, opt, &t, diff_needed_out, piles)) return -1;
        if (ticket_out) { *ticket_out = t; return 0; }
        return wait_impl(t);
    } catch (const std::exception &e) {
        lrm_set_error("host-side failure: %s", e.what());
        return -1;
    } catch (...) {
        lrm_set_error("host-side failure");
        return -1;
    }
}

}  // namespace

extern "C" int lrm_seed_batch(lrm_index *idx, const char *reads_buf, uint64_t stride, const uint32_t *lens,
                              uint64_t n, lrm_params p, lrm_entry *best_out) {
    if (!idx || !reads_buf || !lens || !best_out) { lrm_set_error("null argument"); return -1; }
    MapJob j = {};
    j.mode = DO_SEED; j.reads = const_cast<char *>(reads_buf); j.stride = stride; j.lens = lens; j.n = n; j.p = p; j.best_out = best_out;
    return run_job(idx, j, nullptr, nullptr);
}

extern "C" int lrm_extend_batch(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                                const lrm_entry *best, lrm_gact_params gp, lrm_cigar *cig_out, uint8_t *store_mem,
                                uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out, int *meta_r_out) {
    if (!idx || !reads_buf || !lens || !best || !cig_out || !store_mem || !score_out || !meta_out || !meta_r_out) {
        lrm_set_error("null argument");
        return -1;
    }
    MapJob j = {};
    j.mode = DO_EXTEND; j.reads = reads_buf; j.stride = stride; j.lens = lens; j.n = n; j.gp = gp; j.best_in = best;
    j.p.seed_len = 20; j.p.thres = 300;                              // only sizes the workspace when none is cached yet
    j.cig = cig_out; j.store_mem = store_mem; j.store_stride = store_stride; j.score = score_out; j.meta = meta_out; j.meta_r = meta_r_out;
    return run_job(idx, j, nullptr, nullptr);
}

static int map_job_of(MapJob &j, lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                      lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out, uint8_t *store_mem,
                      uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out, int *meta_r_out) {
    if (!idx || !reads_buf || !lens || !best_out || !cig_out || !store_mem || !score_out || !meta_out || !meta_r_out) {
        lrm_set_error("null argument");
        return -1;
    }
    j = MapJob{};
    j.mode = DO_SEED | DO_EXTEND; j.reads = reads_buf; j.stride = stride; j.lens = lens; j.n = n; j.p = p; j.gp = gp;
    j.best_out = best_out;
    j.cig = cig_out; j.store_mem = store_mem; j.store_stride = store_stride; j.score = score_out; j.meta = meta_out; j.meta_r = meta_r_out;
    return 0;
}

extern "C" int lrm_map_batch(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                             lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out, uint8_t *store_mem,
                             uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out, int *meta_r_out) {
    MapJob j;
    if (map_job_of(j, idx, reads_buf, stride, lens, n, p, gp, best_out, cig_out, store_mem, store_stride, score_out, meta_out, meta_r_out)) return -1;
    return run_job(idx, j, nullptr, nullptr);
}

// The per-call extras (lrm_batch_extras).  mapq_out: the mapping-quality stage behind every seed sub-batch (docs/GACT_SPEC.md,
// "Mapping quality"); summary_out: the alignment summary stage behind every group's extension ("Alignment summary and PAF").
// diff: the difference events on top (lrm_batch_diff; docs/GACT_SPEC.md, "Difference events and MD:Z"): the stage runs when every
// extension group is collected, into the one buffer the whole batch shares.
// pile: one accumulator per replica (lrm_batch_pileup; docs/GACT_SPEC.md, "Pileup on the host-buffer path and across replicas"):
// every extension group is added to its replica's accumulator behind its extension.
extern "C" int lrm_map_batch_submit_ex3(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                                        lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                                        uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                                        int *meta_r_out, const lrm_map_options *opt, const lrm_batch_extras *ex,
                                        const lrm_batch_diff *diff, const lrm_batch_pileup *pile, lrm_ticket **ticket_out) {
    if (!ticket_out) { lrm_set_error("null argument"); return -1; }
    MapJob j;
    if (map_job_of(j, idx, reads_buf, stride, lens, n, p, gp, best_out, cig_out, store_mem, store_stride, score_out, meta_out, meta_r_out)) return -1;
    if (ex) {                                                        // as many fields as the caller's struct holds (0: all)
        const size_t have = ex->struct_size ? ex->struct_size : sizeof(*ex);
        if (have >= offsetof(lrm_batch_extras, mapq_out) + sizeof(ex->mapq_out)) j.mapq_out = ex->mapq_out;
        if (have >= offsetof(lrm_batch_extras, summary_out) + sizeof(ex->summary_out)) j.summary_out = ex->summary_out;
    }
    lrm_pileup *const *piles = nullptr;
    if (pile) {                                                      // checked before anything of the request is written or queued
        if (pile->struct_size < sizeof(lrm_batch_pileup)) { lrm_set_error("lrm_batch_pileup.struct_size %u: the struct has %zu bytes", pile->struct_size, sizeof(lrm_batch_pileup)); return -1; }
        if (pile->reserved != 0u) { lrm_set_error("lrm_batch_pileup.reserved is %u, not 0", pile->reserved); return -1; }
        const int np = lrm_index_replicas(idx);
        if (!pile->pileups || pile->n_pileups != (uint32_t) np) { lrm_set_error("lrm_batch_pileup: %u accumulators for a handle of %d replicas (one per replica)", pile->pileups ? pile->n_pileups : 0u, np); return -1; }
        for (int r = 0; r < np; ++r) {
            const lrm_pileup *pl = pile->pileups[r];
            if (!pl) { lrm_set_error("lrm_batch_pileup: pileups[%d] is NULL", r); return -1; }
            if (pl->idx != lrm_index_replica(idx, r)) { lrm_set_error("lrm_batch_pileup: pileups[%d] was not created on replica %d of this handle", r, r); return -1; }
        }
        if (pile->min_mapq != 0u && !j.mapq_out) { lrm_set_error("lrm_batch_pileup.min_mapq needs lrm_batch_extras.mapq_out (the filter reads the records of the mapping-quality stage)"); return -1; }
        if (store_stride > LRM_PILEUP_MAX_STRIDE) { lrm_set_error("pileup: store_stride %llu above 2^31 (the column counts of a row are 32-bit)", (unsigned long long) store_stride); return -1; }
        piles = pile->pileups;
        j.pile = piles[0];
        j.pile_min_mapq = pile->min_mapq;
    }
    uint64_t *needed_out = nullptr;
    if (diff) {
        if (diff->struct_size < sizeof(lrm_batch_diff)) { lrm_set_error("lrm_batch_diff.struct_size %u: the struct has %zu bytes", diff->struct_size, sizeof(lrm_batch_diff)); return -1; }
        if (!diff->needed_out || (n && (!diff->off_out || !diff->cnt_out)) || (diff->cap && !diff->events_out)) { lrm_set_error("null array in lrm_batch_diff"); return -1; }
        *diff->needed_out = 0;
        j.diff_off = diff->off_out; j.diff_cnt = diff->cnt_out; j.diff_events = diff->events_out; j.diff_cap = diff->cap;
        needed_out = diff->needed_out;
    }
    return run_job(idx, j, opt, ticket_out, needed_out, piles);
}
extern "C" int lrm_map_batch_submit_ex2(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                                        lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                                        uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                                        int *meta_r_out, const lrm_map_options *opt, const lrm_batch_extras *ex,
                                        const lrm_batch_diff *diff, lrm_ticket **ticket_out) {
    return lrm_map_batch_submit_ex3(idx, reads_buf, stride, lens, n, p, gp, best_out, cig_out, store_mem, store_stride, score_out,
                                    meta_out, meta_r_out, opt, ex, diff, nullptr, ticket_out);
}
extern "C" int lrm_map_batch_submit_ex(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                                       lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                                       uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                                       int *meta_r_out, const lrm_map_options *opt, const lrm_batch_extras *ex, lrm_ticket **ticket_out) {
    return lrm_map_batch_submit_ex2(idx, reads_buf, stride, lens, n, p, gp, best_out, cig_out, store_mem, store_stride, score_out,
                                    meta_out, meta_r_out, opt, ex, nullptr, ticket_out);
}
extern "C" int lrm_map_batch_submit_mapq(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                                         lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                                         uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                                         int *meta_r_out, const lrm_map_options *opt, lrm_mapq *mapq_out, lrm_ticket **ticket_out) {
    const lrm_batch_extras ex = {(uint32_t) sizeof(lrm_batch_extras), 0, mapq_out, nullptr};
    return lrm_map_batch_submit_ex(idx, reads_buf, stride, lens, n, p, gp, best_out, cig_out, store_mem, store_stride, score_out,
                                   meta_out, meta_r_out, opt, &ex, ticket_out);
}
extern "C" int lrm_map_batch_submit(lrm_index *idx, char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                                    lrm_params p, lrm_gact_params gp, lrm_entry *best_out, lrm_cigar *cig_out,
                                    uint8_t *store_mem, uint64_t store_stride, int *score_out, lrm_seq_meta *meta_out,
                                    int *meta_r_out, const lrm_map_options *opt, lrm_ticket **ticket_out) {
    return lrm_map_batch_submit_mapq(idx, reads_buf, stride, lens, n, p, gp, best_out, cig_out, store_mem, store_stride, score_out,
                                     meta_out, meta_r_out, opt, nullptr, ticket_out);
}

// ---- the second passes over a batch that has come back (split reads, secondary alignments): a plan names the rows of a
// compact batch, the rows are gathered on the host.  What both begin with: ----
// the handle's tune under the call's options
static LrmMapTune host_tune(lrm_index *ix, const lrm_map_options *opt) { LrmMapTune mt = ix->mtune; if (opt) lrm_call_map_tune(ix, opt, &mt); return mt; }
struct HostSpan { uint32_t read, start, len; };           // row s is R[start .. start + len) of this read
// the longest of the k planned rows (span(s): row s), checked against the row stride
template <typename SpanOf>
static int host_longest_row(const char *stage, const char *row, uint64_t k, uint64_t row_stride, SpanOf span, uint32_t *longest_out) {
    uint32_t longest = 0;
    for (uint64_t s = 0; s < k; ++s) longest = span(s).len > longest ? span(s).len : longest;
    *longest_out = longest;
    if (!(row_stride & 15u) && row_stride > longest) return 0;
    lrm_set_error("%s: row_stride %llu must be a multiple of 16 above the longest %s (%u)", stage, (unsigned long long) row_stride, row, longest);
    return -1;
}
// the k rows and their lengths: row s = R[start .. start + len), zeros behind it to the end of the row (pad_row) or to the next
// multiple of 16.  turned: the caller's copy of a mapped reverse-strand read holds R's reverse complement
template <typename SpanOf>
static void host_gather_rows(const char *reads_buf, uint64_t stride, const uint32_t *lens, const lrm_seq_meta *meta, const int *meta_r,
                             bool turned, uint64_t k, SpanOf span, char *rows, uint64_t row_stride, bool pad_row, uint32_t *row_lens) {
    const int nt = lrm_host_threads();
#pragma omp parallel for schedule(dynamic, 64) num_threads(nt)
    for (uint64_t s = 0; s < k; ++s) {
        const HostSpan g = span(s);
        const char *src = reads_buf + (uint64_t) g.read * stride;
        char *dst = rows + s * row_stride;
        if (turned && meta_r[g.read] != 0 && meta[g.read].strand == 1)
            for (uint32_t x = 0; x < g.len; ++x) dst[x] = lrm_comp_table.t[(uint8_t) src[lens[g.read] - 1 - (g.start + x)]];
        else memcpy(dst, src + g.start, g.len);
        memset(dst + g.len, 0, (size_t) ((pad_row ? row_stride : ((uint64_t) g.len + 16) & ~15ull) - g.len));
        row_lens[s] = g.len;
    }
}

// ---- split reads: the second pass over a batch that came back with end clipping (docs/GACT_SPEC.md, "Split reads") ----------
static int split_batch_impl(lrm_index *idx, const char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                            const lrm_cigar *cig, const lrm_seq_meta *meta, const int *meta_r, lrm_params p, lrm_gact_params gp,
                            const lrm_map_options *opt, lrm_split_out *out) {
    const LrmMapTune mt = host_tune(idx, opt);
    if (!mt.clip || !mt.anchored) { lrm_set_error("lrm_split_batch needs lrm_map_options.clip (and with it .anchored)"); return -1; }
    uint32_t M;
    if (lrm_split_min_len(mt.split_min_len, &M)) return -1;
    if (n > 0x7fffffffull) { lrm_set_error("batch too large"); return -1; }
    // the clip counts, as the op bytes or the text of every read have them
    std::vector<lrm_clip> clip((size_t) n);
    lrm_clips_of_batch(cig, meta_r, nullptr, mt.cigar_text, n, clip.data());
    uint64_t n_seg = 0;
    const int prc = lrm_split_plan(lens, clip.data(), n, M, out->seg, out->cap, &n_seg);
    out->n_seg = n_seg;
    if (prc) return prc;
    if (n_seg == 0) return 0;
    const auto span = [&](uint64_t s) { const lrm_segment &g = out->seg[s]; return HostSpan{g.read, g.start, g.len}; };
    uint32_t longest;
    if (host_longest_row("split", "segment", n_seg, out->row_stride, span, &longest)) return -1;
    // gather on the host: R is the caller's row, or its reverse complement when the caller kept its reads as they were
    host_gather_rows(reads_buf, stride, lens, meta, meta_r, mt.keep_reads != 0, n_seg, span, out->rows, out->row_stride, false, out->lens);
    // the segment batch through the pipeline, in the caller's result layout
    lrm_map_options o2;
    lrm_map_options_init(&o2);
    if (opt) lrm_options_over_defaults(&o2, opt);
    else {
        o2.dense_results = mt.dense; o2.cigar_text = (uint32_t) mt.cigar_text; o2.gact_impl = mt.gact_impl; o2.seed_rounds = mt.seed_rounds;
        o2.anchor_min_len = mt.anchor_min_len; o2.clip_penalty = mt.clip_penalty; o2.clip_end_bonus = mt.clip_end_bonus;
        o2.copy_threads = mt.copy_threads;
    }
    o2.struct_size = (uint32_t) sizeof(o2);
    o2.anchored = 1; o2.clip = 1; o2.keep_reads = 0; o2.split = 0;
    MapJob j = {};
    j.mode = DO_SEED | DO_EXTEND; j.reads = out->rows; j.stride = out->row_stride; j.lens = out->lens; j.n = n_seg; j.p = p; j.gp = gp;
    j.best_out = out->best; j.cig = out->cig; j.store_mem = out->store; j.store_stride = out->store_stride; j.score = out->score;
    j.meta = out->meta; j.meta_r = out->meta_r; j.anchor_out = out->anchor;
    if (int rc = run_job(idx, j, &o2, nullptr)) return rc;
    lrm_clips_of_batch(out->cig, out->meta_r, out->score, mt.cigar_text, n_seg, out->clip);
    for (uint64_t s = 0; s < n_seg; ++s)
        if (out->meta_r[s] != 0 && (out->anchor[s].flags & LRM_ANCHOR_ANCHORED)) out->seg[s].flags |= LRM_SEG_ALIGNED;
    return 0;
}

extern "C" int lrm_split_batch(lrm_index *idx, const char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                               const lrm_cigar *cig, const lrm_seq_meta *meta, const int *meta_r, lrm_params p, lrm_gact_params gp,
                               const lrm_map_options *opt, lrm_split_out *out) {
    if (!idx || !out || (n && (!reads_buf || !lens || !cig || !meta || !meta_r))) { lrm_set_error("null argument"); return -1; }
    out->n_seg = 0;
    if (out->cap && (!out->seg || !out->rows || !out->lens || !out->best || !out->cig || !out->store || !out->score || !out->meta ||
                     !out->meta_r || !out->anchor || !out->clip)) { lrm_set_error("null array in lrm_split_out"); return -1; }
    try { return split_batch_impl(idx, reads_buf, stride, lens, n, cig, meta, meta_r, p, gp, opt, out); }
    catch (const std::exception &e) { lrm_set_error("host-side failure: %s", e.what()); return -1; }
}

// ---- secondary alignments: the second pass over a batch that came back with MAPQ records (docs/GACT_SPEC.md, "Secondary
// alignments").  The host pipeline is not touched: the candidates -- few reads -- go through ONE synchronous device pass on
// a workspace of their own: seed + mapping quality + rival on the candidate rows (a read's records do not depend on its
// batch, so every row is a candidate again and gets the entry it has in the primary batch), the extension `so` names,
// download, flags. ----
namespace {
struct SecWs {                                            // the pass's workspace, freed on every way out
    lrm_workspace *ws = nullptr;
    ~SecWs() { if (ws) lrm_workspace_free(ws); }
};
template <typename T>
int sec_download(T *dst, const DevBuf &src, uint64_t count) {
    HIPCHK(hipMemcpy(dst, src.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}
}  // namespace

static int secondary_batch_impl(lrm_index *idx, const char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                                const lrm_mapq *mapq, const lrm_seq_meta *meta, const int *meta_r, lrm_params p, lrm_gact_params gp,
                                const lrm_map_options *opt, const lrm_secondary_options *so, lrm_secondary_out *out) {
    lrm_index *ix = idx->peers ? idx->peers[0] : idx;     // a group handle: its first device does this pass
    const LrmMapTune mt = host_tune(ix, opt);
    lrm_secondary_options o;
    memset(&o, 0, sizeof(o));
    lrm_options_over_defaults(&o, so);
    const bool anchored = o.anchored || o.clip;
    if (out->cap && ((anchored && !out->anchor) || (o.clip && !out->clip))) { lrm_set_error("null array in lrm_secondary_out"); return -1; }
    uint64_t k = 0;
    const int prc = lrm_secondary_plan(mapq, n, o.min_hits, o.ratio_pct, out->table, out->cap, &k);
    out->n_sec = k;
    if (prc) return prc;
    if (k == 0) return 0;
    const auto span = [&](uint64_t s) { const uint32_t read = out->table[s].read; return HostSpan{read, 0u, lens[read]}; };
    uint32_t longest;
    if (host_longest_row("secondary", "candidate", k, out->row_stride, span, &longest)) return -1;
    const uint64_t need = anchored ? lrm_anchored_store_stride(longest) : 2ull * longest;
    if ((out->store_stride & 15u) || out->store_stride < need) {
        lrm_set_error("secondary: store_stride %llu must be a multiple of 16 of at least %llu", (unsigned long long) out->store_stride, (unsigned long long) need);
        return -1;
    }
    // gather on the host, as sequenced: without keep_reads the caller's copy of a reverse-strand read was reverse-complemented
    host_gather_rows(reads_buf, stride, lens, meta, meta_r, !mt.keep_reads && meta, k, span, out->rows, out->row_stride, true, out->lens);
    // the device pass
    if (lrm_require_device(ix->device)) return -1;
    SecWs w;
    if (lrm_workspace_create(&w.ws, ix, k, longest, p.seed_len, p.thres)) return -1;
    DevBuf d_rows, d_lens, d_best, d_mapq, d_rival, d_store, d_n_ops, d_score, d_meta, d_meta_r, d_anchor, d_clip;
    if (d_rows.alloc(k * out->row_stride) || d_lens.alloc(k * 4) || d_best.alloc(k * sizeof(lrm_entry)) || d_mapq.alloc(k * sizeof(lrm_mapq)) ||
        d_rival.alloc(k * sizeof(lrm_entry)) || d_store.alloc(k * out->store_stride) || d_n_ops.alloc(k * 4) || d_score.alloc(k * 4) ||
        d_meta.alloc(k * sizeof(lrm_seq_meta)) || d_meta_r.alloc(k * 4) || d_anchor.alloc(k * sizeof(lrm_anchor)) || d_clip.alloc(k * sizeof(lrm_clip))) {
        (void) hipGetLastError();
        lrm_set_error("secondary: device allocation for %llu candidates failed", (unsigned long long) k);
        return -1;
    }
    HIPCHK(hipMemcpy(d_rows.p, out->rows, k * out->row_stride, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_lens.p, out->lens, k * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_meta.p, 0, k * sizeof(lrm_seq_meta)));          // (the padding bytes of the records come down too)
    HIPCHK(hipMemset(d_anchor.p, 0, k * sizeof(lrm_anchor)));
    HIPCHK(hipMemset(d_clip.p, 0, k * sizeof(lrm_clip)));
    uint8_t *d_phase = lrm_mapq_phase_buf(w.ws);
    if (!d_phase) return -1;
    const uint32_t *dl = (const uint32_t *) d_lens.p;
    if (int rc = lrm_launch_seed(ix, w.ws, (const char *) d_rows.p, out->row_stride, dl, k, p.seed_len, p.thres, (lrm_entry *) d_best.p, mt, nullptr, d_phase)) return rc;
    if (int rc = lrm_launch_mapq(ix, w.ws, dl, k, p.seed_len, p.thres, (const lrm_entry *) d_best.p, (lrm_mapq *) d_mapq.p, nullptr)) return rc;
    if (int rc = lrm_launch_rival(ix, w.ws, dl, k, p.seed_len, (const lrm_entry *) d_best.p, (const lrm_mapq *) d_mapq.p, o.min_hits, o.ratio_pct,
                                  (lrm_entry *) d_rival.p, nullptr)) return rc;
    const LrmExtendBatch b = {(char *) d_rows.p, out->row_stride, dl, k, longest, (const lrm_entry *) d_rival.p, (uint8_t *) d_store.p,
                              out->store_stride, (int32_t *) d_n_ops.p, (int32_t *) d_score.p, (lrm_seq_meta *) d_meta.p, (int32_t *) d_meta_r.p};
    if (anchored) {
        const LrmClipOpt clip = o.clip ? LrmClipOpt{1, o.clip_penalty, o.clip_end_bonus, (lrm_clip *) d_clip.p} : LrmClipOpt{};
        if (int rc = lrm_launch_extend_anchored(ix, w.ws, b, gp, (lrm_anchor *) d_anchor.p, o.anchor_min_len, clip, mt, nullptr)) return rc;
    } else if (int rc = lrm_launch_extend(ix, w.ws, b, gp, mt, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    if (lrm_ws_take_error(w.ws)) return -2;
    // download: the rows as the extension left them, the small arrays, the op bytes in the layout opt names
    std::vector<int32_t> n_ops((size_t) k);
    std::vector<uint8_t> ops((size_t) (k * out->store_stride));
    HIPCHK(hipMemcpy(out->rows, d_rows.p, k * out->row_stride, hipMemcpyDeviceToHost));
    if (sec_download(out->rival, d_rival, k) || sec_download(n_ops.data(), d_n_ops, k) || sec_download(out->score, d_score, k) ||
        sec_download(out->meta, d_meta, k) || sec_download(out->meta_r, d_meta_r, k) || sec_download(ops.data(), d_store, k * out->store_stride)) return -1;
    if (anchored && sec_download(out->anchor, d_anchor, k)) return -1;
    if (o.clip && sec_download(out->clip, d_clip, k)) return -1;
    const uint64_t room = out->cap * out->store_stride;
    uint64_t at = 0;                                      // dense layouts: where the next alignment goes
    for (uint64_t s = 0; s < k; ++s) {
        const bool aligned = out->meta_r[s] != 0 && out->score[s] != -1;
        const uint8_t *src = ops.data() + s * out->store_stride;
        lrm_cigar &c = out->cig[s];
        c.n_cigar_op = n_ops[s]; c.score = out->score[s];
        if (mt.cigar_text) {                              // the run-length text parse_cigar prints, NUL-terminated, 16-byte units
            const int len = lrm_parse_cigar(src, aligned ? n_ops[s] : 0, (char *) out->store + at, (int) (room - at < 0x7fffffffull ? room - at : 0x7fffffffull));
            if (len < 0) { lrm_set_error("secondary: the store has no room for the CIGAR text of candidate %llu", (unsigned long long) s); return -1; }
            c.cigar = out->store + at;
            at += ((uint64_t) len + 1 + 15) & ~15ull;
        } else {
            const uint64_t bytes = n_ops[s] > 0 ? (uint64_t) n_ops[s] : 0;
            c.cigar = out->store + (mt.dense ? at : s * out->store_stride);
            memcpy(c.cigar, src, bytes);
            if (mt.dense) at += (bytes + 15) & ~15ull;
        }
        out->table[s].hits = (uint32_t) out->rival[s].val;
        const uint32_t read = out->table[s].read;
        const lrm_seq_meta none = {0, 0, -1, 0};
        out->table[s].flags = lrm_sec_flags(meta != nullptr, meta ? meta_r[read] : 0, meta ? meta[read] : none, out->meta_r[s], out->meta[s],
                                            out->score[s], out->lens[s], anchored, anchored ? out->anchor[s].flags : 0u);
    }
    return 0;
}

extern "C" int lrm_secondary_batch(lrm_index *idx, const char *reads_buf, uint64_t stride, const uint32_t *lens, uint64_t n,
                                   const lrm_mapq *mapq, const lrm_seq_meta *meta, const int *meta_r, lrm_params p, lrm_gact_params gp,
                                   const lrm_map_options *opt, const lrm_secondary_options *so, lrm_secondary_out *out) {
    if (!idx || !out || (n && (!reads_buf || !lens || !mapq))) { lrm_set_error("null argument"); return -1; }
    out->n_sec = 0;
    if ((meta == nullptr) != (meta_r == nullptr)) { lrm_set_error("secondary: meta and meta_r come together"); return -1; }
    if (out->cap && (!out->table || !out->rows || !out->lens || !out->rival || !out->cig || !out->store || !out->score || !out->meta ||
                     !out->meta_r)) { lrm_set_error("null array in lrm_secondary_out"); return -1; }
    if (n > 0x7fffffffull) { lrm_set_error("batch too large"); return -1; }
    try { return secondary_batch_impl(idx, reads_buf, stride, lens, n, mapq, meta, meta_r, p, gp, opt, so, out); }
    catch (const std::exception &e) { lrm_set_error("host-side failure: %s", e.what()); return -1; }
}

extern "C" int lrm_map_batch_wait(lrm_ticket *ticket) {
    if (!ticket) { lrm_set_error("null ticket"); return -1; }
    try { return wait_impl(ticket); }
    catch (...) { lrm_set_error("host-side failure"); return -1; }
}

// Pinned host memory for the caller's batch buffers (reads_buf, store_mem): the DMA engines read and write it
// directly, no staging copy.  lrm_host_register pins memory the caller already owns (malloc'd at alnmain.c:297-320).
extern "C" void *lrm_host_alloc(uint64_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void) hipGetLastError(); lrm_set_error("hipHostMalloc of %llu bytes failed", (unsigned long long) bytes); return nullptr; }
    return p;
}
extern "C" void lrm_host_free(void *p) { if (p) (void) hipHostFree(p); }
extern "C" int lrm_host_register(void *p, uint64_t bytes) {
    if (!p || !bytes) { lrm_set_error("bad argument"); return -1; }
    HIPCHK(hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped));
    return 0;
}
extern "C" int lrm_host_unregister(void *p) {
    if (!p) return 0;
    HIPCHK(hipHostUnregister(p));
    return 0;
}
