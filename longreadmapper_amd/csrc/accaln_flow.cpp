// accaln_flow.cpp -- `accaln genome reads` on the GPU path (lrm_accaln, lrm_accaln_opt, lrm_accaln_mapq, lrm_accaln_md, lrm_accaln_paf,
// include/lrm_io_host.h): single_end() (alnmain.c:277-551) as a pipeline of threads around the asynchronous batch calls.
// Host-side C++; the kernels are reached only through the C-ABI.
//
// A loader thread parses batch k+2 (parallel FASTQ parser, sequences straight into a pinned buffer), the calling thread
// keeps two batches in flight on the device (lrm_map_batch_submit / _wait, dense results DMA'd into pinned memory), a
// formatter thread turns batch k-1 into SAM text in parallel and a flusher thread writes the parts of the text before
// it with parallel pwrites.  Four sets of buffers go round.  The reference does the stages one after the other; at
// device mapping rates the text stages are the whole run time, so they have to overlap AND be parallel.  Output is
// identical: batches are written in input order.
#include <hip/hip_runtime_api.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/lrm_index_host.h"
#include "sam_text.h"
#include "paf_text.h"
#include "lrm_internal.h"
#include "extend_stage.h"

namespace {

// bounded hand-off between two stages of the pipeline
template <typename T>
struct StageQueue {
    std::mutex m;
    std::condition_variable cv;
    std::deque<T> q;
    size_t cap;
    bool closed = false;
    explicit StageQueue(size_t c) : cap(c) {}
    bool push(T v) {                                     // false: the queue was closed by the consumer (an error downstream)
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return q.size() < cap || closed; });
        if (closed) return false;
        q.push_back(std::move(v));
        cv.notify_all();
        return true;
    }
    bool pop(T &v) {                                     // false: closed and drained
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return !q.empty() || closed; });
        if (q.empty()) return false;
        v = std::move(q.front());
        q.pop_front();
        cv.notify_all();
        return true;
    }
    void close() { std::lock_guard<std::mutex> lk(m); closed = true; cv.notify_all(); }
};

// what a second pass writes for one batch (lrm_split_batch, lrm_secondary_batch): pageable buffers grown on demand, and the
// table that points at them.  The two out structs differ in their record (TABLE) and in the name of their entries (ENTRY)
template <typename Out, typename Rec, Rec *Out::*TABLE, lrm_entry *Out::*ENTRY>
struct PassBufs {
    Out out;
    std::vector<Rec> table;
    std::vector<char> rows;
    std::vector<uint8_t> store;
    std::vector<uint32_t> lens;
    std::vector<lrm_entry> entry;
    std::vector<lrm_cigar> cig;
    std::vector<int> score, meta_r;
    std::vector<lrm_seq_meta> meta;
    std::vector<lrm_anchor> anchor;
    std::vector<lrm_clip> clip;
    PassBufs() { memset(&out, 0, sizeof(out)); }
    // an empty table for k == 0, else room for k rows with rows and op bytes at these strides
    Out *fit(uint64_t k, uint64_t row_stride, uint64_t store_stride) {
        memset(&out, 0, sizeof(out));
        if (k == 0) return &out;
        auto room = [](auto &v, uint64_t n) { v.resize((size_t) n); return v.data(); };
        out.cap = k; out.row_stride = row_stride; out.store_stride = store_stride;
        out.*TABLE = room(table, k); out.rows = room(rows, k * row_stride); out.store = room(store, k * store_stride);
        out.lens = room(lens, k); out.*ENTRY = room(entry, k); out.cig = room(cig, k); out.score = room(score, k);
        out.meta_r = room(meta_r, k); out.meta = room(meta, k); out.anchor = room(anchor, k); out.clip = room(clip, k);
        return &out;
    }
};
using SplitBufs = PassBufs<lrm_split_out, lrm_segment, &lrm_split_out::seg, &lrm_split_out::best>;
using SecBufs = PassBufs<lrm_secondary_out, lrm_secondary, &lrm_secondary_out::table, &lrm_secondary_out::rival>;   // (docs/GACT_SPEC.md, "Secondary alignments")

// one batch on its way through the pipeline, with the caller-side buffers of the hot path (pinned: the DMA engines
// read the reads and write the dense op bytes straight from / into them); recycled.  A set belongs to the thread that
// popped it from a queue, until that thread pushes it on.
struct BatchSet {
    lrm_read_batch b;
    char *reads_pin = nullptr; uint64_t reads_cap = 0;           // written by the pinner, read by the others once pin_ready is set
    uint8_t *store_pin = nullptr; uint64_t store_cap = 0;
    std::atomic<bool> pin_ready{false};          // the pinner thread has given this set its pinned buffers
    uint8_t *store_pg = nullptr; uint64_t store_pg_cap = 0;      // pageable stand-in until then (or when a batch outgrows the pinned one)
    uint8_t *store = nullptr;
    std::vector<lrm_entry> best;
    std::vector<lrm_cigar> cig;
    std::vector<int> score, meta_r;
    std::vector<lrm_seq_meta> meta;
    uint64_t sstride = 0;
    lrm_ticket *ticket = nullptr;
    SecBufs sc;                                  // secondary alignments: the second pass over this batch's candidates (lrm_secondary_batch)
    SplitBufs sp;                                // split reads: the second pass over this batch's clipped ends (lrm_split_batch)
    std::vector<lrm_mapq> mq;                    // lrm_accaln_mapq: the records of the batch
    std::vector<lrm_aln_summary> sum;            // lrm_accaln_paf, lrm_accaln_md: the alignment summary records of the batch
    // lrm_accaln_md: the difference events of the batch.  The buffer has room for the bound (a read has no more events than
    // columns) and is never cleared: the pages the events do not reach are never touched
    std::vector<uint64_t> diff_off;
    std::vector<uint32_t> diff_cnt;
    uint32_t *events = nullptr; uint64_t events_cap = 0, events_needed = 0;
    BatchSet() { memset(&b, 0, sizeof(b)); }
    ~BatchSet() { lrm_host_free(reads_pin); lrm_host_free(store_pin); free(store_pg); free(events); }
};

struct TextBatch { std::vector<std::string> parts; };   // the SAM text of one batch, one part per formatting thread

struct StageError {                                      // lrm_last_error() is thread-local: stages report through this
    std::mutex m;
    int rc = 0;
    std::string msg;
    void set(int code) {
        std::lock_guard<std::mutex> lk(m);
        if (!rc) { rc = code; msg = lrm_last_error(); }
    }
    int get() { std::lock_guard<std::mutex> lk(m); return rc; }
};

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One run of the flow.  The fields are what the threads share; next to each: which thread writes it while they run
// ("main" is the caller's thread, which submits and waits).  The member functions are the stages.
struct AccalnRun {
    static constexpr int NSETS = 4;                      // loading, two on the device, formatting
    // ---- written by main before the threads start, only read from then on ----
    const lrm_params p;
    const lrm_gact_params gp;
    int device;
    const bool mapq;                                     // the mapping-quality records come back with every batch and are printed
    const bool paf;                                      // PAF instead of SAM: the summary records come back too, no header
    const bool md;                                       // NM:i and MD:Z: the summary records and the difference events come back and are printed
    const bool verbose = getenv("LRM_HOST_VERBOSE") != nullptr;            // stage times on stderr (tuning aid)
    lrm_map_options mopt;
    bool split = false;                                  // after a batch's wait its clipped ends go through lrm_split_batch
    bool sec = false;                                    // ... and its candidates through lrm_secondary_batch (needs mapq)
    lrm_secondary_options so;
    // lrm_accaln_pileup: every batch adds to one accumulator over [pile_lo, pile_hi), created behind the upload; sam_path may
    // then be null -- the reads are mapped and downloaded, nothing is formatted or written
    bool pile_on = false;
    lrm_accaln_pileup_options po;
    lrm_pileup *acc = nullptr;
    uint64_t pile_lo = 0, pile_hi = 0;
    bool vcf_on = false;                                 // lrm_accaln_pileup_vcf: the variant records of the same accumulator as VCF
    lrm_accaln_vcf_options vo;
    bool want_pinned = false;
    lrm_host_index hi;
    lrm_index *gpu = nullptr;
    lrm_reader *rd = nullptr;                            // (the loader is its only user)
    int out_fd = -1;
    const char *sam_path = nullptr;
    const uint64_t bs;
    const int io_threads = lrm_host_threads() > 2 ? lrm_host_threads() / 2 : 1;     // loader and formatter share the host
    double t_begin = now(), t_read_idx = 0, t_upload = 0;
    std::vector<std::unique_ptr<BatchSet>> sets;
    // ---- the hand-offs (their own locks) ----
    StageQueue<BatchSet *> free_sets{NSETS}, loaded{NSETS}, mapped{NSETS};  // to the loader, loader -> main, main -> formatter
    StageQueue<std::unique_ptr<TextBatch>> texts{2}, free_texts{3};         // formatter -> flusher, and back
    StageError err;                                      // any stage; the first error stays
    // ---- the size of the pinned buffers, under dims_m ----
    std::mutex dims_m;
    std::condition_variable dims_cv;
    uint64_t dim_reads = 0, dim_store = 0;               // loader (once, from the first batch); the pinner reads them
    bool dims_known = false;                             // loader
    bool first_submitted = false, dims_stop = false;     // main
    // ---- each stage's own ----
    double t_load = 0;                                   // loader
    double t_map = 0;                                    // main
    std::deque<BatchSet *> inflight;                     // main: submitted and not yet waited for, oldest first
    double t_fmt = 0;                                    // formatter
    uint64_t total = 0, valid = 0;                       // formatter
    double t_write = 0;                                  // flusher
    uint64_t out_off = 0;                                // flusher (main sets it behind the header before the threads start)

    AccalnRun(lrm_params p_, lrm_gact_params gp_, int device_, bool mapq_, bool paf_ = false, bool md_ = false)
        : p(p_), gp(gp_), device(device_), mapq(mapq_), paf(paf_), md(md_), bs(p_.batch_size ? p_.batch_size : 1000) {}

    // op bytes per read: alnmain.c:316-320, a multiple of 16; the anchored mode's targets are an eighth longer than the reads
    uint64_t store_stride_of(uint64_t max_len) const {
        const uint64_t s = ((mopt.anchored ? lrm_anchored_store_stride((uint32_t) max_len) : 2 * max_len) + 15) & ~15ull;
        return s > 0 ? s : (uint64_t) 16;
    }
    void recycle(BatchSet *s) { lrm_read_batch_free(&s->b); free_sets.push(s); }

    // user: only the fields that change WHAT is computed are taken (anchored, anchor_min_len, clip, clip_penalty,
    // clip_end_bonus, split, split_min_len); the shape of the pipeline is this flow's own choice
    int take_options(const lrm_map_options *user) {
        // The fields came in three groups, and a group counts only if the caller's struct holds all of it (a caller built
        // before the clip fields existed has them inside its zeroed reserved words or not at all).  struct_size == 0
        // means "take nothing" here -- not "take everything" as in lrm_options_over_defaults.
        lrm_map_options u;
        memset(&u, 0, sizeof(u));
        lrm_options_take_fields(&u, user, offsetof(lrm_map_options, anchored), offsetof(lrm_map_options, clip));
        lrm_options_take_fields(&u, user, offsetof(lrm_map_options, clip), offsetof(lrm_map_options, split));
        lrm_options_take_fields(&u, user, offsetof(lrm_map_options, split), offsetof(lrm_map_options, split_min_len) + sizeof(uint32_t));
        if (u.split && paf) { lrm_set_error("PAF output of split reads is not there yet: the segments have no alignment summary records (lrm_split_out is fixed-size)"); return -1; }
        if (u.split && !u.clip) { lrm_set_error("lrm_map_options.split needs lrm_map_options.clip"); return -1; }
        lrm_map_options_init(&mopt);
        mopt.cigar_text = 1;                        // parse_cigar (alnmain.c:497-498) runs on the device: the SAM CIGAR text comes back
        mopt.copy_threads = 2;                      // the parser and the formatter need the cores
        mopt.keep_reads = 1;                        // reverse-strand reads are reverse-complemented by the formatter as it copies them
        if (u.anchored) { mopt.anchored = 1; mopt.anchor_min_len = u.anchor_min_len; }
        if (u.clip) { mopt.clip = 1; mopt.clip_penalty = u.clip_penalty; mopt.clip_end_bonus = u.clip_end_bonus; }
        split = u.clip && u.split;
        if (split) { mopt.split = 1; mopt.split_min_len = u.split_min_len; }
        return 0;
    }

    // init() (alnmain.c:179-256) behind the index files: the device image, the SAM file with its header, the reader
    int begin(const char *reads_path, const char *sam, long rg_id) {
        t_read_idx = now();
        sam_path = sam;
        struct stat st;
        const bool sized = stat(reads_path, &st) == 0;            // (a file that cannot be sized is under neither rule)
        lrm_index_options iopt;
        lrm_index_options_init(&iopt);
        // a reads file below 64 GiB (some tens of Gbp) does not repay the 0.7-2 s the 64 GiB seed table costs at upload
        if (sized && (uint64_t) st.st_size < (64ull << 30)) iopt.lc_long_max = 15;
        // Pinning the batch buffers (0.2 s per GB to pin and to release, and the device stalls while the runtime pins)
        // pays from a few tens of Gbp on: reads files below 16 GiB run through pageable buffers.
        want_pinned = sized && (uint64_t) st.st_size >= (16ull << 30);
        int rc = lrm_index_upload_opt(&gpu, &hi.fmi, &hi.lch, &hi.sa, hi.content, hi.con_len, hi.mta, hi.mta_len, &device, 1, &iopt);
        t_upload = now();
        if (rc) return rc;
        if (pile_on && lrm_pileup_create_ins(&acc, gpu, pile_lo, pile_hi, po.ins_cols)) return -1;
        if (!sam_path) return lrm_reader_open(&rd, reads_path);       // (lrm_accaln_pileup alone)
        out_fd = open(sam_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (out_fd < 0) { lrm_set_error("cannot create: %s", sam_path); return -1; }
        if (!paf) {                                                   // (PAF has no header)
            uint64_t hl = 0;
            char *h = lrm_sam_header(hi.mta, hi.mta_len, rg_id, &hl);
            if (pwrite(out_fd, h, hl, 0) != (ssize_t) hl) { lrm_set_error("cannot write: %s", sam_path); rc = -1; }
            out_off = hl;
            free(h);
        }
        return rc ? rc : lrm_reader_open(&rd, reads_path);
    }

    // Pinning memory costs ~0.2 s per GB: a thread of its own sizes the sets' pinned buffers from the first batch
    // (+ 1/8) while the first batches already run through pageable memory (staged upload, staged dense download).
    void pinner() {
        if (hipSetDevice(device) != hipSuccess) { (void) hipGetLastError(); }
        {
            std::unique_lock<std::mutex> lk(dims_m);
            // (after the first submit: that call builds the handle's host context -- streams, staging, mirrors -- and
            //  would queue behind the runtime's lock while gigabytes are being pinned here)
            dims_cv.wait(lk, [&] { return (dims_known && first_submitted) || dims_stop; });
            if (!dims_known || dims_stop || !want_pinned) return;
        }
        for (auto &sp : sets) {
            { std::lock_guard<std::mutex> lk(dims_m); if (dims_stop) return; }
            BatchSet *s = sp.get();
            s->reads_pin = (char *) lrm_host_alloc(dim_reads);
            s->store_pin = (uint8_t *) lrm_host_alloc(dim_store);
            if (!s->reads_pin || !s->store_pin) { lrm_host_free(s->reads_pin); lrm_host_free(s->store_pin); s->reads_pin = nullptr; s->store_pin = nullptr; return; }
            s->reads_cap = dim_reads; s->store_cap = dim_store;
            s->pin_ready.store(true, std::memory_order_release);
            if (verbose) fprintf(stderr, "[lrm accaln] %.3f pinned a set (%.2f + %.2f GB)\n", now() - t_upload, dim_reads / 1e9, dim_store / 1e9);
        }
    }

    void loader() {                                                           // alnmain.c:302
        BatchSet *s = nullptr;
        while (!err.get() && free_sets.pop(s)) {
            const double t0 = now();
            const bool pinned = s->pin_ready.load(std::memory_order_acquire);
            int64_t n = lrm_reader_next_into(rd, bs, &s->b, pinned ? s->reads_pin : nullptr, pinned ? s->reads_cap : 0);
            t_load += now() - t0;
            if (verbose) fprintf(stderr, "[lrm accaln] %.3f loaded %lld reads in %.3f s (%s)\n", now() - t_upload, (long long) n, now() - t0, pinned ? "pinned" : "pageable");
            if (n < 0) { err.set(-1); break; }
            if (n == 0) { recycle(s); break; }
            if (!dims_known) {
                std::lock_guard<std::mutex> lk(dims_m);
                const uint64_t rb = s->b.n * s->b.stride, sb = s->b.n * (store_stride_of(s->b.max_len) + 16);
                dim_reads = rb + rb / 8 + 4096; dim_store = sb + sb / 8 + 4096;
                dims_known = true;
                dims_cv.notify_all();
            }
            if (!loaded.push(s)) break;
        }
        loaded.close();
    }

    // PART 3, alnmain.c:458-527, in two stages: the formatter turns a mapped batch into SAM text (one part per thread)
    // and gives the set back; the flusher writes the parts of the previous batch with parallel pwrites meanwhile.
    void formatter() {
        BatchSet *s = nullptr;
        while (mapped.pop(s)) {
            std::unique_ptr<TextBatch> tb;
            if (!sam_path) {                                          // no text asked for: the counters alone
                const uint64_t n = s->b.n;
                total += n;
                for (uint64_t i = 0; i < n; ++i) valid += (s->score[i] >= 0 && s->meta_r[i] != 0) ? 1 : 0;
            } else if (!err.get() && free_texts.pop(tb)) {
                const uint64_t n = s->b.n;
                const double t0 = now();
                if (paf) {
                    const PafBatch pb = {&s->b, hi.mta, hi.mta_len, s->cig.data(), s->score.data(), s->meta.data(), s->meta_r.data(), n,
                                         /* cigar_is_text */ true, s->sum.data(), mapq ? s->mq.data() : nullptr};
                    paf_format_parts(pb, io_threads, tb->parts);
                } else {
                    const SamBatch sb = {&s->b, hi.mta, hi.mta_len, s->cig.data(), s->score.data(), s->meta.data(), s->meta_r.data(), n,
                                         /* cigar_is_text */ true, /* revcomp_here */ true, split ? &s->sp.out : nullptr, mapq ? s->mq.data() : nullptr,
                                         md ? s->sum.data() : nullptr, md ? s->diff_off.data() : nullptr, md ? s->diff_cnt.data() : nullptr, md ? s->events : nullptr,
                                         sec ? &s->sc.out : nullptr};
                    sam_format_parts(sb, io_threads, tb->parts);
                }
                t_fmt += now() - t0;
                if (verbose) fprintf(stderr, "[lrm accaln] %.3f formatted %llu reads in %.3f s\n", now() - t_upload, (unsigned long long) n, now() - t0);
                total += n;
                for (uint64_t i = 0; i < n; ++i) valid += (s->score[i] >= 0 && s->meta_r[i] != 0) ? 1 : 0;   // alnmain.c:464-469,489-491
                if (!texts.push(std::move(tb))) err.set(-1);
            }
            recycle(s);
        }
        texts.close();
    }

    void flusher() {
        std::unique_ptr<TextBatch> tb;
        while (texts.pop(tb)) {
            if (!err.get()) {
                const double t1 = now();
                const std::vector<std::string> &parts = tb->parts;
                const std::vector<uint64_t> at = sam_part_offsets(parts, out_off);
                bool ok = true;
#pragma omp parallel for schedule(static, 1) num_threads((int) parts.size()) reduction(&& : ok)
                for (size_t k = 0; k < parts.size(); ++k) {
                    size_t done = 0;
                    while (done < parts[k].size()) {
                        const ssize_t w = pwrite(out_fd, parts[k].data() + done, parts[k].size() - done, (off_t) (at[k] + done));
                        if (w <= 0) { ok = false; break; }
                        done += (size_t) w;
                    }
                }
                out_off = at[parts.size()];
                if (!ok) { lrm_set_error("cannot write: %s", sam_path); err.set(-1); }
                t_write += now() - t1;
                if (verbose) fprintf(stderr, "[lrm accaln] %.3f wrote %.2f GB in %.3f s\n", now() - t_upload, (at[parts.size()] - at[0]) / 1e9, now() - t1);
            }
            if (!free_texts.push(std::move(tb))) break;
        }
        free_texts.close();
    }

    // the second pass over a batch that has come back: size the segment buffers from the plan, then lrm_split_batch
    int split_pass(BatchSet *s) {
        const uint64_t n = s->b.n;
        std::vector<lrm_clip> cl((size_t) n);
        lrm_clips_of_batch(s->cig.data(), s->meta_r.data(), s->score.data(), 1, n, cl.data());
        uint32_t longest = 0;
        for (uint64_t i = 0; i < n; ++i) longest = std::max(longest, std::max(cl[i].left, cl[i].right));
        uint64_t k = 0;
        if (lrm_split_plan(s->b.lens, cl.data(), n, mopt.split_min_len, nullptr, 0, &k) == -1) return -1;
        lrm_split_out *o = s->sp.fit(k, ((uint64_t) longest + 16) & ~15ull, store_stride_of(longest));
        if (k == 0) return 0;
        return lrm_split_batch(gpu, s->b.seqs, s->b.stride, s->b.lens, n, s->cig.data(), s->meta.data(), s->meta_r.data(), p, gp, &mopt, o);
    }

    // ... and over its candidates: size the buffers from the plan, then lrm_secondary_batch
    int secondary_pass(BatchSet *s) {
        const uint64_t n = s->b.n;
        uint64_t k = 0;
        if (lrm_secondary_plan(s->mq.data(), n, so.min_hits, so.ratio_pct, nullptr, 0, &k) == -1) return -1;
        const uint64_t L = s->b.max_len;
        const uint64_t need = (so.anchored || so.clip) ? lrm_anchored_store_stride((uint32_t) L) : 2 * L;
        lrm_secondary_out *o = s->sc.fit(k, (L + 16) & ~15ull, ((need + 15) & ~15ull) + 16);
        if (k == 0) return 0;
        return lrm_secondary_batch(gpu, s->b.seqs, s->b.stride, s->b.lens, n, s->mq.data(), s->meta.data(), s->meta_r.data(), p, gp, &mopt, &so, o);
    }

    void finish_oldest() {
        BatchSet *s = inflight.front();
        inflight.pop_front();
        const double t0 = now();
        int mrc = lrm_map_batch_wait(s->ticket);
        if (!mrc && md && s->events_needed > s->events_cap) {
            lrm_set_error("difference events: a batch needs %llu, more than the bound of %llu", (unsigned long long) s->events_needed, (unsigned long long) s->events_cap);
            mrc = -1;
        }
        if (!mrc && split) mrc = split_pass(s);
        if (!mrc && sec) mrc = secondary_pass(s);
        t_map += now() - t0;
        if (verbose) fprintf(stderr, "[lrm accaln] %.3f waited %.3f s for a batch of %llu\n", now() - t_upload, now() - t0, (unsigned long long) s->b.n);
        s->ticket = nullptr;
        if (mrc) { err.set(-1); recycle(s); return; }
        (void) mapped.push(s);                                                // (only this thread closes `mapped`, behind the last batch)
    }

    // the result buffers of the batch in s: the pinned store if it is there and large enough, else a pageable one
    bool fit_results(BatchSet *s) {
        const size_t n = (size_t) s->b.n;
        s->best.resize(n); s->cig.resize(n); s->score.resize(n); s->meta_r.resize(n); s->meta.resize(n);
        if (mapq) s->mq.resize(n);
        if (paf || md) s->sum.resize(n);
        s->sstride = store_stride_of(s->b.max_len);
        if (md) {
            s->diff_off.resize(n); s->diff_cnt.resize(n);
            if (n * s->sstride > s->events_cap) {
                free(s->events);
                s->events_cap = n * s->sstride;
                s->events = (uint32_t *) malloc((size_t) s->events_cap * sizeof(uint32_t));
                if (!s->events) { s->events_cap = 0; lrm_set_error("out of memory"); return false; }
            }
        }
        if (s->pin_ready.load(std::memory_order_acquire) && n * s->sstride <= s->store_cap) { s->store = s->store_pin; return true; }
        if (n * s->sstride > s->store_pg_cap) {
            free(s->store_pg);
            s->store_pg_cap = n * s->sstride;
            s->store_pg = (uint8_t *) malloc(s->store_pg_cap ? s->store_pg_cap : 1);
            if (!s->store_pg) { s->store_pg_cap = 0; lrm_set_error("out of memory"); return false; }
        }
        s->store = s->store_pg;
        return true;
    }

    // PART 1 + PART 2 in one device pass, asynchronously: two batches on the device, one queued behind them
    void submit_loop() {
        BatchSet *s = nullptr;
        while (loaded.pop(s)) {
            if (err.get()) { recycle(s); continue; }                          // drain what the loader already parsed
            if (!fit_results(s)) { err.set(-1); recycle(s); continue; }
            const double t0 = now();
            const lrm_batch_extras ex = {(uint32_t) sizeof(lrm_batch_extras), 0, mapq ? s->mq.data() : nullptr, paf || md ? s->sum.data() : nullptr};
            const lrm_batch_diff df = {(uint32_t) sizeof(lrm_batch_diff), 0, s->diff_off.data(), s->diff_cnt.data(), s->events, s->events_cap, &s->events_needed};
            const lrm_batch_pileup bp = {(uint32_t) sizeof(lrm_batch_pileup), po.min_mapq, &acc, 1u, 0u};
            const int src = lrm_map_batch_submit_ex3(gpu, s->b.seqs, s->b.stride, s->b.lens, s->b.n, p, gp, s->best.data(), s->cig.data(),
                                                    s->store, s->sstride, s->score.data(), s->meta.data(), s->meta_r.data(), &mopt,
                                                    &ex, md ? &df : nullptr, acc ? &bp : nullptr, &s->ticket);
            t_map += now() - t0;
            if (verbose) fprintf(stderr, "[lrm accaln] %.3f submitted %llu reads (%s store) in %.3f s\n", now() - t_upload, (unsigned long long) s->b.n, s->store == s->store_pin ? "pinned" : "pageable", now() - t0);
            if (!first_submitted) { { std::lock_guard<std::mutex> lk(dims_m); first_submitted = true; } dims_cv.notify_all(); }
            if (src) { err.set(-1); recycle(s); continue; }
            inflight.push_back(s);
            if (inflight.size() >= 3) finish_oldest();
        }
        while (!inflight.empty()) finish_oldest();
    }

    // ---- lrm_accaln_pileup: the sites table and the polished sequences of the selected sequences, behind the last wait ----
    struct DevMem {                                                           // device memory of the read side, freed on every way out
        void *p = nullptr;
        ~DevMem() { if (p) (void) hipFree(p); }
        int room(uint64_t bytes) {
            if (p) (void) hipFree(p);
            p = nullptr;
            if (hipMalloc(&p, bytes ? bytes : 1) == hipSuccess) return 0;
            (void) hipGetLastError();
            p = nullptr;
            lrm_set_error("pileup output: device allocation of %llu bytes failed", (unsigned long long) bytes);
            return -1;
        }
    };
    static int down(void *dst, const void *src, uint64_t bytes) {
        if (bytes && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) { (void) hipGetLastError(); lrm_set_error("pileup output: download failed"); return -1; }
        return 0;
    }
    // the sites of window positions [first, first + count) as text lines; a table that did not fit is asked for again with
    // the reported total (the counters do not move)
    int write_sites_of(FILE *f, uint64_t first, uint64_t count) {
        DevMem d_sites, d_n, d_al;
        uint64_t cap = std::min<uint64_t>(count, 4096 + count / 256), n_sites = 0;
        if (d_n.room(8)) return -1;
        for (;;) {
            if (d_sites.room(cap * sizeof(lrm_pileup_site))) return -1;
            if (lrm_pileup_sites_dev(acc, &po.call, first, count, (lrm_pileup_site *) d_sites.p, cap, (uint64_t *) d_n.p, nullptr, nullptr)) return -1;
            if (down(&n_sites, d_n.p, 8)) return -1;
            if (n_sites <= cap) break;
            cap = n_sites;
        }
        std::vector<lrm_pileup_site> sites((size_t) n_sites);
        std::vector<lrm_pileup_ins_allele> al;
        if (down(sites.data(), d_sites.p, n_sites * sizeof(lrm_pileup_site))) return -1;
        if (po.ins_cols && n_sites) {
            al.resize((size_t) n_sites);
            if (d_al.room(n_sites * sizeof(lrm_pileup_ins_allele))) return -1;
            if (lrm_pileup_site_alleles_dev(acc, &po.call, (const lrm_pileup_site *) d_sites.p, n_sites, (lrm_pileup_ins_allele *) d_al.p, nullptr)) return -1;
            if (down(al.data(), d_al.p, n_sites * sizeof(lrm_pileup_ins_allele))) return -1;
        }
        uint64_t longest = 0;
        for (int k = 0; k < hi.mta_len; ++k) longest = std::max<uint64_t>(longest, hi.mta[k].name ? hi.mta[k].name_len : 0);
        const uint64_t chunk = 1u << 16;
        std::vector<char> text((size_t) ((longest + 128) * std::min(chunk, n_sites) + 1));
        for (uint64_t at = 0; at < n_sites; at += chunk) {
            const uint64_t k = std::min(chunk, n_sites - at);
            const int64_t len = lrm_pileup_sites_format_ins(hi.mta, hi.mta_len, sites.data() + at, po.ins_cols ? al.data() + at : nullptr, k, text.data(), (int64_t) text.size());
            if (len < 0) return -1;
            if (fwrite(text.data(), 1, (size_t) len, f) != (size_t) len) { lrm_set_error("cannot write: %s", po.sites_path); return -1; }
        }
        return 0;
    }
    // the variant records of window positions [first, first + count) as VCF lines; a table that did not fit is asked for again
    // with the reported total
    int write_variants_of(FILE *f, uint64_t first, uint64_t count) {
        DevMem d_vars, d_n;
        const lrm_pileup_variant_options opt = {po.call, vo.hom_pct, {0u, 0u, 0u}};
        uint64_t cap = std::min<uint64_t>(3 * count, 4096 + count / 256), n_vars = 0;
        if (d_n.room(8)) return -1;
        for (;;) {
            if (d_vars.room(cap * sizeof(lrm_pileup_variant))) return -1;
            if (lrm_pileup_variants_dev(acc, &opt, first, count, (lrm_pileup_variant *) d_vars.p, cap, (uint64_t *) d_n.p, nullptr)) return -1;
            if (down(&n_vars, d_n.p, 8)) return -1;
            if (n_vars <= cap) break;
            cap = n_vars;
        }
        std::vector<lrm_pileup_variant> vars((size_t) n_vars);
        if (down(vars.data(), d_vars.p, n_vars * sizeof(lrm_pileup_variant))) return -1;
        uint64_t longest = 0;
        for (int k = 0; k < hi.mta_len; ++k) longest = std::max<uint64_t>(longest, hi.mta[k].name ? hi.mta[k].name_len : 0);
        const uint64_t chunk = 1u << 14;
        std::vector<char> text;
        for (uint64_t at = 0; at < n_vars; at += chunk) {
            const uint64_t k = std::min(chunk, n_vars - at);
            uint64_t room = 1;                                                // (a deletion's REF holds its deleted bases)
            for (uint64_t j = 0; j < k; ++j) room += longest + 128u + (vars[at + j].kind == LRM_CALL_DEL ? vars[at + j].len : 0u);
            if (text.size() < room) text.resize((size_t) room);
            const int64_t len = lrm_pileup_variants_format_vcf(hi.mta, hi.mta_len, (const char *) hi.content, vars.data() + at, k, text.data(), (int64_t) text.size());
            if (len < 0) return -1;
            if (fwrite(text.data(), 1, (size_t) len, f) != (size_t) len) { lrm_set_error("cannot write: %s", vo.vcf_path); return -1; }
        }
        return 0;
    }
    // the polished bytes of window positions [first, first + count), 60 columns a line; col: the column the line stands at
    int write_polish_of(FILE *f, uint64_t first, uint64_t count, uint32_t *col) {
        DevMem d_seq, d_len;
        uint64_t cap = count + count / 64 + 64, len = 0;
        if (d_len.room(8)) return -1;
        for (;;) {
            if (d_seq.room(cap)) return -1;
            if (lrm_pileup_polish_dev(acc, &po.call, first, count, (uint8_t *) d_seq.p, cap, (uint64_t *) d_len.p, nullptr)) return -1;
            if (down(&len, d_len.p, 8)) return -1;
            if (len <= cap) break;
            cap = len;
        }
        std::vector<char> seq((size_t) len);
        if (down(seq.data(), d_seq.p, len)) return -1;
        std::string lines;
        lines.reserve((size_t) (len + len / 60 + 2));
        for (uint64_t at = 0; at < len;) {
            const uint64_t k = std::min<uint64_t>(60u - *col, len - at);
            lines.append(seq.data() + at, (size_t) k);
            at += k;
            *col += (uint32_t) k;
            if (*col == 60u) { lines.push_back('\n'); *col = 0; }
        }
        if (fwrite(lines.data(), 1, lines.size(), f) != lines.size()) { lrm_set_error("cannot write: %s", po.fasta_path); return -1; }
        return 0;
    }
    int write_pileup() {
        if (hipSetDevice(device) != hipSuccess) { (void) hipGetLastError(); lrm_set_error("no HIP device %d", device); return -1; }
        FILE *fs = nullptr, *ff = nullptr;
        if (po.sites_path && !(fs = fopen(po.sites_path, "wb"))) { lrm_set_error("cannot create: %s", po.sites_path); return -1; }
        if (po.fasta_path && !(ff = fopen(po.fasta_path, "wb"))) { lrm_set_error("cannot create: %s", po.fasta_path); if (fs) fclose(fs); return -1; }
        FILE *fv = nullptr;
        if (vcf_on && !(fv = fopen(vo.vcf_path, "wb"))) { lrm_set_error("cannot create: %s", vo.vcf_path); if (fs) fclose(fs); if (ff) fclose(ff); return -1; }
        // (site ranks and byte ranks of one call are 32-bit: a sequence goes through in pieces below both bounds)
        const uint64_t piece = 0xFFFFFFFFull / (po.ins_cols + 1u);
        int rc = 0;
        if (fv) {                                                             // the header names every sequence of the index
            uint64_t room = 2048 + (vo.sample ? strlen(vo.sample) : 0);
            for (int k = 0; k < hi.mta_len; ++k) room += 64u + (hi.mta[k].name ? hi.mta[k].name_len : 0);
            std::vector<char> head((size_t) room);
            const int64_t len = lrm_vcf_header(hi.mta, hi.mta_len, vo.sample, head.data(), (int64_t) head.size());
            if (len < 0) rc = -1;
            else if (fwrite(head.data(), 1, (size_t) len, fv) != (size_t) len) { lrm_set_error("cannot write: %s", vo.vcf_path); rc = -1; }
        }
        // (record ranks of one call are 32-bit too, three records a position: a run is cut only where a sequence ends or a
        // piece of 2^32 / 3 positions does)
        const uint64_t var_piece = 0xFFFFFFFFull / 3u;
        for (int s = po.seq < 0 ? 0 : po.seq; !rc && s < (po.seq < 0 ? hi.mta_len : po.seq + 1); ++s) {
            const lrm_mta_entry &m = hi.mta[s];
            uint32_t col = 0;
            if (ff && (fputc('>', ff) == EOF || (m.name && fwrite(m.name, 1, m.name_len, ff) != m.name_len) || fputc('\n', ff) == EOF)) { lrm_set_error("cannot write: %s", po.fasta_path); rc = -1; }
            for (uint64_t at = 0; !rc && at < m.seq_len; at += piece) {
                const uint64_t first = m.offset - pile_lo + at, count = std::min<uint64_t>(piece, m.seq_len - at);
                if (fs) rc = write_sites_of(fs, first, count);
                if (!rc && ff) rc = write_polish_of(ff, first, count, &col);
            }
            if (!rc && ff && col && fputc('\n', ff) == EOF) { lrm_set_error("cannot write: %s", po.fasta_path); rc = -1; }
            for (uint64_t at = 0; fv && !rc && at < m.seq_len; at += var_piece)
                rc = write_variants_of(fv, m.offset - pile_lo + at, std::min<uint64_t>(var_piece, m.seq_len - at));
        }
        if (fv && fclose(fv) != 0 && !rc) { lrm_set_error("cannot write: %s", vo.vcf_path); rc = -1; }
        if (fs && fclose(fs) != 0 && !rc) { lrm_set_error("cannot write: %s", po.sites_path); rc = -1; }
        if (ff && fclose(ff) != 0 && !rc) { lrm_set_error("cannot write: %s", po.fasta_path); rc = -1; }
        return rc;
    }

    // all batches: starts the stages, submits on this thread, and takes everything down again in the order that matters
    int run() {
        for (int k = 0; k < NSETS; ++k) { sets.emplace_back(new BatchSet); free_sets.push(sets.back().get()); }
        for (int k = 0; k < 3; ++k) free_texts.push(std::unique_ptr<TextBatch>(new TextBatch));
        std::thread pin(&AccalnRun::pinner, this), load(&AccalnRun::loader, this), fmt(&AccalnRun::formatter, this), flush(&AccalnRun::flusher, this);
        submit_loop();
        mapped.close();
        free_sets.close();
        load.join();
        fmt.join();
        flush.join();
        { std::lock_guard<std::mutex> lk(dims_m); dims_stop = true; }
        dims_cv.notify_all();
        pin.join();
        int rc = err.get();
        if (rc) lrm_set_error("%s", err.msg.c_str());
        else if (acc) rc = write_pileup();                                    // every batch has been waited for: all counts are in
        const double t_done = now();
        if (acc) { lrm_pileup_free(acc); acc = nullptr; }
        if (gpu) { lrm_index_free(gpu); gpu = nullptr; }                      // before the pinned buffers of the sets go
        sets.clear();
        if (verbose) fprintf(stderr, "[lrm accaln] last batch written %.2f s after the upload; freeing the device image and the pinned sets %.2f s\n",
                             t_done - t_upload, now() - t_done);
        return rc;
    }

    void end() {
        if (rd) lrm_reader_close(rd);
        if (out_fd >= 0) close(out_fd);
        if (verbose)
            fprintf(stderr, "[lrm accaln] index files %.2f s, upload %.2f s, batches %.2f s wall (busy: loader %.2f, device waits %.2f, "
                            "formatter %.2f, write %.2f)\n", t_read_idx - t_begin, t_upload - t_read_idx, now() - t_upload, t_load, t_map,
                    t_fmt, t_write);
        if (acc) lrm_pileup_free(acc);
        if (gpu) lrm_index_free(gpu);
        lrm_host_index_free(&hi);
    }
};

}  // namespace

// one run of the flow: SAM (lrm_accaln*) or PAF (lrm_accaln_paf) into out_path
static int accaln_run(const char *genome, const char *reads_path, const char *out_path, lrm_params p, lrm_gact_params gp, int device,
                      long rg_id, uint64_t *total_out, uint64_t *valid_out, const lrm_map_options *user, bool mapq, bool paf, bool md = false,
                      const lrm_secondary_options *so = nullptr, const lrm_accaln_pileup_options *po = nullptr,
                      const lrm_accaln_vcf_options *vo = nullptr) {
    AccalnRun r(p, gp, device, mapq, paf, md);
    memset(&r.so, 0, sizeof(r.so));
    memset(&r.po, 0, sizeof(r.po));
    memset(&r.vo, 0, sizeof(r.vo));
    if (vo) { r.vcf_on = true; r.vo = *vo; }
    if (so) { r.sec = true; lrm_options_over_defaults(&r.so, so); }
    if (r.take_options(user)) return -1;
    if (lrm_host_index_read(genome, &r.hi)) return -1;
    int rc = 0;
    if (po) {                                                                 // the window of the accumulator: one sequence, or all of them
        r.pile_on = true;
        r.po = *po;
        if (po->seq < -1 || po->seq >= r.hi.mta_len) { lrm_set_error("lrm_accaln_pileup_options.seq %d: -1 or a sequence of the index (%d)", po->seq, r.hi.mta_len); rc = -1; }
        else if (r.hi.mta_len < 1) { lrm_set_error("the index holds no sequence"); rc = -1; }
        else {
            const lrm_mta_entry &a = r.hi.mta[po->seq < 0 ? 0 : po->seq], &b = r.hi.mta[po->seq < 0 ? r.hi.mta_len - 1 : po->seq];
            r.pile_lo = a.offset; r.pile_hi = b.offset + b.seq_len;
        }
    }
    if (rc == 0) rc = r.begin(reads_path, out_path, rg_id);
    if (rc == 0) rc = r.run();
    r.end();
    if (total_out) *total_out = r.total;
    if (valid_out) *valid_out = r.valid;
    return rc;
}
// mapq: the mapping-quality records come back with every batch, column 5 and v1:i / v2:i print them (lrm_sam_format_mapq)
extern "C" int lrm_accaln_mapq(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                               lrm_gact_params gp, int device, long rg_id, uint64_t *total_out, uint64_t *valid_out,
                               const lrm_map_options *user, int mapq) {
    return accaln_run(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, mapq != 0, false);
}
// md: the summary records and the difference events come back with every batch, NM:i and MD:Z print them (lrm_sam_format_md)
extern "C" int lrm_accaln_md(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                             lrm_gact_params gp, int device, long rg_id, uint64_t *total_out, uint64_t *valid_out,
                             const lrm_map_options *user, int mapq, int md) {
    return accaln_run(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, mapq != 0, false, md != 0);
}
// so: after a batch's wait its candidates go through lrm_secondary_batch, FLAG 256 lines print the reported ones
// (lrm_sam_format_secondary); so == NULL: lrm_accaln_mapq with its mode on
extern "C" int lrm_accaln_secondary(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                                    lrm_gact_params gp, int device, long rg_id, uint64_t *total_out, uint64_t *valid_out,
                                    const lrm_map_options *user, const lrm_secondary_options *so) {
    return accaln_run(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, true, false, false, so);
}
// PAF: the alignment summary records come back with every batch, lrm_paf_format's lines print them; no header
extern "C" int lrm_accaln_paf(const char *genome, const char *reads_path, const char *paf_path, lrm_params p, lrm_gact_params gp,
                              int device, uint64_t *total_out, uint64_t *valid_out, const lrm_map_options *user, int mapq) {
    return accaln_run(genome, reads_path, paf_path, p, gp, device, 0, total_out, valid_out, user, mapq != 0, true);
}
extern "C" int lrm_accaln_opt(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                              lrm_gact_params gp, int device, long rg_id, uint64_t *total_out, uint64_t *valid_out,
                              const lrm_map_options *user) {
    return lrm_accaln_mapq(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, 0);
}
extern "C" int lrm_accaln(const char *genome, const char *reads_path, const char *sam_path, lrm_params p,
                          lrm_gact_params gp, int device, long rg_id, uint64_t *total_out, uint64_t *valid_out) {
    return lrm_accaln_mapq(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, nullptr, 0);
}
// po: every batch adds to one accumulator (lrm_map_batch_submit_ex3), and behind the last wait the flow writes the sites table
// and the polished sequences; po == NULL: lrm_accaln_mapq.  vo: the variant records of the same slices as a VCF file too
static int accaln_pileup(const char *genome, const char *reads_path, const char *sam_path, lrm_params p, lrm_gact_params gp, int device,
                         long rg_id, uint64_t *total_out, uint64_t *valid_out, const lrm_map_options *user, int mapq,
                         const lrm_accaln_pileup_options *po, const lrm_accaln_vcf_options *vo) {
    if (!genome || !reads_path) { lrm_set_error("null argument"); return -1; }
    if (po->struct_size < sizeof(lrm_accaln_pileup_options)) { lrm_set_error("lrm_accaln_pileup_options.struct_size %u: the struct has %zu bytes", po->struct_size, sizeof(lrm_accaln_pileup_options)); return -1; }
    if (po->reserved != 0u || po->reserved2 != 0u || po->call.reserved != 0u) { lrm_set_error("lrm_accaln_pileup_options: a reserved field is not 0"); return -1; }
    if (po->min_mapq != 0u && mapq == 0) { lrm_set_error("lrm_accaln_pileup_options.min_mapq needs mapq (the filter reads the records of the mapping-quality stage)"); return -1; }
    if (po->ins_cols > LRM_PILEUP_INS_COLS_MAX) { lrm_set_error("pileup: %u insertion columns, at most %d", po->ins_cols, LRM_PILEUP_INS_COLS_MAX); return -1; }
    if (po->call.min_pct > 100u) { lrm_set_error("pileup calls: min_pct %u above 100", po->call.min_pct); return -1; }
    if (vo) {
        if (vo->struct_size < sizeof(lrm_accaln_vcf_options)) { lrm_set_error("lrm_accaln_vcf_options.struct_size %u: the struct has %zu bytes", vo->struct_size, sizeof(lrm_accaln_vcf_options)); return -1; }
        if (vo->reserved != 0u) { lrm_set_error("lrm_accaln_vcf_options: the reserved field is not 0"); return -1; }
        if (vo->hom_pct > 100u) { lrm_set_error("pileup variants: hom_pct %u above 100", vo->hom_pct); return -1; }
        if (!vo->vcf_path) { lrm_set_error("lrm_accaln_vcf_options.vcf_path is NULL"); return -1; }
    }
    return accaln_run(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, mapq != 0, false, false, nullptr, po, vo);
}
extern "C" int lrm_accaln_pileup(const char *genome, const char *reads_path, const char *sam_path, lrm_params p, lrm_gact_params gp,
                                 int device, long rg_id, uint64_t *total_out, uint64_t *valid_out, const lrm_map_options *user, int mapq,
                                 const lrm_accaln_pileup_options *po) {
    if (!po) return lrm_accaln_mapq(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, mapq);
    return accaln_pileup(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, mapq, po, nullptr);
}
// vo == NULL: exactly lrm_accaln_pileup; the VCF file needs the accumulator, so vo without po is refused
extern "C" int lrm_accaln_pileup_vcf(const char *genome, const char *reads_path, const char *sam_path, lrm_params p, lrm_gact_params gp,
                                     int device, long rg_id, uint64_t *total_out, uint64_t *valid_out, const lrm_map_options *user, int mapq,
                                     const lrm_accaln_pileup_options *po, const lrm_accaln_vcf_options *vo) {
    if (!vo) return lrm_accaln_pileup(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, mapq, po);
    if (!po) { lrm_set_error("lrm_accaln_pileup_vcf: the VCF file needs lrm_accaln_pileup_options (the accumulator)"); return -1; }
    return accaln_pileup(genome, reads_path, sam_path, p, gp, device, rg_id, total_out, valid_out, user, mapq, po, vo);
}
