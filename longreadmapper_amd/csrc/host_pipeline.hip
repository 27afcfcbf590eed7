// host_pipeline.hip -- the upload / compute / download pipeline behind the host-buffer entry points (lrm_host.hip)
//
// Every replica owns TWO long-lived host threads and two SLOTS of device resources (mirrors of the caller's arrays,
// workspaces, dense result buffers):
//   issuer     takes the next slice of a submitted batch, waits for a free slot, and hands the whole slice to the
//              device without waiting for anything: the reads are uploaded and SEEDED in sub-batches (two seed streams),
//              the EXTENSION runs over groups of sub-batches on two extension streams as soon as their seeds are done;
//   collector  follows the extension groups in order: small result arrays, then the op bytes and the
//              reverse-complemented reads (the only rows of reads_buf that changed, alnmain.c:437).
// With two slots the upload and the seeds of batch k+1 run under the extension tail and the result download of
// batch k -- the serial chain that bounds a single call.  Stream priorities: results > extension > seeds.
//
// How results reach the caller (lrm_map_options): always as a DENSE image packed on the device (the used part of every
// CIGAR row, the reverse-complemented reads) that crosses the link by DMA at its full rate -- a strided hipMemcpy2D of
// the same rows does 6 GB/s, and a kernel writing the caller's pinned memory itself collapses to 2-9 GB/s as soon as
// compute kernels own the chip (tools/d2h_under_load.hip).
//   dense_results   the op bytes stay dense: ONE DMA per group straight into the caller's (pinned) store_mem, and
//                   cig[i].cigar points into it (the convention of mutils.c:97-103 kept).  The reverse-complemented
//                   reads are the only rows left to place: through a ring of pinned chunks, by the collector alone.
//   rows (default)  cig[i].cigar = store_mem + i*store_stride as in alnmain.c:322-325: the whole image comes down
//                   through the ring and a small memcpy team scatters it.
//
// Host CPU: every wait for the device is a sleep-poll on an event (hipEventSynchronize and hipStreamSynchronize spin
// a core for the whole wait on this platform, blocking-sync events included: tools/hostlink_bench.hip).
// No CPU fallback: without a HIP device every entry point fails.
#include <unistd.h>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <exception>
#include <new>
#include "host_pipeline.h"
#include "op_rows.h"

namespace {

// Waits for an event WITHOUT spinning: hipEventSynchronize / hipStreamSynchronize burn a core for the whole wait
// (measured, also for hipEventBlockingSync events), and 8 replicas x 2 threads of that is the host's whole CPU share.
int wait_event(hipEvent_t ev) {
    useconds_t nap = 20;
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return 0;
        (void) hipGetLastError();
        if (e != hipErrorNotReady) { lrm_set_error("hipEventQuery failed: %s", hipGetErrorString(e)); return -1; }
        usleep(nap);
        if (nap < 200) nap += 20;
    }
}

}  // namespace

int lrm_wait_event(void *ev) { return wait_event((hipEvent_t) ev); }

void LrmHostCtx::drain() {
    for (Stream &s : seed) (void) hipStreamSynchronize(s);
    for (Stream &s : ext) (void) hipStreamSynchronize(s);
    (void) hipStreamSynchronize(up);
    (void) hipStreamSynchronize(down);
}

namespace {

int new_event(Event &e) {
    if (e.h) return 0;
    if (hipEventCreateWithFlags(&e.h, hipEventDisableTiming) != hipSuccess) { (void) hipGetLastError(); e.h = nullptr; lrm_set_error("event creation failed"); return -1; }
    return 0;
}
int new_chunk(Pinned &p, uint64_t bytes) {
    if (p.h) return 0;
    if (hipHostMalloc(&p.h, bytes, hipHostMallocDefault) != hipSuccess) { p.h = nullptr; lrm_set_error("pinned staging allocation failed"); return -1; }
    return 0;
}
int new_stream(Stream &s, int priority) {
    if (s.h) return 0;
    if (hipStreamCreateWithPriority(&s.h, hipStreamNonBlocking, priority) != hipSuccess) { s.h = nullptr; lrm_set_error("stream creation failed"); return -1; }
    return 0;
}

int ctx_init(LrmHostCtx &c) {
    if (c.ready) return 0;
    for (int b = 0; b < 2; ++b) {
        if (new_chunk(c.pin_up[b], STAGE_CHUNK) || new_event(c.ev_pin_up[b])) return -1;
        for (Slot &S : c.slots) if (new_event(S.ev_dense[b])) return -1;
    }
    for (int b = 0; b < N_RING; ++b)
        if (new_chunk(c.pin_dn[b], RING_CHUNK) || new_event(c.ev_pin_dn[b])) return -1;
    if (new_event(c.ev_small) || new_event(c.ev_tail)) return -1;
    // Priorities: the result path first (pack kernels + downloads), then the extension of a finished group, then
    // the seed kernels of later sub-batches -- otherwise every group's extension finishes at the very end, behind
    // all the seed work, and the downloads of all but the first group run after the compute instead of under it.
    int prio_lo = 0, prio_hi = 0;
    (void) hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);          // numerically lower = higher priority
    const int p_seed = prio_lo, p_ext = prio_hi < prio_lo ? prio_lo - 1 : prio_lo, p_down = prio_hi;
    if (new_stream(c.up, p_down) || new_stream(c.down, p_down)) return -1;
    for (Stream &s : c.ext) if (new_stream(s, p_ext)) return -1;
    for (Stream &s : c.seed) if (new_stream(s, p_seed)) return -1;
    c.ready = true;
    return 0;
}

int ensure_events(std::vector<Event> &v, size_t n) {
    while (v.size() < n) {
        Event e;
        if (new_event(e)) return -1;
        v.push_back(std::move(e));
    }
    return 0;
}

void par_memcpy(void *dst, const void *src, uint64_t bytes, int threads) {
    if (threads <= 1 || bytes < (4ull << 20)) { memcpy(dst, src, bytes); return; }
    const uint64_t piece = 1ull << 20, np = (bytes + piece - 1) / piece;
#pragma omp parallel for schedule(static) num_threads(threads)
    for (uint64_t i = 0; i < np; ++i) {
        const uint64_t o = i * piece, l = bytes - o < piece ? bytes - o : piece;
        memcpy((char *) dst + o, (const char *) src + o, l);
    }
}

// pinned (hipHostMalloc / hipHostRegister) memory can be handed to the DMA engines as it is
bool is_pinned(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void) hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// host -> device on the upload stream; returns when the last byte has been handed to the DMA engine (not when
// it has landed: later work is ordered behind the upload stream)
int h2d(LrmHostCtx &c, void *d_dst, const void *h_src, uint64_t bytes, bool pinned, int threads) {
    if (bytes == 0) return 0;
    if (pinned) { HIPCHK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c.up)); return 0; }
    for (uint64_t o = 0; o < bytes; o += STAGE_CHUNK, ++c.up_seq) {
        const int b = (int) (c.up_seq & 1);
        const uint64_t l = bytes - o < STAGE_CHUNK ? bytes - o : STAGE_CHUNK;
        if (c.pin_up_used[b] && wait_event(c.ev_pin_up[b])) return -1;         // the chunk's previous DMA has drained
        par_memcpy(c.pin_up[b], (const char *) h_src + o, l, threads);
        HIPCHK(hipMemcpyAsync((char *) d_dst + o, c.pin_up[b], l, hipMemcpyHostToDevice, c.up));
        HIPCHK(hipEventRecord(c.ev_pin_up[b], c.up));
        c.pin_up_used[b] = true;
    }
    return 0;
}

// dense device buffer -> the caller's memory through the context's ring of pinned chunks: contiguous DMA pieces, every
// piece copied into place while the next ones fly.  Entries i with off[i] (16-byte aligned, ascending) / len[i] in the
// dense buffer go to dst[i]; dst == nullptr: the image is copied as it is to `flat`.
// `threads` = 1: the collector copies alone with plain memcpy -- no OpenMP team, whose idle threads spin between the
// pieces (8 threads spinning through every download was 0.35 CPU-s per Gbp); the row layout of the op bytes (1.1 GB per
// Gbp to scatter) needs the team.
// `after_issue` runs once, as soon as the last piece has been handed to the DMA engine (before the ring is drained):
// whatever it queues flies while this thread still copies.
template <typename F>
int d2h_ring(LrmHostCtx &c, const uint8_t *d_dense, uint64_t total, const uint64_t *off, const uint32_t *len,
             uint8_t *const *dst, uint64_t rows, uint8_t *flat, int threads, F after_issue) {
    if (total == 0) return after_issue();
    const uint64_t np = (total + RING_CHUNK - 1) / RING_CHUNK;
    uint64_t row_lo = 0;                                              // first entry that may still have bytes at or after the piece
    for (uint64_t k = 0; k < np + N_RING - 1; ++k) {
        if (k < np) {                                                 // issue piece k (its chunk was drained N_RING pieces ago)
            const int b = (int) (k % N_RING);
            const uint64_t o = k * RING_CHUNK, l = total - o < RING_CHUNK ? total - o : RING_CHUNK;
            HIPCHK(hipMemcpyAsync(c.pin_dn[b], d_dense + o, l, hipMemcpyDeviceToHost, c.down));
            HIPCHK(hipEventRecord(c.ev_pin_dn[b], c.down));
            if (k + 1 == np && after_issue()) return -1;
        }
        if (k + 1 < N_RING) continue;
        const uint64_t p = k + 1 - N_RING;                            // drain piece p while the later ones fly
        if (p >= np) break;
        const int pb = (int) (p % N_RING);
        if (wait_event(c.ev_pin_dn[pb])) return -1;
        const uint8_t *chunk = (const uint8_t *) c.pin_dn[pb].h;
        const uint64_t c0 = p * RING_CHUNK, c1 = c0 + (total - c0 < RING_CHUNK ? total - c0 : RING_CHUNK);
        if (!dst) { par_memcpy(flat + c0, chunk, c1 - c0, threads); continue; }
        while (row_lo < rows && off[row_lo] + len[row_lo] <= c0) ++row_lo;
        uint64_t row_hi = row_lo;
        while (row_hi < rows && off[row_hi] < c1) ++row_hi;
        auto place = [&](uint64_t r) {                                // the part of entry r that lies in this piece
            const uint64_t a = off[r] > c0 ? off[r] : c0, e = off[r] + len[r] < c1 ? off[r] + len[r] : c1;
            if (e > a) memcpy(dst[r] + (a - off[r]), chunk + (a - c0), e - a);
        };
        if (threads <= 1) {
            for (uint64_t r = row_lo; r < row_hi; ++r) place(r);
        } else {
#pragma omp parallel for schedule(static) num_threads(threads)
            for (uint64_t r = row_lo; r < row_hi; ++r) place(r);
        }
    }
    return 0;
}

// Seed sub-batches of one device pass: small enough that the first kernels start a few milliseconds after the
// upload begins and the uploads hide behind them.
constexpr uint64_t PIPE_MIN_READS = 8192;
uint64_t pipe_subs(uint64_t n, const LrmMapTune &mt) {
    if (mt.sub_batches >= 1) return mt.sub_batches < n ? mt.sub_batches : n;
    const uint64_t k = n / PIPE_MIN_READS;
    return k < 2 ? 1 : (k > 12 ? 12 : k);
}
// Sub-batches per extension group: the bit-sliced kernel carries one read per LANE, so it wants >= 32 k reads
// per launch for decent SIMD coverage; two groups are in extension at once (two streams).  Measured per 100 k-read
// batch [r2, one batch at a time]: groups of 17 k reads 69 ms, 25 k 73 ms, 33 k 78 ms.
// With ANOTHER slice in flight on the device the chain inside one slice no longer matters, the fill of the chip does:
// groups of ~50 k reads (two per 100 k-read batch: 41.4 ms per batch with two in flight against 48.3 with groups of
// 17 k [r3]; a single call prefers the small groups: 58.0 against 62.0).
constexpr uint64_t EXT_GROUP_READS = 16384, EXT_GROUP_READS_BUSY = 49152;
uint64_t ext_group_subs(uint64_t sub, uint64_t nsub, const LrmMapTune &mt, bool busy) {
    if (mt.group_subs >= 1) return mt.group_subs < nsub ? mt.group_subs : nsub;
    const uint64_t want = busy ? EXT_GROUP_READS_BUSY : EXT_GROUP_READS;
    const uint64_t g = (want + sub - 1) / (sub ? sub : 1);
    return g < 1 ? 1 : (g > nsub ? nsub : g);
}

int get_ws(WsPtr &ws, lrm_index *idx, uint64_t n, uint32_t max_len, uint32_t seed_len, uint32_t thres, int parts) {
    if (ws && n <= ws->n_max && max_len <= ws->max_len && (!(parts & LRM_WS_SEED) || (seed_len == ws->seed_len && thres <= ws->thres))) return 0;
    ws.reset();                                                  // (freed first: the two need not fit side by side)
    lrm_workspace *w = nullptr;
    const int rc = lrm_workspace_create_parts(&w, idx, n, max_len, seed_len, thres, parts);
    ws.reset(w);
    return rc;
}

double thread_cpu_ms() {                                            // CPU time of the calling thread so far (LRM_HOST_VERBOSE)
    timespec ts;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

int take_errors(Slot &s) {
    int rc = 0;
    for (int k = 0; k < N_SEED_STREAMS; ++k) if (lrm_ws_take_error(s.ws_seed[k].get())) rc = -2;
    for (int k = 0; k < N_EXT_STREAMS; ++k) if (lrm_ws_take_error(s.ws_ext[k].get())) rc = -2;
    return rc;
}

}  // namespace

// What the slice asks of every per-read array (host_pipeline.h), decided once: the issuer allocates and launches by it,
// the collector downloads and copies out by it.
void SliceJob::plan_arrays() {
    const bool seed = (j.mode & DO_SEED) != 0, ext = (j.mode & DO_EXTEND) != 0;
    want_anchor = j.anchor_out && ext && mt.anchored;
    want_mapq = j.mapq_out && seed;
    want_diff = j.diff_off && ext;
    want_summary = (j.summary_out || want_diff) && ext;              // (the events are sized and placed by the records' counts)
    text = mt.cigar_text != 0 && ext;
    //               bytes per read        on the device  downloaded   the caller's array
    arr[A_BEST]   = {sizeof(lrm_entry),    true,          seed,        j.best_out};
    arr[A_NOPS]   = {4,                    ext,           ext,         nullptr};          // reaches the caller in cig[]
    arr[A_SCORE]  = {4,                    ext,           ext,         j.score};
    arr[A_META]   = {sizeof(lrm_seq_meta), ext,           ext,         j.meta};
    arr[A_MR]     = {4,                    ext,           ext,         j.meta_r};
    arr[A_TLEN]   = {4,                    text,          text,        nullptr};          // sizes the text rows of the dense image
    arr[A_ANCHOR] = {sizeof(lrm_anchor),   want_anchor,   want_anchor, j.anchor_out};
    arr[A_MAPQ]   = {sizeof(lrm_mapq),     want_mapq,     want_mapq,   j.mapq_out};
    arr[A_SUMMARY] = {sizeof(lrm_aln_summary), want_summary, want_summary, j.summary_out};
    arr[A_READS]  = {j.stride,             true,          false,       nullptr};          // uploaded per sub-batch
    arr[A_LENS]   = {4,                    true,          false,       nullptr};
    arr[A_STORE]  = {dstride,              ext,           false,       nullptr};          // leaves in the dense image
    // pinned staging of a unit of m reads: array after array, m elements each; the parts made of 8-byte multiples (the
    // records, the u64 offset table) start at a multiple of 8 for every m
    uint64_t at = 0;
    auto place = [&at](uint64_t elem) { if (elem % 8 == 0) at = (at + 7) & ~7ull; const uint64_t o = at; at += elem; return o; };
    for (int a = 0; a < N_SMALL; ++a) if (arr[a].down) arr[a].stage = place(arr[a].elem);
    stage_off = place(2 * sizeof(uint64_t));
    stage_len = place(2 * sizeof(uint32_t));
    if (want_diff) stage_diff = place(2 * sizeof(uint64_t));         // m + 1 entries fit the 2 m of a unit
    stage_row = (at + 7) & ~7ull;
}

namespace {

// ---- issuer: plan a slice and hand all of it to the device (no waits but for pageable staging chunks) -------------------------
int plan_and_issue(LrmHostCtx &c, SliceJob &sj) {
    lrm_index *idx = c.idx;
    const MapJob &j = sj.j;
    const LrmMapTune &mt = sj.mt;
    Slot &S = *sj.slot;
    const uint64_t n = j.n, nsub = pipe_subs(n, mt), sub = (n + nsub - 1) / nsub;
    sj.dstride = (j.store_stride + 3) & ~3ull;           // the bit-sliced kernel stores CIGAR bytes four at a time
    sj.seed_only = !(j.mode & DO_EXTEND);
    sj.plan_arrays();
    const uint64_t dstride = sj.dstride;
    const bool want_anchor = sj.want_anchor, want_mapq = sj.want_mapq;
    const bool pin_reads = is_pinned(j.reads);
    std::vector<Range> &subs = sj.subs, &units = sj.units;
    std::vector<size_t> &ends = sj.ends, &unit_of = sj.unit_of;
    for (uint64_t off = 0; off < n; off += sub) subs.push_back({off, n - off < sub ? n - off : sub});
    const uint64_t gsub = (j.mode & DO_EXTEND) ? ext_group_subs(sub, subs.size(), mt, sj.busy) : 1;
    for (size_t k = gsub; k < subs.size(); k += gsub) ends.push_back(k);
    ends.push_back(subs.size());
    unit_of.resize(subs.size());
    for (size_t g = 0, k0 = 0; g < ends.size(); k0 = ends[g], ++g) {
        units.push_back({subs[k0].off, subs[ends[g] - 1].off + subs[ends[g] - 1].m - subs[k0].off});
        for (size_t k = k0; k < ends[g]; ++k) unit_of[k] = g;
    }
    const int n_ext_streams = mt.ext_streams >= 1 && mt.ext_streams <= N_EXT_STREAMS ? mt.ext_streams : 2;
    const int n_seed_streams = mt.seed_streams >= 1 && mt.seed_streams <= N_SEED_STREAMS ? mt.seed_streams : 2;
    uint64_t unit_max = 0;
    for (auto &u : units) unit_max = u.m > unit_max ? u.m : unit_max;
    if (n > 0x7fffffffull) { lrm_set_error("batch too large"); return -1; }
    if (j.mode & DO_SEED)
        for (int s = 0; s < n_seed_streams && (size_t) s < subs.size(); ++s)
            if (get_ws(S.ws_seed[s], idx, sub, sj.max_len, j.p.seed_len, j.p.thres, LRM_WS_SEED) ||
                (want_mapq && !lrm_mapq_phase_buf(S.ws_seed[s].get()))) return -1;
    if (j.mode & DO_EXTEND)
        for (int s = 0; s < n_ext_streams && (size_t) s < units.size(); ++s)
            if (get_ws(S.ws_ext[s], idx, unit_max, sj.max_len, 20, 300, LRM_WS_EXTEND)) return -1;
    if (ensure_events(S.ev_up, subs.size()) || ensure_events(S.ev_seed, subs.size()) || ensure_events(S.ev_ext, units.size())) return -1;
    DevSlot *const d = S.dev;
    for (int a = 0; a < N_ARRAYS; ++a)
        if (sj.arr[a].on_dev && d[a].ensure(n * sj.arr[a].elem)) {
            lrm_set_error(a == A_ANCHOR ? "allocation for the anchor records failed" : a == A_MAPQ ? "allocation for the mapping-quality records failed" :
                          a == A_SUMMARY ? "allocation for the alignment summary records failed" : "device allocation failed");
            return -1;
        }
    // (the dense result buffers and offset tables at their worst-case size for a unit, so that the collector never
    //  reallocates -- a hipFree would drain the whole device -- while other work is in flight)
    if (j.mode & DO_EXTEND)
        for (int b = 0; b < 2; ++b)
            if (S.dense[b].ensure(unit_max * (dstride + j.stride + 32)) || S.offs[b].ensure(unit_max * 2 * 12)) { lrm_set_error("device allocation failed"); return -1; }
    // (the event buffer of a group like the buffers above, so that the collector does not reallocate: sized here for one event
    //  in four of the longest read's bases per read -- twice what ONT reads give -- and never below what an earlier group of
    //  this slot needed; only a group beyond that grows it in the collector)
    if (sj.want_diff && (S.diff_off.ensure((unit_max + 1) * sizeof(uint64_t)) ||
                         S.diff_ev.ensure(unit_max * ((uint64_t) sj.max_len / 4 + 64) * sizeof(uint32_t)))) { lrm_set_error("allocation for the difference events failed"); return -1; }
    if (S.h_small.ensure(n * sj.stage_row)) { lrm_set_error("pinned staging allocation failed"); return -1; }
    S.dense_used[0] = S.dense_used[1] = false;

    for (uint64_t k = 0; k < subs.size(); ++k) {
        if (sj.failed.load()) return 0;                                            // the collector hit an error: stop feeding the device
        const int s = (int) (k % (uint64_t) n_seed_streams);
        const uint64_t m = subs[k].m, off = subs[k].off;
        const double t_i0 = sj.clk.ms();
        char *dr = (char *) d[A_READS].p + off * j.stride;
        if (h2d(c, dr, j.reads + off * j.stride, m * j.stride, pin_reads, mt.copy_threads ? (int) mt.copy_threads : c.copy_threads)) return -1;
        HIPCHK(hipMemcpyAsync((uint32_t *) d[A_LENS].p + off, j.lens + off, m * 4, hipMemcpyHostToDevice, c.up));
        if (!(j.mode & DO_SEED)) HIPCHK(hipMemcpyAsync((lrm_entry *) d[A_BEST].p + off, j.best_in + off, m * sizeof(lrm_entry), hipMemcpyHostToDevice, c.up));
        HIPCHK(hipEventRecord(S.ev_up[k], c.up));
        if (j.mode & DO_SEED) {
            HIPCHK(hipStreamWaitEvent(c.seed[s], S.ev_up[k], 0));
            if (lrm_launch_seed(idx, S.ws_seed[s].get(), dr, j.stride, (const uint32_t *) d[A_LENS].p + off, m, j.p.seed_len, j.p.thres,
                                (lrm_entry *) d[A_BEST].p + off, mt, c.seed[s], want_mapq ? lrm_mapq_phase_buf(S.ws_seed[s].get()) : nullptr)) return -1;
            // (the next sub-batch on this workspace overwrites the survivor lists: the records are made right here)
            if (want_mapq && lrm_launch_mapq(idx, S.ws_seed[s].get(), (const uint32_t *) d[A_LENS].p + off, m, j.p.seed_len, j.p.thres,
                                             (const lrm_entry *) d[A_BEST].p + off, (lrm_mapq *) d[A_MAPQ].p + off, c.seed[s])) return -1;
            HIPCHK(hipEventRecord(S.ev_seed[k], c.seed[s]));
        }
        const uint64_t g = unit_of[k];
        const bool closes = k + 1 == ends[g];
        if (closes && (j.mode & DO_EXTEND)) {                                  // the group's extension, behind its seeds / uploads
            const int xs = (int) (g % (uint64_t) n_ext_streams);
            for (uint64_t x = g ? ends[g - 1] : 0; x <= k; ++x) HIPCHK(hipStreamWaitEvent(c.ext[xs], (j.mode & DO_SEED) ? S.ev_seed[x] : S.ev_up[x], 0));
            const Range &u = units[g];
            const LrmExtendBatch b = {(char *) d[A_READS].p + u.off * j.stride, j.stride, (const uint32_t *) d[A_LENS].p + u.off, u.m, sj.max_len,
                                      (const lrm_entry *) d[A_BEST].p + u.off, (uint8_t *) d[A_STORE].p + u.off * dstride, dstride,
                                      (int32_t *) d[A_NOPS].p + u.off, (int32_t *) d[A_SCORE].p + u.off, (lrm_seq_meta *) d[A_META].p + u.off,
                                      (int32_t *) d[A_MR].p + u.off};
            if (want_anchor) {                                                 // what lrm_launch_extend does in this mode, with the records kept
                if (lrm_launch_extend_anchored(idx, S.ws_ext[xs].get(), b, j.gp, (lrm_anchor *) d[A_ANCHOR].p + u.off, mt.anchor_min_len, lrm_clip_of(mt),
                                               mt, c.ext[xs])) return -1;
            } else if (lrm_launch_extend(idx, S.ws_ext[xs].get(), b, j.gp, mt, c.ext[xs])) return -1;
            if (sj.want_summary &&                                             // what the alignments consist of, while the op bytes are in HBM
                lrm_launch_aln_summary(LrmOpRows{b.store, dstride, b.n_ops, b.score, b.meta_r, b.meta, u.m}, (lrm_aln_summary *) d[A_SUMMARY].p + u.off, c.ext[xs])) return -1;
            // the pileup of the group, from the mirrors as the extension left them (reverse-strand reads reverse-complemented in
            // place, with keep_reads too: that option only keeps them from coming down); the MAPQ records of the group's
            // sub-batches were complete before their ev_seed
            if (j.pile &&
                lrm_launch_pileup_add(j.pile, (const uint8_t *) b.reads, j.stride, b.lens, LrmOpRows{b.store, dstride, b.n_ops, b.score, b.meta_r, b.meta, u.m},
                                      j.pile_min_mapq ? (const lrm_mapq *) d[A_MAPQ].p + u.off : nullptr, j.pile_min_mapq, c.ext[xs])) return -1;
            if (mt.cigar_text &&                                               // length of every read's run-length CIGAR text
                lrm_launch_cigar_text(b.store, dstride, b.n_ops, b.score, b.meta_r, (uint32_t *) d[A_TLEN].p + u.off, nullptr, nullptr, u.m, c.ext[xs])) return -1;
            HIPCHK(hipEventRecord(S.ev_ext[g], c.ext[xs]));
        }
        if (closes) {
            { std::lock_guard<std::mutex> lk(sj.m); sj.issued = g + 1; }
            sj.cv.notify_all();
        }
        if (sj.clk.on) fprintf(stderr, "[lrm host] issue   off=%llu m=%llu: %.1f -> %.1f ms\n", (unsigned long long) off, (unsigned long long) m, t_i0, sj.clk.ms());
    }
    if (sj.clk.on)
        fprintf(stderr, "[lrm host] slice issued at %.1f ms (issuer thread CPU so far %.1f ms)\n", sj.clk.ms(), thread_cpu_ms());
    return 0;
}

// ---- collector: the difference events of one unit (docs/GACT_SPEC.md, "Difference events and MD:Z") --------------------------
// The unit's summary records are on the host and its op bytes still in HBM: the counts n_x + n_del become offsets, the unit
// takes its place in the caller's buffer with one atomic add on the batch's running total, the kernel writes into a device
// buffer of the unit's true total and one copy brings the events down (behind everything on the download stream).  A unit
// that does not fit leaves off = UINT64_MAX with the true counts; the total goes on counting.
int collect_diff(LrmHostCtx &c, SliceJob &sj, const Range &u, const lrm_aln_summary *h_sum, uint64_t *h_doff) {
    const MapJob &j = sj.j;
    Slot &S = *sj.slot;
    DevSlot *const d = S.dev;
    const uint64_t m = u.m, o = u.off;
    uint64_t total = 0;
    for (uint64_t i = 0; i < m; ++i) {
        h_doff[i] = total;
        j.diff_cnt[o + i] = h_sum[i].n_x + h_sum[i].n_del;
        total += (uint64_t) h_sum[i].n_x + h_sum[i].n_del;
    }
    h_doff[m] = total;
    const uint64_t base = sj.ticket->diff_total.fetch_add(total);
    const bool fits = base + total <= j.diff_cap;
    for (uint64_t i = 0; i < m; ++i) j.diff_off[o + i] = fits ? base + h_doff[i] : UINT64_MAX;
    if (!fits || total == 0) return 0;
    if (S.diff_ev.ensure((total + total / 4) * sizeof(uint32_t))) { lrm_set_error("allocation for the difference events failed"); return -1; }
    HIPCHK(hipMemcpyAsync(S.diff_off.p, h_doff, (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c.down));
    const LrmOpRows rows = {(const uint8_t *) d[A_STORE].p + o * sj.dstride, sj.dstride, (const int32_t *) d[A_NOPS].p + o,
                            (const int32_t *) d[A_SCORE].p + o, (const int32_t *) d[A_MR].p + o, (const lrm_seq_meta *) d[A_META].p + o, m};
    if (lrm_launch_aln_diff(rows, c.idx->view.content, c.idx->view.con_len, (const uint64_t *) S.diff_off.p, total, (uint32_t *) S.diff_ev.p, c.down)) return -1;
    uint8_t *dst = (uint8_t *) (j.diff_events + base);
    if (is_pinned(dst)) { HIPCHK(hipMemcpyAsync(dst, S.diff_ev.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, c.down)); return 0; }
    return d2h_ring(c, (const uint8_t *) S.diff_ev.p, total * sizeof(uint32_t), nullptr, nullptr, nullptr, 0, dst,
                    sj.mt.copy_threads ? (int) sj.mt.copy_threads : c.copy_threads, []() { return 0; });
}

// ---- collector: one unit [off, off + m) of the slice, once `done` has fired ------------------------------------------------
int collect(LrmHostCtx &c, SliceJob &sj, size_t g) {
    const MapJob &j = sj.j;
    Slot &S = *sj.slot;
    DevSlot *const d = S.dev;
    const Range &u = sj.units[g];
    hipEvent_t done = sj.seed_only ? S.ev_seed[sj.ends[g] - 1] : S.ev_ext[g];
    const double t_in = sj.clk.ms();
    if (wait_event(done)) return -1;
    const double t_done = sj.clk.ms();
    if (take_errors(S)) return -2;                                   // raised by this or an earlier unit: never lost
    const uint64_t m = u.m, o = u.off, dstride = sj.dstride;
    // small arrays: device -> this unit's region of the pinned staging -> the caller's arrays
    uint8_t *hs = (uint8_t *) S.h_small.p + o * sj.stage_row;
    auto staged = [&](int a) { return hs + m * sj.arr[a].stage; };
    for (int a = 0; a < N_SMALL; ++a) {
        const SliceArray &A = sj.arr[a];
        if (A.down) HIPCHK(hipMemcpyAsync(staged(a), (const uint8_t *) d[a].p + o * A.elem, m * A.elem, hipMemcpyDeviceToHost, c.down));
    }
    HIPCHK(hipEventRecord(c.ev_small, c.down));
    if (wait_event(c.ev_small)) return -1;
    for (int a = 0; a < N_SMALL; ++a) {
        const SliceArray &A = sj.arr[a];
        if (A.down && A.host) memcpy((uint8_t *) A.host + o * A.elem, staged(a), m * A.elem);
    }
    if (!(j.mode & DO_EXTEND)) return 0;
    if (sj.want_diff && collect_diff(c, sj, u, (const lrm_aln_summary *) staged(A_SUMMARY), (uint64_t *) (hs + m * sj.stage_diff))) return -1;
    const int32_t *h_nops = (const int32_t *) staged(A_NOPS), *h_score = (const int32_t *) staged(A_SCORE), *h_mr = (const int32_t *) staged(A_MR);
    const lrm_seq_meta *h_meta = (const lrm_seq_meta *) staged(A_META);
    const uint32_t *h_tlen = (const uint32_t *) staged(A_TLEN);       // (read with cigar_text only)
    uint64_t *h_off = (uint64_t *) (hs + m * sj.stage_off);          // 2 x m offsets into the dense image ...
    uint32_t *h_len = (uint32_t *) (hs + m * sj.stage_len);          // ... and lengths: the op rows, then the reads
    const bool text = sj.text;

    // Dense image of the unit on the device: the used part of every CIGAR row, then the reads that were
    // reverse-complemented in place (alnmain.c:437; the other rows of reads_buf did not change).  Everything crosses
    // the link by DMA (hipMemcpyAsync): a hand-written kernel that writes the caller's pinned memory runs at the link
    // rate on an idle chip and at 2-9 GB/s once the compute kernels of the batches in flight own the wave slots, stream
    // priority or not, while the DMA keeps 50-57 GB/s (tools/d2h_under_load.hip, profiles/r3/probes).
    uint8_t *h_store = j.store_mem + o * j.store_stride;
    const bool pin_store = is_pinned(h_store);
    const bool dense = sj.mt.dense != 0;
    const int copy_threads = sj.mt.copy_threads ? (int) sj.mt.copy_threads : c.copy_threads;
    uint64_t total_ops = 0, total = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const uint64_t cap = j.store_stride;
        if (text) h_len[i] = h_tlen[i] + 1u;                                  // the text and its NUL
        else h_len[i] = h_nops[i] > 0 ? (uint32_t) ((uint64_t) h_nops[i] < cap ? (uint64_t) h_nops[i] : cap) : 0u;
        h_off[i] = total_ops;
        total_ops += ((uint64_t) h_len[i] + 15) & ~15ull;
    }
    if (text && total_ops > m * j.store_stride) {
        lrm_set_error("run-length CIGAR text of a group (%llu bytes) does not fit the %llu bytes of its rows in store_mem",
                      (unsigned long long) total_ops, (unsigned long long) (m * j.store_stride));
        return -3;
    }
    total = total_ops;
    uint64_t n_rev = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const bool rev = !sj.mt.keep_reads && h_mr[i] != 0 && h_meta[i].strand == 1;   // (keep_reads: the caller's buffer stays as it is)
        h_len[m + i] = rev ? j.lens[o + i] : 0u;
        h_off[m + i] = total;
        total += ((uint64_t) h_len[m + i] + 15) & ~15ull;
        n_rev += rev;
    }
    const int b = (int) (g & 1);
    if (S.dense_used[b] && wait_event(S.ev_dense[b])) return -1;     // the transfer two units ago has left the buffer
    const uint8_t *d_store = (const uint8_t *) d[A_STORE].p + o * dstride, *d_reads = (const uint8_t *) d[A_READS].p + o * j.stride;
    uint64_t *d_off = (uint64_t *) S.offs[b].p;
    uint32_t *d_len = (uint32_t *) ((uint8_t *) S.offs[b].p + 2 * m * 8);
    uint8_t *dn = (uint8_t *) S.dense[b].p;
    if (total) {
        HIPCHK(hipMemcpyAsync(d_len, h_len, 2 * m * 4, hipMemcpyHostToDevice, c.down));
        HIPCHK(hipMemcpyAsync(d_off, h_off, 2 * m * 8, hipMemcpyHostToDevice, c.down));
        if (n_rev && lrm_launch_pack_rows(d_reads, j.stride, j.stride, d_len + m, d_off + m, dn, m, c.down)) return -1;
        if (total_ops && text) {
            if (lrm_launch_cigar_text(d_store, dstride, (const int32_t *) d[A_NOPS].p + o, (const int32_t *) d[A_SCORE].p + o,
                                      (const int32_t *) d[A_MR].p + o, nullptr, d_off, dn, m, c.down)) return -1;
        } else if (total_ops && lrm_launch_pack_rows(d_store, dstride, j.store_stride, d_len, d_off, dn, m, c.down)) return -1;
        std::vector<uint8_t *> dst(2 * m);
        for (uint64_t i = 0; i < m; ++i) {
            dst[i] = j.store_mem + (o + i) * j.store_stride;
            dst[m + i] = (uint8_t *) j.reads + (o + i) * j.stride;
        }
        if (dense) {
            // The reverse-complemented reads are the only rows the host has to place: through the chunk ring, copied by
            // this thread alone.  Then the op bytes: ONE DMA straight into the region of the caller's pinned store_mem
            // the unit's rows would occupy (sum of the 16-aligned lengths <= m * store_stride because
            // store_stride % 16 == 0) -- it flies while this thread goes on to the next unit.
            // The ring is deep enough (N_RING chunks) for every piece of a unit's reads to be handed to the DMA engine before
            // the first is drained, so the op bytes follow right behind them on the same stream and fly while this thread
            // places the reads.  (With four chunks the op bytes waited until the collector had copied nearly all of
            // the reads through them: 48 ms per batch on a box with a slow host memcpy against 32 with keep_reads, whose op
            // bytes leave at once; the op bytes on a second stream next to the ring: 38-40 ms -- two blit copies at a time
            // share the link badly; helper threads for the placement: no difference.)
            auto ops_dma = [&]() -> int {
                if (total_ops && pin_store) HIPCHK(hipMemcpyAsync(h_store, dn, total_ops, hipMemcpyDeviceToHost, c.down));
                return 0;
            };
            std::vector<uint64_t> roff(m);
            for (uint64_t i = 0; i < m; ++i) roff[i] = h_off[m + i] - total_ops;
            if (d2h_ring(c, dn + total_ops, total - total_ops, roff.data(), h_len + m, dst.data() + m, m, nullptr, 1, ops_dma)) return -1;
            if (total_ops && !pin_store && d2h_ring(c, dn, total_ops, nullptr, nullptr, nullptr, 0, h_store, copy_threads, []() { return 0; })) return -1;
        } else {
            // row layout (alnmain.c:322-325): every used CIGAR row and every reverse-complemented read is placed by the
            // host's memcpy team
            if (d2h_ring(c, dn, total, h_off, h_len, dst.data(), 2 * m, nullptr, copy_threads, []() { return 0; })) return -1;
        }
        HIPCHK(hipEventRecord(S.ev_dense[b], c.down));
        S.dense_used[b] = true;
    }
    for (uint64_t i = 0; i < m; ++i) {                               // alnmain.c:322-325, mutils.c:99-104
        j.cig[o + i].cigar = dense ? h_store + h_off[i] : j.store_mem + (o + i) * j.store_stride;
        j.cig[o + i].n_cigar_op = h_nops[i];
        j.cig[o + i].score = h_score[i];
    }
    if (sj.clk.on) fprintf(stderr, "[lrm host] collect off=%llu m=%llu: wait-from %.1f kernels-done %.1f issued %.1f ms (%s, %.0f MB)\n",
                           (unsigned long long) o, (unsigned long long) m, t_in, t_done, sj.clk.ms(), dense ? (pin_store ? "dense, DMA into store_mem" : "dense, staged") : "rows", total / 1e6);
    return 0;
}

void issuer_main(LrmHostCtx *cp) {
    LrmHostCtx &c = *cp;
    if (hipSetDevice(c.idx->device) != hipSuccess) { (void) hipGetLastError(); }
    for (;;) {
        std::unique_ptr<SliceJob> job;
        Slot *slot = nullptr;
        {
            std::unique_lock<std::mutex> lk(c.mu);
            c.cv.wait(lk, [&] {
                if (c.stop) return true;
                if (c.q_issue.empty()) return false;
                for (int k = 0; k < c.n_slots; ++k) if (!c.slots[k].busy) return true;
                return false;
            });
            if (c.stop && c.q_issue.empty()) return;
            if (c.q_issue.empty()) continue;
            for (int k = 0; k < c.n_slots; ++k) if (!c.slots[k].busy) { slot = &c.slots[k]; break; }
            if (!slot) continue;
            slot->busy = true;
            job = std::move(c.q_issue.front());
            c.q_issue.pop_front();
            job->busy = c.n_active > 1;
        }
        SliceJob *sj = job.get();
        sj->slot = slot;
        sj->clk.on = sj->mt.verbose != 0;
        {   // the collector follows the slice from now on
            std::lock_guard<std::mutex> lk(c.mu);
            c.q_collect.push_back(std::move(job));
        }
        c.cv.notify_all();
        int rc;
        try { rc = plan_and_issue(c, *sj); }
        catch (const std::exception &e) { lrm_set_error("issuer thread: %s", e.what()); rc = -1; }
        if (rc) sj->fail(rc);
        {   // (notified under the lock: the collector deletes the slice once it has seen issue_done)
            std::lock_guard<std::mutex> lk(sj->m);
            sj->issue_done = true;
            sj->cv.notify_all();
        }
    }
}

void collector_main(LrmHostCtx *cp) {
    LrmHostCtx &c = *cp;
    if (hipSetDevice(c.idx->device) != hipSuccess) { (void) hipGetLastError(); }
    for (;;) {
        std::unique_ptr<SliceJob> job;
        {
            std::unique_lock<std::mutex> lk(c.mu);
            c.cv.wait(lk, [&] { return c.stop || !c.q_collect.empty(); });
            if (c.q_collect.empty()) { if (c.stop) return; continue; }
            job = std::move(c.q_collect.front());
            c.q_collect.pop_front();
        }
        SliceJob &sj = *job;
        Slot &S = *sj.slot;
        for (size_t g = 0;; ++g) {
            {
                std::unique_lock<std::mutex> lk(sj.m);
                sj.cv.wait(lk, [&] { return sj.issued > g || sj.issue_done || sj.rc; });
                if (sj.rc || sj.issued <= g) break;                       // failed, or every unit has been collected
            }
            int rc;
            try { rc = collect(c, sj, g); }
            catch (const std::exception &e) { lrm_set_error("collector thread: %s", e.what()); rc = -1; }
            if (rc) { sj.fail(rc); break; }
        }
        { std::unique_lock<std::mutex> lk(sj.m); sj.cv.wait(lk, [&] { return sj.issue_done; }); }
        int rc = sj.rc;
        std::string err = sj.err;
        if (!rc) {
            // the last transfers into the caller's memory (DMA and device row writes are ordered on the download stream)
            if (hipEventRecord(c.ev_tail, c.down) != hipSuccess || wait_event(c.ev_tail)) { rc = -1; err = lrm_last_error(); }
        }
        if (rc) {                                                        // error path: let everything issued for this slot drain
            c.drain();
            (void) take_errors(S);                                        // reported now: do not fail the next batch
        }
        if (sj.clk.on)
            fprintf(stderr, "[lrm host] slice of %llu reads, %zu seed sub-batches, %zu units: %.1f ms (collector thread CPU so far %.1f ms)\n", (unsigned long long) sj.j.n,
                    sj.subs.size(), sj.units.size(), sj.clk.ms(), thread_cpu_ms());
        lrm_ticket *t = sj.ticket;
        job.reset();
        {
            std::lock_guard<std::mutex> lk(c.mu);
            S.busy = false;
            --c.n_active;
        }
        c.cv.notify_all();
        t->part_done(rc, err);
    }
}

std::mutex g_host_ctx_init;             // creation of a handle's host context (the context's own mutex lives inside it)

}  // namespace

int lrm_host_ensure_ctx(lrm_index *idx, int group_size) {
    if (lrm_require_device(idx->device)) return -1;
    std::lock_guard<std::mutex> g(g_host_ctx_init);
    if (!idx->host) {
        idx->host = new (std::nothrow) LrmHostCtx;
        if (!idx->host) { lrm_set_error("out of memory"); return -1; }
        idx->host->idx = idx;
    }
    LrmHostCtx &c = *idx->host;
    if (ctx_init(c)) return -1;
    // the memcpy team of the pageable paths: a library must not fan out over every core of its host, and the
    // replicas of a group share the host's CPU share
    int ct = lrm_host_threads() / (group_size > 0 ? group_size : 1);
    c.copy_threads = ct < 1 ? 1 : (ct > 8 ? 8 : ct);
    { long long v; if (idx->env.get("LRM_HOST_SLOTS", &v) && v >= 1 && v <= N_SLOTS) c.n_slots = (int) v; }
    if (!c.threads_up) {
        try {
            c.issuer = std::thread(issuer_main, &c);
            try { c.collector = std::thread(collector_main, &c); }
            catch (...) {
                { std::lock_guard<std::mutex> lk(c.mu); c.stop = true; }
                c.cv.notify_all();
                c.issuer.join();
                c.stop = false;
                throw;
            }
        } catch (const std::exception &e) {
            lrm_set_error("cannot start the host pipeline threads: %s", e.what());
            return -1;
        }
        c.threads_up = true;
    }
    return 0;
}

// The owners of LrmHostCtx release everything; what stays by hand is the order: batches in flight run to completion, the
// threads end, every stream drains, and only then is anything freed.
void lrm_host_ctx_free(lrm_index *idx) {
    LrmHostCtx *c = idx->host;
    if (!c) return;
    idx->host = nullptr;
    if (c->threads_up) {
        {   // batches still queued or in flight run to completion first (their tickets stay valid)
            std::unique_lock<std::mutex> lk(c->mu);
            c->cv.wait(lk, [&] { return c->n_active == 0; });
            c->stop = true;
        }
        c->cv.notify_all();
        c->issuer.join();
        c->collector.join();
    }
    if (c->ready) c->drain();
    delete c;
}
