// host_pipeline.h -- what the host-buffer entry points (lrm_host.hip) and the pipeline behind them (host_pipeline.hip)
// share: a batch as the caller handed it over (MapJob), its slices (SliceJob), the per-handle context (LrmHostCtx)
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "lrm_hip_util.h"
#include "extend_stage.h"

// completion of one submitted batch: `pending` slices (over all replicas) still to be collected
struct lrm_ticket {
    std::mutex m;
    std::condition_variable cv;
    int pending = 0;
    int rc = 0;
    std::string err;
    std::atomic<uint64_t> diff_total{0};     // difference events: every extension group adds its events and takes what was there as its base
    uint64_t *diff_needed_out = nullptr;     // ... and the wait writes the batch's total here
    void part_done(int code, const std::string &msg) {
        std::lock_guard<std::mutex> g(m);
        if (code && !rc) { rc = code; err = msg; }
        --pending;
        cv.notify_all();
    }
};

struct HostClock {
    bool on = false;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// ---- owners: every device object of the context releases itself (the streams have been drained by then: lrm_host_ctx_free) ----
template <typename T, hipError_t (*DESTROY)(T)>
struct Owned {                                     // a HIP handle or pinned block
    T h = nullptr;
    Owned() = default;
    Owned(Owned &&o) : h(o.h) { o.h = nullptr; }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { if (h) (void) DESTROY(h); }
    operator T() const { return h; }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Pinned = Owned<void *, hipHostFree>;
template <bool PINNED>
struct GrowBuf {                                   // device (or pinned host) memory that only grows
    void *p = nullptr; uint64_t cap = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    ~GrowBuf() { release(); }
    void release() { if (p) (void) (PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
    int ensure(uint64_t bytes) {
        if (bytes <= cap) return 0;
        release();
        if ((PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes)) != hipSuccess) { (void) hipGetLastError(); p = nullptr; return -1; }
        cap = bytes;
        return 0;
    }
};
using DevSlot = GrowBuf<false>;
using PinSlot = GrowBuf<true>;
struct WsFree { void operator()(lrm_workspace *ws) const { lrm_workspace_free(ws); } };
using WsPtr = std::unique_ptr<lrm_workspace, WsFree>;

constexpr uint64_t STAGE_CHUNK = 32ull << 20;      // pinned chunks of the pageable upload staging
constexpr uint64_t RING_CHUNK = 16ull << 20;       // ... and of the download ring
constexpr int N_RING = 16;          // 256 MiB of pinned chunks per replica: a unit's reverse-complemented reads (0.25 GB) fit whole
constexpr int N_SEED_STREAMS = 3;
constexpr int N_EXT_STREAMS = 4;
constexpr int N_SLOTS = 3;            // upper bound on the batches (slices) in flight per replica; n_slots of them are used

// ---- a batch as the entry points hand it to the pipeline -------------------------------------------------------------------
enum { DO_SEED = 1, DO_EXTEND = 2 };
struct MapJob {
    int mode;
    char *reads; uint64_t stride; const uint32_t *lens; uint64_t n;
    lrm_params p; lrm_gact_params gp;
    const lrm_entry *best_in; lrm_entry *best_out;
    lrm_cigar *cig; uint8_t *store_mem; uint64_t store_stride; int *score; lrm_seq_meta *meta; int *meta_r;
    lrm_anchor *anchor_out;           // anchored mode: the anchor records too (null: they stay in the workspace)
    lrm_mapq *mapq_out;               // mapping quality: the stage runs behind every seed sub-batch, the records come down with the small arrays (null: no stage)
    lrm_aln_summary *summary_out;     // alignment summary: the stage runs behind every group's extension, the records come down likewise (null: no stage)
    // difference events (lrm_batch_diff): per read where its events are and how many (null: no stage); the event buffer and
    // its room are the batch's, shared by every slice
    uint64_t *diff_off; uint32_t *diff_cnt; uint32_t *diff_events; uint64_t diff_cap;
    // pileup (lrm_batch_pileup): the accumulator of the replica this job runs on -- every slice of the replica's share adds to
    // it behind its groups' extension -- and the MAPQ a read needs to be counted (null: no stage)
    lrm_pileup *pile; uint32_t pile_min_mapq;
    MapJob slice(uint64_t o, uint64_t m) const {        // reads [o, o + m): every array of the caller moves on by o elements
        MapJob j = *this;
        j.n = m;
        auto adv = [o](auto *&ptr, uint64_t pitch = 1) { if (ptr) ptr += o * pitch; };
        adv(j.reads, stride); adv(j.lens); adv(j.best_in); adv(j.best_out); adv(j.anchor_out); adv(j.mapq_out); adv(j.summary_out); adv(j.diff_off); adv(j.diff_cnt);
        adv(j.cig); adv(j.store_mem, store_stride); adv(j.score); adv(j.meta); adv(j.meta_r);
        return j;
    }
};

// The per-read arrays of a slice on the device.  The first N_SMALL come down with every unit through the pinned staging of
// the slot, in this order on the download stream; the others are uploaded (reads, lens) or leave as the dense image (store).
enum { A_BEST, A_NOPS, A_SCORE, A_META, A_MR, A_TLEN, A_ANCHOR, A_MAPQ, A_SUMMARY, N_SMALL, A_READS = N_SMALL, A_LENS, A_STORE, N_ARRAYS };
struct SliceArray {
    uint64_t elem;                    // bytes per read
    bool on_dev;                      // the slice needs the device mirror
    bool down;                        // every unit downloads its part ...
    void *host;                       // ... into this array of the caller (null: the collector alone reads it)
    uint64_t stage;                   // where the part starts in a unit's pinned staging, in bytes per read of the unit
};
static_assert(alignof(lrm_entry) <= 8 && alignof(lrm_seq_meta) <= 8 && alignof(lrm_anchor) <= 8 && alignof(lrm_mapq) <= 8 &&
              alignof(lrm_aln_summary) <= 8 && sizeof(lrm_mapq) % 4 == 0, "SliceJob::plan_arrays places an array of 8-byte multiples at a multiple of 8, any other at a multiple of 4");

// device-side resources of one slice in flight
struct Slot {
    WsPtr ws_seed[N_SEED_STREAMS];                 // seed-stage scratch, one per seed stream (sub-batch sized)
    WsPtr ws_ext[N_EXT_STREAMS];                   // extension scratch (group sized), one per extension stream
    DevSlot dev[N_ARRAYS];                         // device mirrors of the caller's arrays
    DevSlot dense[2], offs[2];                     // dense result image + offset table, alternating over the groups
    DevSlot diff_ev, diff_off;                     // difference events of a group and their offsets (the download stream runs group after group)
    Event ev_dense[2];                             // the last transfer out of dense[b] has drained
    bool dense_used[2] = {false, false};
    PinSlot h_small;                               // pinned staging of the small result arrays and offset tables (SliceJob::stage_row bytes per read)
    std::vector<Event> ev_up, ev_seed, ev_ext;     // per sub-batch / per extension group, grown on demand
    bool busy = false;
};

struct Range { uint64_t off, m; };

// one slice of a submitted batch on one replica, from the issuer's queue to its collection
struct SliceJob {
    MapJob j;
    LrmMapTune mt;
    lrm_ticket *ticket = nullptr;
    uint32_t max_len = 0;
    Slot *slot = nullptr;
    bool busy = false;                // another slice was queued or in flight when this one was issued
    // plan (made by the issuer)
    std::vector<Range> subs, units;
    std::vector<size_t> ends, unit_of;
    uint64_t dstride = 0;
    bool seed_only = false;
    bool want_anchor = false, want_mapq = false, want_summary = false, text = false;     // the anchor, mapping-quality and summary records, run-length CIGAR text
    bool want_diff = false;                                          // the difference events (they need the summary records on the host)
    uint64_t stage_diff = 0;                                         // staging of a unit's event offsets (m + 1 x u64)
    SliceArray arr[N_ARRAYS] = {};
    uint64_t stage_off = 0, stage_len = 0, stage_row = 0;           // staging of a unit's offset table (2 x u64) and lengths (2 x u32); bytes per read in all
    void plan_arrays();
    HostClock clk;
    // issuer -> collector hand-off
    std::mutex m;
    std::condition_variable cv;
    uint64_t issued = 0;              // units handed to the device
    bool issue_done = false;
    int rc = 0;
    std::string err;
    std::atomic<bool> failed{false};
    void fail(int code) {
        std::lock_guard<std::mutex> g(m);
        if (!rc) { rc = code; err = lrm_last_error(); }
        failed.store(true);
        cv.notify_all();
    }
};

struct LrmHostCtx {
    lrm_index *idx = nullptr;
    int copy_threads = 4;                // memcpy team of the pageable paths (staging upload, result scatter)
    int n_slots = 2;                     // slices in flight (LRM_HOST_SLOTS)
    // --- queues (mu) ---
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::unique_ptr<SliceJob>> q_issue, q_collect;
    bool stop = false;
    int n_active = 0;                    // slices queued or in flight (lrm_host_ctx_free drains them)
    std::thread issuer, collector;
    bool threads_up = false;
    // --- device objects (destroyed in reverse order: the slots and their workspaces go before the streams) ---
    Stream up, down, seed[N_SEED_STREAMS], ext[N_EXT_STREAMS];
    Slot slots[N_SLOTS];
    // issuer only: staging of pageable uploads
    Pinned pin_up[2];
    Event ev_pin_up[2];
    bool pin_up_used[2] = {false, false};
    uint64_t up_seq = 0;
    // collector only: chunks of the scatter path, event of the small copies
    Pinned pin_dn[N_RING];
    Event ev_pin_dn[N_RING];
    Event ev_small, ev_tail;
    bool ready = false;
    void drain();                        // every stream runs dry
};

// creates the context of a replica on its first batch and starts its two threads; group_size: replicas sharing the host's CPUs
int lrm_host_ensure_ctx(lrm_index *idx, int group_size);
