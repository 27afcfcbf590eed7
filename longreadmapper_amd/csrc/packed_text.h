// packed_text.h -- what the index builder's files share (suffix_sort.cpp, index_build.cpp): the 2-bit image of the text,
// the block ranges of their parallel loops, the internal entry of the suffix sorter, the builder's environment knobs.
// Everything but sa_build is inline: it sits in the hot loops of both files.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <omp.h>
#include "lrm_internal.h"

// ---- the builder's knobs: environment only, for tuning sessions and tests; read once per lrm_sa_build / lrm_host_index_build
// call; the suffix array and the tables never depend on them -----------------------------------------------------------------
//   LRM_SA_ALGO=sais          the linear-time SA-IS sorts every text
//   LRM_SA_ALGO=bucket        the parallel bucket sorter without its tie budget (it never gives up a repetitive text; a text with
//                             bytes other than upper-case ACGT still goes to SA-IS)
//   LRM_SA_SCRATCH_ROWS=n     rows of the bucket sorter's scratch instead of L/6 + 2^20 (n >= 1024; never less than the largest
//                             bucket): tests make the buckets go through many groups with it
//   LRM_BUILD_VERBOSE=1       stage times of the builder on stderr
struct BuildKnobs { bool force_sais, force_bucket, verbose; uint64_t scratch_rows; };      // scratch_rows 0: automatic
static inline BuildKnobs build_knobs() {
    const char *algo = getenv("LRM_SA_ALGO"), *rows = getenv("LRM_SA_SCRATCH_ROWS");
    const long long v = rows ? atoll(rows) : 0;
    return {algo && !strcmp(algo, "sais"), algo && !strcmp(algo, "bucket"), getenv("LRM_BUILD_VERBOSE") != nullptr,
            v >= 1024 ? (uint64_t) v : 0};
}
struct LRM_LOCAL StageTimer {
    double t0; bool on;
    explicit StageTimer(bool on_) : t0(omp_get_wtime()), on(on_) {}
    void lap(const char *what) { if (on) { const double t = omp_get_wtime(); fprintf(stderr, "[lrm build] %-28s %8.2f s\n", what, t - t0); t0 = t; } }
};

// block i of [0, n) cut into blocks of B elements
struct BlockRange { uint64_t lo, hi; };
static inline uint64_t block_count(uint64_t n, uint64_t B) { return (n + B - 1) / B; }
static inline BlockRange block_range(uint64_t i, uint64_t B, uint64_t n) { const uint64_t lo = i * B; return {lo, lo + B < n ? lo + B : n}; }

// The text at 2 bits per base, first base most significant, so that the integer order of a 64-bit window is the lexicographic
// order of 32 bases; positions past the last base read as 'A' (0).
struct LRM_LOCAL PackedText {
    std::vector<uint64_t> w;      // 32 bases per word, first base in bits 63..62
    uint64_t n = 0;               // bases (text length without '$')
    inline uint64_t base(uint64_t p) const { return (w[p >> 5] >> (62 - 2 * (p & 31))) & 3ull; }
    inline uint64_t window(uint64_t p) const {             // bases p .. p+31, zero padded
        const uint64_t i = p >> 5, sh = (p & 31) * 2;
        const uint64_t a = w[i], b = w[i + 1];
        return sh ? ((a << sh) | (b >> (64 - sh))) : a;
    }
    inline uint64_t roll(uint64_t win, uint64_t p) const { return (win << 2) | base(p + 32); }   // window(p) -> window(p + 1)
};

// f(p, window(p)) for p = lo .. hi-1, one shift and one base per step
template <typename F>
static inline void for_each_window(const PackedText &t, uint64_t lo, uint64_t hi, F f) {
    uint64_t win = t.window(lo);
    for (uint64_t p = lo; p < hi; ++p) { f(p, win); win = t.roll(win, p); }
}

// 2-bit image of text[0 .. L-1) (the '$' at L-1 is not part of it); false if the text holds a byte other than
// upper-case ACGT (such texts take the generic paths and never read the image)
static inline bool pack_text(const char *text, uint64_t L, PackedText &t) {
    const uint64_t n = L - 1;
    t.n = n;
    t.w.assign(n / 32 + 4, 0);
    int bad = 0;
    const uint64_t nwords = block_count(n, 32);
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static) reduction(| : bad)
    for (uint64_t wi = 0; wi < nwords; ++wi) {
        uint64_t v = 0;
        const BlockRange r = block_range(wi, 32, n);
        for (uint64_t i = r.lo; i < r.hi; ++i) {
            const int c = base_code(text[i]);
            if (c < 0) bad = 1;
            v |= (uint64_t) (c & 3) << (62 - 2 * (i - r.lo));
        }
        t.w[wi] = v;
    }
    return !bad;
}

// suffix_sort.cpp: the suffix array of text[0 .. L) into out, after the checks of lrm_sa_build ('$' last and nowhere else).
// packed: the 2-bit image of a text of upper-case ACGT (the parallel sorter runs on it); null: SA-IS
LRM_LOCAL int sa_build(const char *text, uint64_t L, const PackedText *packed, const BuildKnobs &knobs, lrm_ui40 *out);
