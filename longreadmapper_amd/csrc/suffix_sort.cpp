// suffix_sort.cpp -- the suffix sorters of the index builder: lrm_sa_build (include/lrm_index_host.h) and its internal
// entry sa_build (packed_text.h).  A parallel bucket sorter for texts of upper-case ACGT, the linear-time SA-IS for every
// other text and for texts too repetitive for the first.  The suffix array of a text that ends in a unique minimal '$' is
// unique, so either reproduces the reference's .sa5 byte for byte (it uses the vendored pSAscan, psascan/sa_use.cc:8-18).
#include <algorithm>
#include "../../include/lrm_index_host.h"
#include "packed_text.h"

// ------------------------------------------------------------------------------------------
// SA-IS (Nong, Zhang, Chan: "Two efficient algorithms for linear time suffix array
// construction").  s[n-1] must be the unique smallest symbol.
// ------------------------------------------------------------------------------------------
namespace {

template <typename I>
struct SaIs {
    static inline bool tget(const uint8_t *t, I i) { return (t[i >> 3] >> (i & 7)) & 1; }
    static inline void tset(uint8_t *t, I i, bool b) {
        if (b) t[i >> 3] |= (uint8_t) (1u << (i & 7)); else t[i >> 3] &= (uint8_t) ~(1u << (i & 7));
    }
    static inline bool is_lms(const uint8_t *t, I i) { return i > 0 && tget(t, i) && !tget(t, i - 1); }

    template <typename C>
    static void buckets(const C *s, I *bkt, I n, I K, bool end) {
        for (I i = 0; i <= K; ++i) bkt[i] = 0;
        for (I i = 0; i < n; ++i) bkt[(I) s[i]]++;
        I sum = 0;
        for (I i = 0; i <= K; ++i) { sum += bkt[i]; bkt[i] = end ? sum : sum - bkt[i]; }
    }
    template <typename C>
    static void induce_l(const uint8_t *t, I *SA, const C *s, I *bkt, I n, I K) {
        buckets(s, bkt, n, K, false);
        for (I i = 0; i < n; ++i) {
            I j = SA[i] - 1;
            if (SA[i] > 0 && !tget(t, j)) SA[bkt[(I) s[j]]++] = j;
        }
    }
    template <typename C>
    static void induce_s(const uint8_t *t, I *SA, const C *s, I *bkt, I n, I K) {
        buckets(s, bkt, n, K, true);
        for (I i = n - 1; i >= 0; --i) {
            I j = SA[i] - 1;
            if (SA[i] > 0 && tget(t, j)) SA[--bkt[(I) s[j]]] = j;
        }
    }

    template <typename C>
    static void run(const C *s, I *SA, I n, I K) {
        if (n == 1) { SA[0] = 0; return; }
        std::vector<uint8_t> tv((size_t) n / 8 + 1, 0);
        uint8_t *t = tv.data();
        tset(t, n - 2, false);
        tset(t, n - 1, true);
        for (I i = n - 3; i >= 0; --i)
            tset(t, i, s[i] < s[i + 1] || (s[i] == s[i + 1] && tget(t, i + 1)));
        std::vector<I> bv((size_t) K + 1);
        I *bkt = bv.data();
        // stage 1: sort the LMS substrings
        buckets(s, bkt, n, K, true);
        for (I i = 0; i < n; ++i) SA[i] = -1;
        for (I i = 1; i < n; ++i)
            if (is_lms(t, i)) SA[--bkt[(I) s[i]]] = i;
        induce_l(t, SA, s, bkt, n, K);
        induce_s(t, SA, s, bkt, n, K);
        I n1 = 0;
        for (I i = 0; i < n; ++i)
            if (is_lms(t, SA[i])) SA[n1++] = SA[i];
        for (I i = n1; i < n; ++i) SA[i] = -1;
        I name = 0, prev = -1;
        for (I i = 0; i < n1; ++i) {
            I pos = SA[i];
            bool diff = false;
            for (I d = 0; d < n; ++d) {
                if (prev == -1 || s[pos + d] != s[prev + d] || tget(t, pos + d) != tget(t, prev + d)) { diff = true; break; }
                else if (d > 0 && (is_lms(t, pos + d) || is_lms(t, prev + d))) break;
            }
            if (diff) { name++; prev = pos; }
            SA[n1 + pos / 2] = name - 1;
        }
        for (I i = n - 1, j = n - 1; i >= n1; --i)
            if (SA[i] >= 0) SA[j--] = SA[i];
        // stage 2: solve the reduced problem
        I *SA1 = SA, *s1 = SA + n - n1;
        if (name < n1) run<I>(s1, SA1, n1, name - 1);
        else for (I i = 0; i < n1; ++i) SA1[s1[i]] = i;
        // stage 3: induce the final order
        buckets(s, bkt, n, K, true);
        for (I i = 1, j = 0; i < n; ++i)
            if (is_lms(t, i)) s1[j++] = i;
        for (I i = 0; i < n1; ++i) SA1[i] = s1[SA1[i]];
        for (I i = n1; i < n; ++i) SA[i] = -1;
        for (I i = n1 - 1; i >= 0; --i) {
            I j = SA[i];
            SA[i] = -1;
            SA[--bkt[(I) s[j]]] = j;
        }
        induce_l(t, SA, s, bkt, n, K);
        induce_s(t, SA, s, bkt, n, K);
    }
};

}  // namespace

// ------------------------------------------------------------------------------------------
// Parallel suffix sorter for nucleotide texts (the builder GRCh38-sized references need: 6.2 G rows in
// minutes on the host cores next to the GPU; the reference uses the parallel external-memory pSAscan,
// psascan/sa_use.cc:8-18, asindex.c:138).  The suffix array of a text that ends in a unique minimal '$' is
// unique, so any correct sorter reproduces the reference's .sa5 byte for byte.
//
//   1. the text is packed to 2 bits per base, first base most significant, so that the integer order of a
//      64-bit window is the lexicographic order of 32 bases; positions past the last base read as 'A' (0)
//   2. suffixes are distributed by their first PB bases into 4^PB buckets (histogram, prefix sums)
//   3. the buckets are processed in groups that fit a bounded scratch: one parallel scan of the text collects
//      {next 32 bases, position} of every suffix of the group, each bucket is sorted by that key in cache,
//      and only runs of equal keys (40+ common bases) are compared through the packed text
//   4. the sorted positions go straight into the caller's ui40 array (8-byte slots, padding zeroed)
// A suffix that runs into '$' compares as if padded with 'A' and loses ties to longer suffixes, which is the
// order '$' < 'A' gives.  Texts with very long exact repeats would make step 3 quadratic: the work spent on
// ties is counted and the build falls back to the linear-time SA-IS above when it exceeds a budget.
// ------------------------------------------------------------------------------------------
namespace {

struct KeyPos { uint64_t key, pos; };

// exact order of the suffixes at p and q, known to share their first d bases (padded semantics, see above)
static inline bool suffix_less(const PackedText &t, uint64_t p, uint64_t q, uint64_t d, uint64_t &work) {
    while (true) {
        const int64_t lp = (int64_t) t.n - (int64_t) (p + d), lq = (int64_t) t.n - (int64_t) (q + d);
        if (lp <= 0 || lq <= 0) return p > q;                        // the one that has reached '$' is smaller
        const uint64_t wp = t.window(p + d), wq = t.window(q + d);
        ++work;
        if (wp != wq) {
            const int64_t first = __builtin_clzll(wp ^ wq) >> 1, lmin = lp < lq ? lp : lq;
            if (first >= lmin) return p > q;                          // equal up to the shorter one's '$'
            return wp < wq;
        }
        d += 32;
    }
}

template <typename F>
static void sort_ties(KeyPos *a, uint64_t n, F less) {
    for (uint64_t i = 0; i < n;) {
        uint64_t j = i + 1;
        while (j < n && a[j].key == a[i].key) ++j;
        if (j - i > 1) std::sort(a + i, a + j, less);
        i = j;
    }
}

// top-bits distribution + std::sort of the pieces: ~3x fewer comparisons than std::sort alone on a 100 k-row bucket
static void sort_by_key(KeyPos *a, uint64_t m, std::vector<KeyPos> &tmp) {
    auto by_key = [](const KeyPos &x, const KeyPos &y) { return x.key < y.key; };
    if (m < 2048) { std::sort(a, a + m, by_key); return; }
    constexpr int RB = 11;
    uint32_t cnt[(1u << RB) + 1] = {0};
    for (uint64_t i = 0; i < m; ++i) cnt[(a[i].key >> (64 - RB)) + 1]++;
    for (uint32_t b = 0; b < (1u << RB); ++b) cnt[b + 1] += cnt[b];
    if (tmp.size() < m) tmp.resize(m);
    uint32_t cur[1u << RB];
    memcpy(cur, cnt, sizeof(cur));
    for (uint64_t i = 0; i < m; ++i) tmp[cur[a[i].key >> (64 - RB)]++] = a[i];
    memcpy(a, tmp.data(), m * sizeof(KeyPos));
    for (uint32_t b = 0; b < (1u << RB); ++b)
        if (cnt[b + 1] - cnt[b] > 1) std::sort(a + cnt[b], a + cnt[b + 1], by_key);
}

static int sa_build_bucketed(const PackedText &t, uint64_t L, lrm_ui40 *out, uint64_t tie_budget_per_row, const BuildKnobs &knobs) {
    const uint64_t n = L - 1;
    StageTimer tm(knobs.verbose);

    const int PB = L > (1ull << 26) ? 8 : (L > (1ull << 18) ? 5 : 2);     // bases of the distribution prefix
    const uint64_t NB = 1ull << (2 * PB);
    const int nth = lrm_host_threads();        // the team size of the region below (the caller's OpenMP limit may differ)
    // histogram of prefixes (per-thread, merged)
    std::vector<uint64_t> cnt(NB + 1, 0);
    {
        std::vector<std::vector<uint64_t>> local((size_t) nth, std::vector<uint64_t>(NB, 0));
#pragma omp parallel num_threads(nth)
        {
            std::vector<uint64_t> &h = local[(size_t) omp_get_thread_num()];
#pragma omp for schedule(static)
            for (uint64_t blk = 0; blk < block_count(n, 65536); ++blk) {
                const BlockRange r = block_range(blk, 65536, n);
                for_each_window(t, r.lo, r.hi, [&](uint64_t, uint64_t win) { h[win >> (64 - 2 * PB)]++; });
            }
        }
        for (int th = 0; th < nth; ++th) for (uint64_t bkt = 0; bkt < NB; ++bkt) cnt[bkt + 1] += local[(size_t) th][bkt];
    }
    for (uint64_t bkt = 0; bkt < NB; ++bkt) cnt[bkt + 1] += cnt[bkt];      // cnt[b] = suffixes in buckets < b
    tm.lap("sa: prefix histogram");
    ui40_put(out, n);                                                      // the suffix "$"

    // groups of consecutive buckets within the scratch bound
    uint64_t scratch_rows = knobs.scratch_rows ? knobs.scratch_rows : (L / 6) + (1ull << 20);
    uint64_t max_bucket = 0;
    for (uint64_t bkt = 0; bkt < NB; ++bkt) max_bucket = std::max(max_bucket, cnt[bkt + 1] - cnt[bkt]);
    if (scratch_rows < max_bucket) scratch_rows = max_bucket;
    KeyPos *scratch;
    if (!lrm_alloc(scratch, scratch_rows, "suffix sorter scratch")) return -1;
    std::vector<uint64_t> cursor(NB);
    uint64_t work_total = 0;
    const uint64_t budget = tie_budget_per_row * L + (1ull << 24);
    bool over = false;
    for (uint64_t g0 = 0; g0 < NB && !over;) {
        uint64_t g1 = g0 + 1;
        while (g1 < NB && cnt[g1 + 1] - cnt[g0] <= scratch_rows) ++g1;
        const uint64_t base = cnt[g0], rows = cnt[g1] - cnt[g0];
        if (rows == 0) { g0 = g1; continue; }
        for (uint64_t bkt = g0; bkt < g1; ++bkt) cursor[bkt] = cnt[bkt] - base;
        // collect {key, position} of the group's suffixes: threads reserve space in small batches
#pragma omp parallel num_threads(lrm_host_threads())
        {
            constexpr int LB = 8;
            std::vector<KeyPos> lbuf((size_t) (g1 - g0) * LB);
            std::vector<uint8_t> lcnt((size_t) (g1 - g0), 0);
            auto flush = [&](uint64_t bkt) {
                const uint64_t k = bkt - g0;
                const uint8_t m = lcnt[k];
                if (!m) return;
                uint64_t at;
#pragma omp atomic capture
                { at = cursor[bkt]; cursor[bkt] += m; }
                memcpy(scratch + at, &lbuf[k * LB], (size_t) m * sizeof(KeyPos));
                lcnt[k] = 0;
            };
#pragma omp for schedule(dynamic, 4) nowait
            for (uint64_t blk = 0; blk < block_count(n, 262144); ++blk) {
                const BlockRange r = block_range(blk, 262144, n);
                for_each_window(t, r.lo, r.hi, [&](uint64_t p, uint64_t win) {
                    const uint64_t bkt = win >> (64 - 2 * PB);
                    if (bkt < g0 || bkt >= g1) return;
                    const uint64_t k = bkt - g0;
                    lbuf[k * LB + lcnt[k]] = KeyPos{t.window(p + (uint64_t) PB), p};
                    if (++lcnt[k] == LB) flush(bkt);
                });
            }
            for (uint64_t bkt = g0; bkt < g1; ++bkt) flush(bkt);
        }
        tm.lap("sa: collect group");
        // sort every bucket: by key in cache, ties through the text
        uint64_t work = 0;
#pragma omp parallel num_threads(lrm_host_threads()) reduction(+ : work)
        {
        std::vector<KeyPos> tmp;
#pragma omp for schedule(dynamic, 1)
        for (uint64_t bkt = g0; bkt < g1; ++bkt) {
            KeyPos *a = scratch + (cnt[bkt] - base);
            const uint64_t m = cnt[bkt + 1] - cnt[bkt];
            if (m == 0) continue;
            sort_by_key(a, m, tmp);
            uint64_t wk = 0;
            sort_ties(a, m, [&](const KeyPos &x, const KeyPos &y) { return suffix_less(t, x.pos, y.pos, (uint64_t) PB + 32, wk); });
            work += wk;
            lrm_ui40 *dst = out + 1 + cnt[bkt];
            for (uint64_t i = 0; i < m; ++i) ui40_put(dst + i, a[i].pos);
        }
        }
        work_total += work;
        tm.lap("sa: sort group");
        if (work_total > budget) over = true;
        g0 = g1;
    }
    free(scratch);
    return over ? 1 : 0;           // 1: too repetitive for this scheme, the caller falls back to SA-IS
}

}  // namespace

// SA-IS over the bytes of any text: remapped to a dense alphabet, '$' -> 0 (must be unique and last)
static int sa_build_sais(const char *text, uint64_t L, lrm_ui40 *out) {
    std::vector<uint8_t> s((size_t) L);
    int map[256];
    bool seen[256] = {false};
    for (uint64_t i = 0; i < L; ++i) seen[(unsigned char) text[i]] = true;
    int K = 0;
    for (int c = 0; c < 256; ++c) map[c] = seen[c] ? K++ : -1;
    if (map[(unsigned char) '$'] != 0) { lrm_set_error("'$' is not the smallest byte of the text"); return -1; }
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
    for (uint64_t i = 0; i < L; ++i) s[i] = (uint8_t) map[(unsigned char) text[i]];
    if (L < (1ull << 31) - 8) {
        std::vector<int32_t> sa((size_t) L);
        SaIs<int32_t>::run<uint8_t>(s.data(), sa.data(), (int32_t) L, (int32_t) (K - 1));
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
        for (uint64_t i = 0; i < L; ++i) ui40_put(out + i, (uint64_t) (uint32_t) sa[i]);
    } else {
        // in place: SA-IS works on the caller's 8-byte slots as int64 (no second array) and leaves values < 2^40 in them,
        // which is what ui40_put would have written
        SaIs<int64_t>::run<uint8_t>(s.data(), reinterpret_cast<int64_t *>(out), (int64_t) L, (int64_t) (K - 1));
    }
    return 0;
}

int sa_build(const char *text, uint64_t L, const PackedText *packed, const BuildKnobs &knobs, lrm_ui40 *out) {
    if (text[L - 1] != '$') { lrm_set_error("text must end in '$'"); return -1; }
    {   // '$' must not occur inside the text
        uint64_t inner = ~0ull;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static) reduction(min : inner)
        for (uint64_t i = 0; i < L - 1; ++i) if (text[i] == '$' && i < inner) inner = i;
        if (inner != ~0ull) { lrm_set_error("'$' occurs inside the text (offset %llu)", (unsigned long long) inner); return -1; }
    }
    if (packed && !knobs.force_sais && L >= 2) {
        const int rc = sa_build_bucketed(*packed, L, out, knobs.force_bucket ? (1ull << 40) / L + 1024 : 24, knobs);
        if (rc <= 0) return rc;
        // too repetitive: the linear-time path
    }
    return sa_build_sais(text, L, out);
}

extern "C" int lrm_sa_build(const char *text, uint64_t L, lrm_ui40 *out) {
    if (!text || !out || L < 1) { lrm_set_error("bad argument"); return -1; }
    const BuildKnobs knobs = build_knobs();
    PackedText own;
    const bool pure = !knobs.force_sais && L >= 2 && pack_text(text, L, own);
    return sa_build(text, L, pure ? &own : nullptr, knobs, out);
}
