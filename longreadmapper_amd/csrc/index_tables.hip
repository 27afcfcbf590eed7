// index_tables.hip -- the index tables a handle derives on the device, once, when it is created: the long lc table
// (plain / pair-line / 5-byte entries + side table), the core table of small texts and the seed table.  Never on the hot
// path; what the kernels write here is read through seed_index_dev.h.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "seed_index_dev.h"

// entry of the long table for one hl-mer (code: first base lowest): the lc entry of its last hlen bases followed by
// hl - hlen backward steps -- the (k, l) the reference reaches after those steps -- as k | count << 40, 0 = absent,
// count 0xFFFFFF = "too long for 24 bits: take the reference's path"
__device__ __forceinline__ uint64_t lcl_entry(const LrmIndexView &ix, int hl, uint64_t code) {
    const int ext = hl - ix.hlen;
    uint64_t k, l;
    lc_lookup(ix, code >> (2 * ext), k, l);
    if (k == 0 && l == 0) return 0;
    for (int i = ext - 1; i >= 0 && k <= l; --i) {
        const uint32_t c = (uint32_t) (code >> (2 * i)) & 3u;
        uint64_t ra, rb;
        occ_lf2(ix, c, k - 1, l, ra, rb);
        k = ra + 1;
        l = rb;
    }
    if (k > l) return 0;
    const uint64_t cnt = l - k + 1;
    return cnt >= 0xFFFFFFull ? (0xFFFFFFull << 40) : (k | (cnt << 40));
}

// Long table, one lane per slot.  PLAIN layout: slot = hl-mer code.  PAIR-LINE layout (see seed_one): line S (an
// (hl-1)-mer), slot a < 4: the entry of a.S; slot 4 + b: the entry of S.b -- every hl-mer is stored twice (once as a
// left, once as a right extension of an (hl-1)-mer): 16 bytes per hl-mer, or 10 with 5-byte entries (kbits > 0).
// 5-byte entries whose count does not fit go to `ovf` ({code, entry} pairs, appended once per hl-mer: from its
// left-extension slot) for the side hash table.
__global__ __launch_bounds__(256) void lcl_build_kernel(LrmIndexView ix, int hl, int pair, int kbits, uint64_t *__restrict__ out,
                                                        uint64_t slot0, uint64_t *__restrict__ ovf, uint64_t ovf_cap,
                                                        unsigned long long *__restrict__ n_ovf) {
    const uint64_t slot = slot0 + (uint64_t) blockIdx.x * 256 + threadIdx.x;
    uint64_t code = slot;
    uint32_t w = 0;
    if (pair) {
        const uint64_t S = slot >> 3;
        if (S >= (1ull << (2 * (hl - 1)))) return;
        w = (uint32_t) slot & 7u;
        code = w < 4 ? ((S << 2) | w) : (S | ((uint64_t) (w - 4) << (2 * (hl - 1))));
    } else if (code >= (1ull << (2 * hl))) {
        return;
    }
    const uint64_t e = lcl_entry(ix, hl, code);
    if (!kbits) { out[slot] = e; return; }
    const uint64_t cmax = (1ull << (40 - kbits)) - 1ull, c = e >> 40;
    uint64_t v = e & ((1ull << 40) - 1ull);                            // k (< 2^kbits)
    if (e != 0) {
        if (c < cmax) v |= c << kbits;
        else {
            v |= cmax << kbits;
            if (w < 4) {
                const unsigned long long at = atomicAdd(n_ovf, 1ull);
                if (at < ovf_cap) { ovf[2 * at] = code; ovf[2 * at + 1] = e; }
            }
        }
    }
    uint8_t *p = reinterpret_cast<uint8_t *>(out) + slot * 5;
    const uint32_t lo = (uint32_t) v;
    __builtin_memcpy(p, &lo, 4);
    p[4] = (uint8_t) (v >> 32);
}

__global__ __launch_bounds__(256) void lclx_build_kernel(const uint64_t *__restrict__ ovf, uint64_t n, uint64_t *__restrict__ table, uint64_t mask) {
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t code = ovf[2 * i], e = ovf[2 * i + 1];
    uint64_t slot = (code * 0x9E3779B97F4A7C15ull) >> 20 & mask;
    for (;;) {
        const unsigned long long prev = atomicCAS((unsigned long long *) &table[2 * slot], 0ull, (unsigned long long) (code + 1));
        if (prev == 0ull || prev == code + 1) { table[2 * slot + 1] = e; return; }
        slot = (slot + 1) & mask;
    }
}

// Core table (see seed_one): every 16-mer X the text holds (a non-zero entry of the pair-line table `pl`) enters the lines
// of its four cores, once per role.  A line that cannot take an entry (all eight slots taken, or a count beyond 16 bits)
// goes on the overflow list and is set to all ones afterwards.
__device__ __forceinline__ void core_insert(uint64_t *core, uint64_t corec, uint32_t tag, uint64_t entry, bool fits, uint64_t *ovf,
                                            uint64_t ovf_cap, unsigned long long *n_ovf) {
    uint64_t *line = core + corec * 8;
    (void) tag;
    if (fits)
        for (int sl = 0; sl < 8; ++sl)                                     // slots fill from the front
            if (atomicCAS((unsigned long long *) &line[sl], 0ull, (unsigned long long) entry) == 0ull) return;
    const unsigned long long at = atomicAdd(n_ovf, 1ull);
    if (at < ovf_cap) ovf[at] = corec;
}
__global__ __launch_bounds__(256) void core_build_kernel(const uint64_t *__restrict__ pl, uint64_t *__restrict__ core, uint64_t x0,
                                                         uint64_t *__restrict__ ovf, uint64_t ovf_cap, unsigned long long *n_ovf) {
    const uint64_t X = x0 + (uint64_t) blockIdx.x * 256 + threadIdx.x;                  // a 16-mer, first base lowest
    if (X >> 32) return;
    const uint64_t e = pl[((X >> 2) << 3) + (X & 3u)];                                  // its entry as the left extension of its last 15 bases
    if (e == 0) return;
    const uint64_t c = e >> 40;
    const bool fits = c < 0xFFFFull;
    const uint64_t body = (e & ((1ull << 40) - 1ull)) | ((c & 0xFFFFull) << 40);
    for (uint32_t r = 0; r < 4; ++r) {
        const uint64_t corec = (X >> (2 * (3 - r))) & ((1ull << 26) - 1ull);
        const uint32_t extra = (uint32_t) (X & ((1ull << (2 * (3 - r))) - 1ull)) | ((uint32_t) (X >> (2 * (16 - r))) << (2 * (3 - r)));
        const uint32_t tag = r | (extra << 2);
        core_insert(core, corec, tag, body | ((uint64_t) tag << 56), fits, ovf, ovf_cap, n_ovf);
    }
}
__global__ __launch_bounds__(256) void core_ovf_kernel(uint64_t *__restrict__ core, const uint64_t *__restrict__ ovf, uint64_t n) {
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 8) return;
    core[ovf[i >> 3] * 8 + (i & 7)] = ~0ull;
}

// Seed table build, one lane per text position p: the S-mer at p is searched as a seed would be (through whatever
// tables the handle already has); the first lane to claim the interval's first row k in a bitmap over the rows (distinct
// S-mers have disjoint intervals) enters it -- once per distinct S-mer -- into the lines of its F roles.  What does not
// fit (a full line, a count of cmax or more) goes on the list for the side hash table.  The suffix array is read only
// for the text position a unique S-mer takes along (deduplication goes by the claimed rows, not by SA values).
__global__ __launch_bounds__(256) void sd_build_kernel(LrmIndexView ix, LrmIndexView sdv, uint64_t *__restrict__ sd, uint64_t p0,
                                                       uint32_t *__restrict__ claimed,
                                                       uint64_t *__restrict__ ovf, uint64_t ovf_cap, unsigned long long *__restrict__ n_ovf) {
    const uint64_t p = p0 + (uint64_t) blockIdx.x * 256 + threadIdx.x;
    const int S = sdv.sd_len;
    if (ix.con_len < (uint64_t) S + 1 || p > ix.con_len - 1 - (uint64_t) S) return;          // content[con_len - 1] is the '$'
    uint64_t code = 0;
    for (int i = 0; i < S; ++i) code |= (uint64_t) base_code((uint8_t) ix.content[p + i]) << (2 * i);
    uint64_t k, l;
    const uint64_t rr = seed_one(ix, code, S, (uint32_t) p, k, l);                            // (ix.sd is null here)
    if (rr == 0) return;
    if (atomicOr(&claimed[k >> 5], 1u << (k & 31u)) & (1u << (k & 31u))) return;               // another occurrence entered this S-mer
    const uint64_t cmax = (1ull << sdv.sd_cbits) - 1ull;
    uint64_t c = rr < cmax ? rr : cmax;
    uint64_t side = k | ((rr < 0xFFFFFFull ? rr : 0xFFFFFFull) << 40);
    if (rr == 1 && sdv.sd_kbits <= 38) {
        // a unique S-mer takes its text position along (count code 0): most hits of a read come from unique seeds, and every
        // one of them was a random 64-byte line of the suffix array in the vote stage
        const uint64_t pos = sa_locate(ix, k);
        if (pos >= 1 && pos < (1ull << sdv.sd_kbits)) { k = pos; c = 0; side = pos | LRM_LOCATED_BIT | (1ull << 40); }
    }
    bool to_side = rr >= cmax;
    for (uint32_t r = 0; r < (uint32_t) sdv.sd_f; ++r) {
        const SdKey key = sd_key_of(sdv, code, r);
        uint64_t *line = sd + key.line * 8;
        bool placed = false;
        if (sdv.sd_slot == 8) {
            const uint64_t v = k | (c << sdv.sd_kbits) | (key.tag << (64u - key.tb));
            for (int sl = 0; sl < 8 && !placed; ++sl)
                placed = atomicCAS((unsigned long long *) &line[sl], 0ull, (unsigned long long) v) == 0ull;
            if (!placed) atomicOr((unsigned long long *) &line[0], 1ull << (63u - key.tb));
        } else {
            const uint64_t v = k | (c << sdv.sd_kbits) | (key.tag << (48u - key.tb));
            const uint32_t at = atomicAdd(reinterpret_cast<uint32_t *>(line) + 15, 1u) & 0xFFu;
            if (at >= 250u) atomicAdd(n_ovf, 1ull << 40);                                     // (the count byte would run into the filter: give the table up)
            if (at >= 10u) atomicOr(reinterpret_cast<uint32_t *>(line) + 15, 1u << (8u + sd_filter_bit((uint32_t) key.tag)));
            if (at < 10u) {
                uint16_t *h = reinterpret_cast<uint16_t *>(line) + 3 * at;                   // three 2-byte stores: slots are 6 bytes apart
                h[0] = (uint16_t) v; h[1] = (uint16_t) (v >> 16); h[2] = (uint16_t) (v >> 32);
                placed = true;
            }
        }
        if (!placed) to_side = true;
    }
    if (to_side) {
        const unsigned long long at = atomicAdd(n_ovf, 1ull);
        if (at < ovf_cap) { ovf[2 * at] = code; ovf[2 * at + 1] = side; }
    }
}

__global__ __launch_bounds__(256) void sd_clear_kernel(ulonglong2 *__restrict__ p, uint64_t n16) {
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < n16; i += (uint64_t) gridDim.x * 256) p[i] = make_ulonglong2(0, 0);
}

// Geometry and build of the seed table (see sd_lookup).  Lines: the smallest power of two that keeps the average line
// at <= 2.2 entries of 8 (four positions per line: 4 entries per distinct S-mer) or, where that does not fit, at <= 6 of
// 10 (two positions per line, 6-byte slots) -- an E. coli-sized text: 2 GiB; chr1-sized: 64 GiB; GRCh38-sized (6.2 G
// rows): 128 GiB, 3.5 % of the lines overflow into a side table of ~0.13 G entries.
struct SdPlan { int f, bits, slot, kbits, cbits; uint64_t bytes; };
static bool sd_plan(const lrm_index *idx, uint64_t free_b, SdPlan *pl) {
    const LrmIndexTune &tu = idx->itune;
    const uint64_t L = idx->view.length;
    const int S = tu.sd_len;
    if (tu.sd == 0 || !idx->cpl_ok || L < 64 || idx->view.con_len != L) return false;
    int kbits = 1;
    while ((1ull << kbits) < L) ++kbits;
    for (int f = 4; f >= 2; f -= 2) {
        if (tu.sd_f && tu.sd_f != f) continue;
        const int slot = f == 4 ? 8 : 6, lf = f == 4 ? 2 : 1;
        const double target = f == 4 ? 2.2 : 6.0;
        int bits = 10;
        while ((double) f * (double) L / (double) (1ull << bits) > target && bits < 34) ++bits;
        if (tu.sd_bits) bits = tu.sd_bits;
        const int CL2 = 2 * (S - f + 1);
        if (bits > CL2) bits = CL2;
        if (bits < 11) bits = 11;
        if (bits < CL2 - 31) bits = CL2 - 31;                                    // (sd_key_of: fewer than 32 residue bits)
        const int tb = lf + 2 * (f - 1) + (CL2 - bits);
        int cbits = (slot == 8 ? 63 : 48) - tb - kbits;
        if (cbits < (tu.sd_bits ? 2 : 4) || tb > 40) continue;                  // (tests force few lines: long tags)
        if (cbits > 24) cbits = 24;
        if (tu.sd_cbits && tu.sd_cbits < cbits) cbits = tu.sd_cbits;
        const uint64_t bytes = 64ull << bits;
        // room: the table, its side table (<= 1/8 of it) and what the batch workspaces need afterwards
        const uint64_t spare = bytes >= (32ull << 30) ? (40ull << 30) : (8ull << 30);
        if (tu.sd < 0 && ((uint64_t) free_b < bytes + bytes / 8 + spare || (tu.lc_long_max >= 13 && bytes > (16ull << 30)))) continue;
        pl->f = f; pl->bits = bits; pl->slot = slot; pl->kbits = kbits; pl->cbits = cbits; pl->bytes = bytes;
        return true;
    }
    return false;
}
static void sd_filter_build(lrm_index *idx);
static int sd_build(lrm_index *idx, const SdPlan &pl) {
    uint64_t *d = nullptr, *ovf = nullptr, *tab = nullptr;
    uint32_t *claimed = nullptr;
    unsigned long long *n_ovf = nullptr;
    const char *why = "";
    unsigned long long n = 0;
    auto give_up = [&]() {
        if (idx->mtune.verbose) fprintf(stderr, "[lrm] seed table (share %d, 2^%d lines, %d-byte slots) not built: %s (side entries %llu)\n", pl.f, pl.bits, pl.slot, why, n);
        if (d) (void) hipFree(d); if (ovf) (void) hipFree(ovf); if (tab) (void) hipFree(tab); if (n_ovf) (void) hipFree(n_ovf);
        if (claimed) (void) hipFree(claimed);
        (void) hipGetLastError(); return 0; };
    const uint64_t L = idx->view.length, lines = 1ull << pl.bits;
    // (a core that occurs once in the text brings one entry PER ROLE to its line, so a line holds F x Poisson entries: with two
    //  positions per line and 2.9 cores per line on average 7 % of the lines of a GRCh38-sized text need more than ten slots)
    uint64_t ovf_cap = lines / 4 + 4096;
    if (ovf_cap > (1ull << 30)) ovf_cap = 1ull << 30;
    if (idx->itune.sd_bits) ovf_cap = (uint64_t) pl.f * L + 4096;                 // (tests force crowded lines)
    why = "no room for the table";
    if (hipMalloc(&d, pl.bytes + LRM_SD_TAIL) != hipSuccess) { d = nullptr; return give_up(); }     // (+ the line of zeros, lrm_internal.h)
    why = "no room for the overflow list";
    if (hipMalloc(&ovf, ovf_cap * 16) != hipSuccess) { ovf = nullptr; return give_up(); }
    if (hipMalloc(&n_ovf, 8) != hipSuccess) { n_ovf = nullptr; return give_up(); }
    const uint64_t cl_bytes = ((L + 31) / 32 + 1) * 4;
    if (hipMalloc(&claimed, cl_bytes) != hipSuccess) { claimed = nullptr; return give_up(); }
    why = "memset failed";
    if (hipMemset(claimed, 0, cl_bytes) != hipSuccess) return give_up();
    hipLaunchKernelGGL(sd_clear_kernel, dim3(256 * 64), dim3(256), 0, 0, reinterpret_cast<ulonglong2 *>(d), (pl.bytes + LRM_SD_TAIL) / 16);     // (128 GiB: not a hipMemset)
    if (hipGetLastError() != hipSuccess || hipMemset(n_ovf, 0, 8) != hipSuccess) return give_up();
    LrmIndexView sdv = idx->view;
    sdv.sd_len = idx->itune.sd_len; sdv.sd_f = pl.f; sdv.sd_bits = pl.bits; sdv.sd_kbits = pl.kbits; sdv.sd_slot = pl.slot; sdv.sd_cbits = pl.cbits;
    const uint64_t chunk = 1ull << 22;
    for (uint64_t b0 = 0, blocks = (L + 255) / 256; b0 < blocks; b0 += chunk) {
        const uint64_t nb = blocks - b0 < chunk ? blocks - b0 : chunk;
        hipLaunchKernelGGL(sd_build_kernel, dim3((uint32_t) nb), dim3(256), 0, 0, idx->view, sdv, d, b0 * 256, claimed, ovf, ovf_cap, n_ovf);
    }
    why = "build kernel failed";
    if (hipDeviceSynchronize() != hipSuccess) { give_up(); lrm_set_error("seed table build failed"); return -1; }
    why = "too many entries beside their lines";
    if (hipMemcpy(&n, n_ovf, 8, hipMemcpyDeviceToHost) != hipSuccess || n > ovf_cap) return give_up();       // too crowded: the other tables alone
    uint64_t tslots = 1024;
    while (tslots < 2 * n) tslots <<= 1;
    why = "no room for the side table";
    if (hipMalloc(&tab, tslots * 16) != hipSuccess) { tab = nullptr; return give_up(); }
    if (hipMemset(tab, 0, tslots * 16) != hipSuccess) return give_up();
    if (n) hipLaunchKernelGGL(lclx_build_kernel, dim3((uint32_t) ((n + 255) / 256)), dim3(256), 0, 0, ovf, (uint64_t) n, tab, tslots - 1);
    if (hipDeviceSynchronize() != hipSuccess) { give_up(); lrm_set_error("seed table side build failed"); return -1; }
    (void) hipFree(ovf); (void) hipFree(n_ovf); (void) hipFree(claimed);
    idx->d_sd = d; idx->d_sdx = tab;
    idx->view.sd = d; idx->view.sdx = tab; idx->view.sdx_mask = tslots - 1;
    idx->view.sd_len = sdv.sd_len; idx->view.sd_f = pl.f; idx->view.sd_bits = pl.bits; idx->view.sd_kbits = pl.kbits; idx->view.sd_slot = pl.slot;
    idx->view.sd_cbits = pl.cbits;
    idx->sd_side_entries = n;
    if (idx->mtune.verbose) fprintf(stderr, "[lrm] seed table: %d positions per line, 2^%d lines, %d-byte slots, %d count bits, %llu side entries\n", pl.f, pl.bits, pl.slot, pl.cbits, n);
    sd_filter_build(idx);
    return 0;
}

// Presence bitmap of the seed table's lines, derived from the FINISHED table (after sd_build_kernel and the side-table
// build): bit (line >> g) is set iff any of the 8 words of any of the 2^g lines it covers is non-zero.  seed_search looks
// the bit up before it fetches a line and takes a clear bit for a line of zeros.  Why that is exact: on an all-zero line
// sd_search returns 0, "absent", before the side table is consulted -- no slot matches with e != 0, and the overflow bit of
// slot 0 is clear.  Whatever makes a seed present leaves a non-zero word in ITS line: an entry that found room is a
// non-zero slot (k >= 1 or a tag), an entry that found no room sets the overflow bit of slot 0 of a line that is full, and
// a count of cmax sits in its line beside its side-table entry.  So a clear bit means exactly what the fetched line
// would have said.  One lane per line; a lane reads the word before the atomic, so a bit costs one atomic per wavefront
// that finds it clear, not one per line.
__global__ __launch_bounds__(256) void sd_filter_kernel(const ulonglong2 *__restrict__ sd, uint64_t lines, uint32_t g,
                                                        uint32_t *__restrict__ filt) {
    const uint64_t line = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (line >= lines) return;
    const ulonglong2 x0 = sd[line * 4], x1 = sd[line * 4 + 1], x2 = sd[line * 4 + 2], x3 = sd[line * 4 + 3];
    if (((x0.x | x0.y) | (x1.x | x1.y) | (x2.x | x2.y) | (x3.x | x3.y)) == 0) return;
    const uint64_t bit = line >> g;
    const uint32_t m = 1u << (bit & 31u);
    if (!(filt[bit >> 5] & m)) atomicOr(&filt[bit >> 5], m);
}
__global__ __launch_bounds__(256) void sd_filter_count_kernel(const uint32_t *__restrict__ filt, uint64_t words,
                                                              unsigned long long *__restrict__ n_set) {
    uint32_t c = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < words; i += (uint64_t) gridDim.x * 256) c += __popc(filt[i]);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(n_set, (unsigned long long) c);
}
// Built for the table form that seed_search's SD48 instantiation reads (four positions per line, 8-byte slots, tags of at
// most 32 bits) and kept only when at most HALF of its bits are set: a bitmap fuller than that cannot halve the fetches.
// g is the smallest for which the bitmap is at most itune.sd_filter_kb KiB.  Bench text (9.28 M rows, 2^25 lines): 0.277
// cores per line, 24 % of the lines non-zero; at 2 MiB g = 1 and 1 - exp(-0.553) = 43 % of the bits are set.  A chr1-sized
// text (2^30 lines, g = 6, 15 cores per bit) fills every bit: there the pass over the 64 GiB table is not even made -- a
// text whose every S-mer occurred four times would still set more than half of the bits when cores per bit > 4 ln 2.
// Nothing depends on the bitmap: any failure here leaves the handle without one.
static void sd_filter_build(lrm_index *idx) {
    const LrmIndexView &v = idx->view;
    const int kb = idx->itune.sd_filter_kb;
    if (kb <= 0 || !lrm_sd48_form(v)) return;
    const uint64_t lines = 1ull << v.sd_bits, max_bits = (uint64_t) kb * 8192;
    uint32_t g = 0;
    while ((lines >> g) > max_bits) ++g;
    const uint64_t bits = lines >> g;
    if (bits < 512) return;                                       // (the zeros behind the bitmap start on a 64-byte boundary)
    if ((double) v.length / (double) bits > 4.0 * 0.6931471805599453) {
        if (idx->mtune.verbose) fprintf(stderr, "[lrm] seed filter: not built, %.1f rows per bit at %d KiB\n", (double) v.length / (double) bits, kb);
        return;
    }
    uint32_t *filt = nullptr;
    unsigned long long *d_n = nullptr, n_set = 0;
    // (64 bytes of zeros stand behind the bitmap: the line that seed_search fetches where a bit is clear, sd_issue_filtered)
    bool ok = hipMalloc(&filt, bits / 8 + 64) == hipSuccess && hipMalloc(&d_n, 8) == hipSuccess
              && hipMemset(filt, 0, bits / 8 + 64) == hipSuccess && hipMemset(d_n, 0, 8) == hipSuccess;
    if (ok) {
        const uint64_t chunk = 1ull << 30;                                        // lines per launch
        for (uint64_t l0 = 0; l0 < lines; l0 += chunk) {
            const uint64_t nl = lines - l0 < chunk ? lines - l0 : chunk;
            hipLaunchKernelGGL(sd_filter_kernel, dim3((uint32_t) ((nl + 255) / 256)), dim3(256), 0, 0,
                               reinterpret_cast<const ulonglong2 *>(v.sd) + l0 * 4, nl, g, filt + ((l0 >> g) >> 5));
        }
        hipLaunchKernelGGL(sd_filter_count_kernel, dim3(256), dim3(256), 0, 0, filt, bits / 32, d_n);
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(&n_set, d_n, 8, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (d_n) (void) hipFree(d_n);
    const bool keep = ok && 2 * n_set <= bits;
    if (idx->mtune.verbose && ok)
        fprintf(stderr, "[lrm] seed filter: %llu bytes, one bit per %u lines, %.1f %% of the bits set%s\n", (unsigned long long) (bits / 8), 1u << g,
                100.0 * (double) n_set / (double) bits, keep ? "" : ": more than half, not kept");
    if (!keep) { if (filt) (void) hipFree(filt); (void) hipGetLastError(); return; }
    idx->d_sd_filt = filt;
    idx->view.sd_filt = filt; idx->view.sd_filt_shift = (int32_t) g;
}

// The long seed table.  seed_search's time is its L2 misses divided by ~50 G random 64-byte lines per second
// (tools/randline_bench.hip pins that rate independently), and the first lookup of a seed is a miss whatever the text,
// so the table is (a) as long as HBM allows -- the longer the k-mer, the more noisy seeds die in the lookup instead of one
// random step later -- and (b) in the pair-line layout, where the lookups of two neighbouring read positions share a
// line.  Measured on 100 k x 10 kbp ONT reads, ms per Gbp [r2]: E. coli-sized text plain 13-mers 24.5, pair-line
// 13 / 14 / 15 / 16-mers 19.2 / 18.5 / 17.6 / 15.6; chr1-sized text plain 16 28.4, pair-line 16 20.3; GRCh38-sized text
// plain 16 40.6, plain 17 (128 GiB) 32.4, pair-line 16 (64 GiB) 30.2.
// Automatic choice: texts of >= 2^32 rows (every 16-mer occurs: the lookup decides nothing there) take pair-line 17-mers
// with 5-BYTE entries (160 GiB) when that leaves 40 GiB of HBM free; otherwise pair-line 16-mers with 8-byte entries
// (64 GiB) when that leaves 64 GiB free, else 15 (16 GiB, leaving 32), 14 (4 GiB, leaving 8), 13 (1 GiB).
// lrm_index_options lc_long = 0 (off) | 13..17, lc_pair = 0 | 1, lc_entry_bytes = 5 | 8 override.  A table that cannot
// be allocated is skipped: results never depend on it.  Cost at upload [r2]: 16 GiB and below ~10 ms, the 64 GiB
// table 0.65 s (2 s when the memory was freed a moment ago) -- repaid after a few hundred Gbp of reads, so callers that
// know their run is short cap the length (lrm_index_options.lc_long_max; lrm_accaln does it from the size of the reads
// file).
static int lcl_prepare_tables(lrm_index *idx, size_t free_b, bool have_sd);
int lrm_lcl_prepare_index(lrm_index *idx) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); free_b = 0; }
    // The seed table (seeds of the usual length) is planned first and built last, through the tables made here for the seeds
    // of any other length; those make do with the HBM it leaves.
    SdPlan sdp;
    const bool want_sd = sd_plan(idx, free_b, &sdp);
    if (want_sd) { const uint64_t need = sdp.bytes + sdp.bytes / 8; free_b = free_b > need ? free_b - need : 0; }
    const int rc_lcl = lcl_prepare_tables(idx, free_b, want_sd);
    if (rc_lcl) return rc_lcl;
    return want_sd ? sd_build(idx, sdp) : 0;
}

static int lcl_prepare_tables(lrm_index *idx, size_t free_b, bool have_sd) {
    const uint64_t L = idx->view.length;
    int hl = 13, pair = 1, ebytes = 8;
    int kbits = 1;
    while ((1ull << kbits) < L) ++kbits;
    static const struct { int hl, ebytes; uint64_t spare, min_rows; } ladder[] = {
        {17, 5, 40ull << 30, 1ull << 32}, {16, 8, 64ull << 30, 0}, {15, 8, 32ull << 30, 0}, {14, 8, 8ull << 30, 0}};
    for (const auto &c : ladder)
        if (L >= c.min_rows && kbits <= 36 && !(have_sd && c.hl > 16) && (uint64_t) free_b >= (2ull * c.ebytes << (2 * c.hl)) + c.spare) { hl = c.hl; ebytes = c.ebytes; break; }
    const LrmIndexTune &tu = idx->itune;
    if (tu.lc_long_max >= 13 && hl > tu.lc_long_max) { hl = tu.lc_long_max; ebytes = 8; }      // the caller expects a short run
    if (tu.lc_long >= 0) { if (tu.lc_long != hl) ebytes = 8; hl = tu.lc_long; }
    if (tu.lc_pair >= 0) pair = tu.lc_pair != 0;
    if (tu.lc_entry_bytes) ebytes = tu.lc_entry_bytes;
    if (!pair || kbits > 36) ebytes = 8;                               // (>= 4 count bits; the plain layout keeps aligned 8-byte entries)
    if (tu.lc_count_bits && 40 - tu.lc_count_bits >= kbits) kbits = 40 - tu.lc_count_bits;       // (tests: few count bits force the side table)
    if (hl <= idx->view.hlen || hl > 17 || L < 2) return 0;
    uint64_t *d = nullptr, *ovf = nullptr, *tab = nullptr;
    unsigned long long *n_ovf = nullptr;
    const uint64_t slots = (pair ? 2ull : 1ull) << (2 * hl);
    const uint64_t ovf_cap = ebytes == 5 ? (slots / 64 < (64ull << 20) ? slots / 64 + 1024 : (64ull << 20)) : 0;
    auto give_up = [&]() { if (d) (void) hipFree(d); if (ovf) (void) hipFree(ovf); if (tab) (void) hipFree(tab); if (n_ovf) (void) hipFree(n_ovf); (void) hipGetLastError(); };
    if (hipMalloc(&d, slots * (uint64_t) ebytes + 16) != hipSuccess) { d = nullptr; give_up(); return 0; }     // no room: the reference's table alone
    if (ebytes == 5 && (hipMalloc(&ovf, ovf_cap * 16) != hipSuccess || hipMalloc(&n_ovf, 8) != hipSuccess || hipMemset(n_ovf, 0, 8) != hipSuccess)) { give_up(); return 0; }
    const uint64_t chunk = 1ull << 22;                                // 2^30 threads per launch (grid limit 2^32)
    for (uint64_t b0 = 0, blocks = slots / 256; b0 < blocks; b0 += chunk) {
        const uint64_t nb = blocks - b0 < chunk ? blocks - b0 : chunk;
        hipLaunchKernelGGL(lcl_build_kernel, dim3((uint32_t) nb), dim3(256), 0, 0, idx->view, hl, pair, ebytes == 5 ? kbits : 0, d, b0 * 256,
                           ovf, ovf_cap, n_ovf);
    }
    if (hipDeviceSynchronize() != hipSuccess) { give_up(); lrm_set_error("long lc table build failed"); return -1; }
    uint64_t mask = 0;
    if (ebytes == 5) {
        unsigned long long n = 0;
        if (hipMemcpy(&n, n_ovf, 8, hipMemcpyDeviceToHost) != hipSuccess || n > ovf_cap) { give_up(); return 0; }   // (too many: the lchash image alone)
        uint64_t tslots = 1024;
        while (tslots < 2 * n) tslots <<= 1;
        mask = tslots - 1;
        if (hipMalloc(&tab, tslots * 16) != hipSuccess || hipMemset(tab, 0, tslots * 16) != hipSuccess) { give_up(); return 0; }
        if (n) hipLaunchKernelGGL(lclx_build_kernel, dim3((uint32_t) ((n + 255) / 256)), dim3(256), 0, 0, ovf, (uint64_t) n, tab, mask);
        if (hipDeviceSynchronize() != hipSuccess) { give_up(); lrm_set_error("long lc side table build failed"); return -1; }
        (void) hipFree(ovf); (void) hipFree(n_ovf);
    }
    idx->d_lcl = d;
    idx->d_lclx = tab;
    idx->view.lcl = d;
    idx->view.hl = hl;
    idx->view.lcl_pair = pair;
    idx->view.lcl_kbits = ebytes == 5 ? kbits : 0;
    idx->view.lclx = tab;
    idx->view.lclx_mask = mask;
    // Core table on top of pair-line 16-mers with 8-byte entries, for texts small enough that a 13-mer's line holds the
    // 16-mers around it (4 L / 4^13 entries per line on average: 0.55 for an E. coli-sized text, 2 at 2^25 rows).
    const bool core_auto = L <= (1ull << 25);
    if (hl == 16 && pair && ebytes == 8 && (tu.lc_core > 0 || (tu.lc_core < 0 && core_auto))) {
        uint64_t *dc = nullptr, *covf = nullptr;
        unsigned long long *cn = nullptr;
        const uint64_t lines = 1ull << 26, ocap = 16ull << 20;
        bool ok = hipMalloc(&dc, lines * 64) == hipSuccess && hipMalloc(&covf, ocap * 8) == hipSuccess && hipMalloc(&cn, 8) == hipSuccess &&
                  hipMemset(dc, 0, lines * 64) == hipSuccess && hipMemset(cn, 0, 8) == hipSuccess;
        if (ok) {
            for (uint64_t b0 = 0, blocks = (1ull << 32) / 256; b0 < blocks; b0 += chunk) {
                const uint64_t nb = blocks - b0 < chunk ? blocks - b0 : chunk;
                hipLaunchKernelGGL(core_build_kernel, dim3((uint32_t) nb), dim3(256), 0, 0, (const uint64_t *) d, dc, b0 * 256, covf, ocap, cn);
            }
            unsigned long long n = 0;
            ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(&n, cn, 8, hipMemcpyDeviceToHost) == hipSuccess && n <= ocap;
            if (ok && n) {
                hipLaunchKernelGGL(core_ovf_kernel, dim3((uint32_t) ((n * 8 + 255) / 256)), dim3(256), 0, 0, dc, (const uint64_t *) covf, (uint64_t) n);
                ok = hipDeviceSynchronize() == hipSuccess;
            }
        }
        if (covf) (void) hipFree(covf);
        if (cn) (void) hipFree(cn);
        if (ok) { idx->d_core = dc; idx->view.core = dc; }
        else { if (dc) (void) hipFree(dc); (void) hipGetLastError(); }      // no room or too many crowded lines: the pair-line table alone
    }
    return 0;
}
