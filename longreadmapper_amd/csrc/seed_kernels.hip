// seed_kernels.hip -- gfx950 kernels for PART 1 of the accaln hot path
// (reference: alnmain.c:333-405; lchash.c:12-16,36-49,89-104; fmidx.c:18-33,277-313;
//  histo.c:26-56,84-96).  Integer gathers + LDS voting; no MFMA (nothing here is a
// contraction).  The lookups in the index tables are in seed_index_dev.h, the kernels that build them in index_tables.hip.
//
// Decomposition (MI355X-first, not the reference's per-read loop nest):
//   pack2bit      reads (1 B/base) -> 2 bit/base stream, so a seed is ONE bit-field window
//   seed_search   one lane per seed: lc lookup + FM backward extension; compact survivor lists   (K1, HBM gathers)
//   vote          one wavefront or workgroup per (read, phase): flat hit expansion, SA gather, LDS vote table (K2, vote_kernels.hip)
//   decide        one lane per read: the phase state machine of alnmain.c:371-403
//
// The reference evaluates phases one after another and stops at the first phase whose
// top-2 vote passes 0.6.  Phases are independent computations, so evaluating them
// speculatively and replaying the decisions in order is exact.  To avoid 21x waste on
// clean reads the host launches phase 0 first and phases 1..s only for undecided reads.
#include <hip/hip_runtime.h>
#include "seed_index_dev.h"

// ----------------------------------------------------------------------------------------
// pack2bit: one thread per output dword (16 bases: one 16-byte load -- rows start at any byte, the hardware
// takes the unaligned dwords -- and one 4-byte store).  Bases past the read end pack as 0.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack2bit_kernel(const char *__restrict__ reads, uint64_t stride,
                                                       const uint32_t *__restrict__ lens,
                                                       uint8_t *__restrict__ out, uint64_t bytes_per_read,
                                                       uint32_t chunks_per_read, uint64_t n) {
    uint64_t read = blockIdx.x / chunks_per_read;
    uint32_t chunk = blockIdx.x % chunks_per_read;
    if (read >= n) return;
    uint64_t ow = (uint64_t) chunk * 256 + threadIdx.x;
    if (ow * 4 >= bytes_per_read) return;
    uint32_t len = lens[read];
    const uint8_t *r = (const uint8_t *) reads + read * stride;
    uint64_t p = ow * 16;
    uint32_t v = 0;
    if (p + 16 <= len) {
        uint32_t w[4];
        __builtin_memcpy(w, r + p, 16);
#pragma unroll
        for (int t = 0; t < 16; ++t) v |= base_code((w[t >> 2] >> (8 * (t & 3))) & 0xffu) << (2 * t);
    } else {
        for (int t = 0; t < 16; ++t) {
            uint32_t code = (p + t < len) ? base_code(r[p + t]) : 0u;
            v |= code << (2 * t);
        }
    }
    *reinterpret_cast<uint32_t *>(out + read * bytes_per_read + ow * 4) = v;
}

template <int CTRL>
__device__ __forceinline__ uint64_t quad_perm64(uint64_t v) {
    const uint32_t lo = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) v, CTRL, 0xf, 0xf, true);
    const uint32_t hi = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) (v >> 32), CTRL, 0xf, 0xf, true);
    return (uint64_t) lo | ((uint64_t) hi << 32);
}
// The lanes of a wavefront hold CONSECUTIVE read positions (lane id == position, mod sd_f): the sd_f lanes that share a line
// fetch it TOGETHER -- every lane one quarter (half) of the line of the group's first lane, a contiguous 64-byte request per
// group instead of four 16-byte requests per lane -- and pass the pieces around inside the quad (DPP quad_perm: no LDS).
// Every lane of the wavefront must be here (lanes without a seed come with win = 0 and ignore the answer); a lane whose
// group's first lane has no seed has none either (positions grow with the lane id).
// sd_issue_shared starts the fetch (the lane's piece: a, and b with two positions per line), sd_finish_shared gathers the
// line and searches it.  (Keeping the fetches of 2 / 4 / 8 of a lane's seeds in flight between the two, all issued together
// and all waited for together: 7.85 / 8.56 / 10.3 ms per Gbp on the bench workload against 7.63 for one.  What pays is the
// fetch of the NEXT position under way while THIS one is searched -- the loop of seed_search_kernel, 6.84 against 7.3 [r13].)
__device__ __forceinline__ void sd_issue_shared(const LrmIndexView &ix, const SdKey &key, ulonglong2 &a, ulonglong2 &b) {
    const uint32_t lane = __lane_id();
    if (ix.sd_f == 4) {
        const uint64_t line = quad_perm64<0x00>(key.line);                                    // quad_perm [0,0,0,0]
        a = *reinterpret_cast<const ulonglong2 *>(ix.sd + line * 8 + (lane & 3u) * 2);
        b = a;
    } else {
        const uint64_t line = quad_perm64<0xA0>(key.line);                                    // [0,0,2,2]
        const uint64_t *src = ix.sd + line * 8 + (lane & 1u) * 4;
        a = *reinterpret_cast<const ulonglong2 *>(src);
        b = *reinterpret_cast<const ulonglong2 *>(src + 2);
    }
}
// The same fetch behind the presence bitmap of the table's lines (index_tables.hip, sd_filter_build; four positions per line
// only), in two steps.  sd_filter_issue: the quad starts the load of the bitmap word of its line (the four lanes share the
// core, so the word).  sd_issue_filtered, with the word in hand: a quad whose bit is set fetches its line, the others fetch
// the 64 bytes of zeros that stand behind the bitmap -- a line of zeros is what the table holds where the bit is clear, so
// sd_finish_shared answers "absent" with no branch of its own, and the fetch INSTRUCTION is issued on every path, whatever
// the bits say: the count of loads in flight stays the same everywhere, which the counted waits of the loop need.  A
// position past the end (real false) loads word 0 and fetches the zeros.  What a clear bit saves is a random line of a
// table of GiB; what it costs is a word of a bitmap of a few MiB, which does NOT all stay in the L2 beside the streaming
// table lines (bench text, 4 MiB: about four in ten bitmap loads miss it, 2 MiB: two in ten) but is cheap all the same --
// the larger bitmap has more L2 misses and is the faster one (profiles/r19, section 1).
__device__ __forceinline__ uint32_t sd_filter_issue(const LrmIndexView &ix, const SdKey &key, bool real, uint32_t &bit) {
    const uint64_t line = quad_perm64<0x00>(key.line);                                        // quad_perm [0,0,0,0]
    bit = real ? (uint32_t) (line >> (uint32_t) ix.sd_filt_shift) : 0u;
    return ix.sd_filt[bit >> 5];
}
__device__ __forceinline__ void sd_issue_filtered(const LrmIndexView &ix, const SdKey &key, bool real, uint32_t word, uint32_t bit,
                                                  ulonglong2 &a, ulonglong2 &b) {
    const uint32_t lane = __lane_id();
    const uint64_t line = quad_perm64<0x00>(key.line);
    const uint64_t *zeros = reinterpret_cast<const uint64_t *>(ix.sd_filt + ((1ull << ix.sd_bits) >> (uint32_t) ix.sd_filt_shift >> 5));
    const bool pass = real && ((word >> (bit & 31u)) & 1u);
    const uint64_t *src = pass ? ix.sd + line * 8 : zeros;
    a = *reinterpret_cast<const ulonglong2 *>(src + (lane & 3u) * 2);
    b = a;
}
// The same two steps for a table that ends below 2^32 bytes (lrm_sd_off32), where a line index is ONE register: one DPP
// move, 32-bit shifts, and the fetch addressed as the table's base (scalar) plus a 32-bit byte offset.  A quad whose bit is
// clear fetches the line of zeros at the table's own end (LRM_SD_TAIL): one select between two offsets in registers, no
// second base address.  line is the quad's line, kept from the first step for the second; piece and zpiece are the byte
// offsets of the lane's 16 bytes inside a line and inside the line of zeros, both the same in every step.  A position past
// the end comes with key.line == 0, so its bit index is 0 with no select.  (Per position 9 vector instructions where the
// 64-bit form above has 22, profiles/r20, section 1.)
__device__ __forceinline__ uint32_t sd_filter_issue32(const LrmIndexView &ix, const SdKey &key, uint32_t &bit, uint32_t &line) {
    line = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) key.line, 0x00, 0xf, 0xf, true);      // quad_perm [0,0,0,0]
    bit = line >> (uint32_t) ix.sd_filt_shift;
    return ix.sd_filt[bit >> 5];
}
__device__ __forceinline__ void sd_issue_filtered32(const LrmIndexView &ix, bool real, uint32_t word, uint32_t bit, uint32_t line,
                                                    uint32_t piece, uint32_t zpiece, ulonglong2 &a, ulonglong2 &b) {
    const bool pass = real && ((word >> (bit & 31u)) & 1u);
    const uint32_t off = pass ? (line << 6) + piece : zpiece;
    a = *reinterpret_cast<const ulonglong2 *>(reinterpret_cast<const char *>(ix.sd) + off);
    b = a;
}
// The gather and the search of sd_finish_shared / sd_search in one, for the loop behind the bitmap (four positions per line,
// 8-byte slots, tags of at most 32 bits), slot by slot from the last to the first as there.  The tag compare is
// `x = hi ^ (tag << sh)`, `x < 2^sh`: x is zero above the slot's count exactly where the tags agree and IS the slot's high
// dword below the tag, so the one value serves the compare and the select, and the DPP move of a high dword -- one use, and
// that use next to it -- folds into the xor: five vector instructions per slot where gather-then-search has six.  The chain
// of high dwords starts at `tag << sh`, which the last xor turns into 0, "no slot".  (2^sh sits in a scalar register behind
// an empty asm: where the compiler can see the power of two it turns the compare back into a shift and a compare.)
template <int CTRL>
__device__ __forceinline__ void sd_slot32(uint64_t w, uint32_t tsh, uint32_t lim, uint32_t &elo, uint32_t &ex, uint32_t &x, uint32_t &lo) {
    x = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) (w >> 32), CTRL, 0xf, 0xf, true) ^ tsh;
    lo = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) w, CTRL, 0xf, 0xf, true);
    const bool m = x < lim;
    elo = m ? lo : elo;
    ex = m ? x : ex;
}
__device__ __forceinline__ int sd_finish_quad32(const LrmIndexView &ix, const SdKey &key, uint64_t code, const ulonglong2 &a,
                                                uint64_t &k, uint64_t &c) {
    const uint32_t sh = 32u - key.tb, tsh = (uint32_t) key.tag << sh;
    uint32_t lim = 1u << sh, elo = 0, ex = tsh, x, lo;
    asm("" : "+s"(lim));
    sd_slot32<0xFF>(a.y, tsh, lim, elo, ex, x, lo); sd_slot32<0xFF>(a.x, tsh, lim, elo, ex, x, lo);       // slots 7, 6: [3,3,3,3]
    sd_slot32<0xAA>(a.y, tsh, lim, elo, ex, x, lo); sd_slot32<0xAA>(a.x, tsh, lim, elo, ex, x, lo);       // 5, 4: [2,2,2,2]
    sd_slot32<0x55>(a.y, tsh, lim, elo, ex, x, lo); sd_slot32<0x55>(a.x, tsh, lim, elo, ex, x, lo);       // 3, 2: [1,1,1,1]
    sd_slot32<0x00>(a.y, tsh, lim, elo, ex, x, lo); sd_slot32<0x00>(a.x, tsh, lim, elo, ex, x, lo);       // 1, 0: [0,0,0,0]
    // bit 63 - tb of slot 0, the line's overflow mark: below the tag in the high dword, where x is the slot's own bits
    const bool ovf = key.tb == 32u ? lo >> 31 : (x >> (sh - 1u)) & 1u;
    return sd_answer(ix, code, (uint64_t) elo | ((uint64_t) (ex ^ tsh) << 32), ovf, k, c, nullptr);
}
__device__ __forceinline__ int sd_finish_shared(const LrmIndexView &ix, const SdKey &key, uint64_t code, const ulonglong2 &a, const ulonglong2 &b,
                                                uint64_t &k, uint64_t &c, uint32_t *cnt) {
    uint64_t W[8];
    if (ix.sd_f == 4) {
        W[0] = quad_perm64<0x00>(a.x); W[1] = quad_perm64<0x00>(a.y);
        W[2] = quad_perm64<0x55>(a.x); W[3] = quad_perm64<0x55>(a.y);                         // [1,1,1,1]
        W[4] = quad_perm64<0xAA>(a.x); W[5] = quad_perm64<0xAA>(a.y);                         // [2,2,2,2]
        W[6] = quad_perm64<0xFF>(a.x); W[7] = quad_perm64<0xFF>(a.y);                         // [3,3,3,3]
    } else {
        const uint64_t pa = quad_perm64<0xB1>(a.x), pb = quad_perm64<0xB1>(a.y);              // [1,0,3,2]: the partner's half
        const uint64_t pc = quad_perm64<0xB1>(b.x), pd = quad_perm64<0xB1>(b.y);
        const bool odd = __lane_id() & 1u;
        W[0] = odd ? pa : a.x; W[1] = odd ? pb : a.y; W[2] = odd ? pc : b.x; W[3] = odd ? pd : b.y;
        W[4] = odd ? a.x : pa; W[5] = odd ? a.y : pb; W[6] = odd ? b.x : pc; W[7] = odd ? b.y : pd;
    }
    if (cnt) cnt[0] += 1;
    return sd_search(ix, key, code, W, k, c, cnt);
}

struct __attribute__((aligned(8))) WordPair { uint64_t a, b; };

__device__ __forceinline__ uint64_t read_window(const uint64_t *__restrict__ words, uint32_t j) {
    uint32_t wi = j >> 5, sh = (j & 31) * 2;
    WordPair w;                                           // ONE 16-byte request; branch-free, so that the compiler
    __builtin_memcpy(&w, words + wi, sizeof(w));          // cannot split it into a load plus a conditional second load
    return (w.a >> sh) | ((w.b << 1) << (63 - sh));       // sh == 0: the second term shifts out entirely
}

// One survivor into the LDS list of its phase.  s_tot[ph] holds the phase's survivor count in its low word and the sum of
// their rr in its high word, so ONE returning 64-bit LDS add reserves the slot and adds the hits (the sum wraps at 32 bits
// out of the top of the word, as the 32-bit global sum it goes into does).
__device__ __forceinline__ void ss_append(uint64_t *s_tot, uint64_t *s_rec, uint32_t *s_q, uint32_t cap_pp, uint32_t ph, uint32_t q, uint64_t k,
                                          uint64_t rr) {
    const uint32_t slot = (uint32_t) atomicAdd(reinterpret_cast<unsigned long long *>(&s_tot[ph]), 1ull | (rr << 32));
    s_rec[ph * cap_pp + slot] = k | (rr << 40);
    s_q[ph * cap_pp + slot] = q;
}

// ----------------------------------------------------------------------------------------
// K1 seed_search: one lane per seed, SS_ITEMS seeds per workgroup (4 or 8 per thread).  Work items of a read are
// (q, iter) with iter fastest, so the 64 lanes of a wavefront hold 64 CONSECUTIVE read positions.
// Output: the SURVIVORS only (0 < rr < thres, ~25 % of the seeds of a noisy read), compact per (read, phase):
//   rec [id][0 .. cnt[id])   k | rr << 40         recq[id][..]  seed ordinal q        (id = read*P + phase)
//   cnt [id]  survivors      hits[id]  sum of rr  (= SA rows the vote will gather; routes the item to its tier)
// A workgroup appends its survivors to per-phase lists in LDS (LDS atomics), reserves room in the global lists with
// ONE global atomic per phase and workgroup, and copies every list segment out with contiguous stores.  (The first
// version stored an 8-byte record per seed POSITION, 75 % zeros, with scattered stores: 16.7 GB written per Gbp,
// and every vote tier re-read all of it.)  The order of a list does not matter: the first-seen order key of a hit,
// (q << tbits) | t, is a property of the hit.
// ----------------------------------------------------------------------------------------
// SS_ITEMS seeds per workgroup (LDS lists of 12 B per seed; LRM_SS_ITEMS=1024|2048|4096 overrides the default 2048).
// Measured per 1-Gbp step [r2]: E. coli-sized text 512 / 1024 / 2048 / 4096 seeds: 26.2 / 25.5 / 24.9 / 31.6 ms;
// GRCh38-sized text 1024 / 2048 / 4096: 44.0 / 40.9 / 42.7 ms.  More resident wavefronts (1024: eight workgroups per
// CU instead of six) do NOT help: the kernel is bound by the memory system's random-request rate, not by latency.
// FEWER hurt [r13, profiles/r13, ms of the kernel alone on the chip per 1-Gbp step]: six workgroups per CU (2048 seeds,
// 26 112 B of LDS) 7.0 - 7.3 with one fetch in flight per lane, 6.5 - 6.85 with two (the shared-lines loop below); FOUR per
// CU -- room for one extension wavefront of 248 VGPRs beside them on every SIMD -- 9.0 - 9.1 with one fetch (LRM_SS_PAD;
// r3: 16.2 -> 21.8 on the kernel of that time), 7.7 with two, and 4096 seeds (three per CU) with two 8.06; the bench on
// three streams follows the kernel alone (60.0 parent, 63.0 six with two fetches, 57.9 four with two, 54.3 four with
// one, 56.9 three with two Gbp/s): the extension's launches get a tenth shorter in the room, a third of what this kernel's
// lose.  So the occupancy stays where the LDS puts it, and
// the attribute only says so to the register allocator: at least six wavefronts per SIMD (the pipelined loop takes 64
// VGPRs, the generic instantiation 61; no scratch).  It is the build that was measured: without it the compiler allocates
// the pipelined loop differently.
// COUNT: the counting build (lrm_workspace_set_counting; bench bookkeeping, never in a timed region) adds up the
// memory requests the device layout really makes -- seeds evaluated, 8-byte table lookups, 16-byte rank requests --
// into counters->seed_traffic.
// SD48: the instantiation for the seed table's usual form (E. coli- to chr1-sized texts: four positions per line, 8-byte
// slots, tags of at most 32 bits; the launcher checks idx->view): the shared-lines loop is compiled for that form alone,
// with no branch on the other table forms in it.  Every other handle, and the counting build, take the generic one.
// FILT (only together with SD48; the launcher takes it when the handle has a presence bitmap of the table's lines,
// idx->view.sd_filt): the kernel sits at the memory system's rate of random lines, and three in four lines of a sparse
// table (a bacterial-sized text) hold nothing, so a position first reads the bit of its line -- from a bitmap of a few
// MiB, of whose loads six in ten hit the L2 at the default size -- and fetches the line only when the bit is set: fewer
// random lines moved this kernel from 6.24 - 6.44 to 5.39 - 5.47 ms alone (profiles/r19), at the price of 0.28 G more vector
// wave-instructions per launch -- and with fewer lines to wait for, those instructions are now the other limit (see the
// note on what binds the kernel, below).  The counting build takes the one-fetch loop WITHOUT the bitmap, so
// seed_table_lookups keeps meaning "lookups that seeds need".  With FILT false nothing of this is compiled in.
// OFF32 (only together with FILT; the launcher takes it while the table and the line of zeros at its end lie below 2^32
// bytes, lrm_sd_off32: the bench text's 2^25 lines are the largest such table): the same three-step loop with fewer vector
// instructions per position -- a line index is one register and a line's address the table's base plus a 32-bit offset
// (sd_filter_issue32, sd_issue_filtered32), the window is cut from the scalar words with shifts whose counts are the same
// in every step, and gather and search are one pass over the slots (sd_finish_quad32).  Results are the same bit for bit;
// the longer tables (up to chr1-sized) keep the FILT loop as it was.  Counts and times: profiles/r20.
template <int SS_ITEMS, bool COUNT, bool SD48, bool FILT = false, bool OFF32 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : 6, 8)))
void seed_search_kernel(LrmIndexView ix, const uint64_t *__restrict__ reads2,
                                                          uint64_t words_per_read,
                                                          const uint32_t *__restrict__ lens,
                                                          const uint8_t *__restrict__ decided, uint64_t n,
                                                          int seed_len, uint32_t thres, int phase_lo, int phase_hi,
                                                          uint32_t cap_q, uint32_t blocks_per_read,
                                                          uint64_t *__restrict__ rec, uint32_t *__restrict__ recq,
                                                          uint32_t *__restrict__ gcnt, uint32_t *__restrict__ ghits,
                                                          LrmDevCounters *counters) {
    __shared__ uint64_t s_rec[SS_ITEMS + 64];
    __shared__ uint32_t s_traffic[3];
    uint32_t my_cnt[2] = {0, 0}, my_seeds = 0;
    if (COUNT && threadIdx.x < 3) s_traffic[threadIdx.x] = 0;
    __shared__ uint32_t s_q[SS_ITEMS + 64];
    __shared__ uint64_t s_tot[64];
    __shared__ uint32_t s_base[64];
    const uint64_t read = blockIdx.x / blocks_per_read;
    const uint32_t chunk = blockIdx.x % blocks_per_read;
    if (read >= n) return;
    if (decided && decided[read]) return;
    const int P = seed_len + 1;
    const uint32_t np = (uint32_t) (phase_hi - phase_lo + 1);
    const uint32_t cap_pp = SS_ITEMS / np + 1;                 // survivors of one phase in one workgroup
    const uint32_t tid = threadIdx.x;
    if (tid < np) s_tot[tid] = 0;
    __syncthreads();
    // iter fastest: neighbouring seeds overlap, so they share their fate (a sequencing error kills ~20 consecutive
    // seeds, a clean stretch lets all of them run the full backward extension): wavefronts diverge little.
    // Measured alternatives that lost: q fastest (+26 %), lane refill from a work chunk (+13 %), packing the
    // survivors of the table lookup into fewer wavefronts (+8 %), and searching 2 / 4 of the lane's seeds TOGETHER
    // (independent chains per lane, all rank gathers of a step in flight at once: 43.4 / 56.7 ms per step against
    // 29.0 [r2]): a wavefront of one-seed lanes stops as soon as its 64 neighbouring seeds are dead, a wavefront of
    // interleaved chains runs until its longest chain ends.  What bound THAT kernel [r2] was the memory system's rate of
    // random requests (56 G 64-byte L2 misses per second on the small text): neither more resident wavefronts (see
    // SS_ITEMS) nor fewer vector instructions (7.1 -> 5.0 G per Gbp with C[] folded into the occ prefixes and the
    // scalar window loads: -2.5 %) moved it much.  That no longer holds for vector instructions: behind the seed table
    // and the bitmap of its lines the kernel alone runs at 92 % of the random-line rate AND at 93 % of the integer issue
    // rate bench.py assumes (3.09 G wave-instructions in 5.4 ms), and in the three-stream step, where the extension's and
    // the vote's instructions share the SIMDs with it, a vector instruction here has a measured price: 0.45 ms of the
    // step per G wave-instructions (profiles/r20, section 0).  Hence the OFF32 form below.  Also measured [r2]: a
    // 2 MiB presence bitmap of the 12-mers in front of the table lookup (57 % of the seeds die on an L2 hit instead of
    // fetching a table line): 27.3 vs 27.5 ms, not kept; non-temporal loads for the one-touch table lines: 31.7 ms.
    // (That bitmap stood in front of ANOTHER kernel: a seed that passed its first lookup went on to about 4.4 dependent
    // rank requests, a wavefront lasted as long as its longest chain, and killing lanes one step earlier shortened
    // nothing.  Since the seed table every seed costs exactly one line and a wavefront iteration is one fetch, so the r2
    // figure does not answer the question for this kernel: see FILT above, which is measured on it.)
    const uint32_t len = lens[read];
    const uint32_t jl = len > (uint32_t) seed_len ? len - (uint32_t) seed_len : 0;   // alnmain.c:353 (fenced for len<s)
    const uint64_t *words = reads2 + read * words_per_read;
    // When (nearly) all phases run in one launch the 64 lanes of a wavefront hold (nearly) consecutive read positions:
    // their 32-base windows lie inside six consecutive words of the packed read, which the wavefront fetches with
    // SCALAR loads (one request per wavefront through the scalar cache instead of 64 lane requests through the
    // texture path) and every lane cuts its window out with selects and a funnel shift.
    const bool dense_lanes = (uint32_t) P - np <= 1u;
    const bool shared_lines = ix.sd && seed_len == ix.sd_len && np == (uint32_t) P && phase_lo == 0;
    LrmIndexView ix_nosd = ix;
    ix_nosd.sd = nullptr;
    LrmIndexView ixs = ix;                                        // the seed table as the shared-lines loop sees it
    if (SD48) { ixs.sd_f = 4; ixs.sd_slot = 8; }
    if (shared_lines) {
        // All phases in this launch: a lane's item IS its read position j, lane id == j mod sd_f, and the lanes that share a
        // line of the seed table fetch it together (sd_issue_shared): every lane of the wavefront stays in until the line is
        // in registers.
        const uint32_t lim = jl < cap_q * np ? jl : cap_q * np;                                     // positions with a seed
        const uint32_t np_inv = 0xFFFFFFFFu / np;
        const uint64_t smask = (1ull << (2 * seed_len)) - 1ull;
        // (q, ph) = (j / np, j % np) of the lane's position: worked out once (no division: a multiply-high and two fix-ups),
        // then carried -- j grows by 256 per iteration, so by 256 / np and 256 % np with one wrap
        const uint32_t dq = 256u / np, dph = 256u % np;
        uint32_t q = __umulhi(chunk * SS_ITEMS + tid, np_inv), ph = chunk * SS_ITEMS + tid - q * np;
        if (ph >= np) { ++q; ph -= np; }
        if (ph >= np) { ++q; ph -= np; }
        // The loop is software-pipelined, two line fetches in flight per lane: a step starts the fetch of the NEXT position
        // (look: cut the window, work out the key, sd_issue_shared) and then searches the line of its own (take).  The two
        // fetches land in two sets of registers that change roles -- a copy of a fetch's registers would have to wait for the
        // fetch -- so the loop body is written out for both.  The number of iterations is wave-uniform (j0 is lane 0's
        // position, a multiple of 64, and positions only grow), and the loop leaves at its end only: every lane of the
        // wavefront takes part in every fetch, and the count of fetches in flight is the same on every path, which is what
        // lets the compiler wait for the older of two (a fetch past the last iteration reads line 0 and is never looked at).
        const uint32_t lane_rel = tid & 63u;
        struct Look { uint64_t code; SdKey key; ulonglong2 a, b; bool have, real; uint32_t word, bit, line; };
        auto look = [&](bool real, uint32_t j, uint32_t j0) {
            Look f;
            f.have = real && j < lim;
            f.code = 0;
            f.key.line = 0; f.key.tag = 0; f.key.tb = 0;
            if (real) {
                const uint64_t *wp = words + (j0 >> 5);                                            // wave-uniform address: scalar loads
                const uint64_t W0 = wp[0], W1 = wp[1], W2 = wp[2];
                if (OFF32) {
                    // rel is the lane id (j0 is lane 0's position and a multiple of 64), so the two shift counts are the
                    // same in every step; and the words are scalars, which a shift takes as they are and a select does
                    // not: both halves of the wavefront's window are cut and ONE select follows, where selects of the
                    // words in front of the shifts cost a register copy per scalar (profiles/r20)
                    const uint32_t sh = (lane_rel & 31u) * 2u;
                    const uint64_t c0 = (W0 >> sh) | ((W1 << 1) << (63 - sh)), c1 = (W1 >> sh) | ((W2 << 1) << (63 - sh));
                    f.code = f.have ? (lane_rel < 32u ? c0 : c1) & smask : 0ull;
                } else {
                const uint32_t rel = j - j0, sh = (rel & 31u) * 2u;
                const uint64_t lo = rel < 32u ? W0 : W1, hi = rel < 32u ? W1 : W2;
                f.code = f.have ? ((lo >> sh) | ((hi << 1) << (63 - sh))) & smask : 0ull;
                }
                f.key = sd_key_of(ixs, f.code, j & (uint32_t) (ixs.sd_f - 1));
            }
            if (SD48) __builtin_assume(f.key.tb <= 32u);
            f.real = real;
            if (FILT && OFF32) f.word = sd_filter_issue32(ixs, f.key, f.bit, f.line);
            else if (FILT) f.word = sd_filter_issue(ixs, f.key, real, f.bit);
            else sd_issue_shared(ixs, f.key, f.a, f.b);
            if (SD48) __builtin_amdgcn_sched_barrier(0);          // the fetch leaves BEFORE the search that follows waits for the one before it
            return f;
        };
        uint32_t j = chunk * SS_ITEMS + tid;
        uint32_t j0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) (j & ~63u));                  // lane 0's position
        auto take = [&](const Look &f) {
            uint64_t k = 0, l = 0, c = 0, rr;
            const int st = OFF32 ? sd_finish_quad32(ixs, f.key, f.code, f.a, k, c)
                                 : sd_finish_shared(ixs, f.key, f.code, f.a, f.b, k, c, COUNT ? my_cnt : nullptr);
            if (f.have) {
                if (st == 1) rr = c;
                else if (st == 0) rr = 0;
                else rr = seed_one(ix_nosd, f.code, seed_len, j, k, l, COUNT ? my_cnt : nullptr);     // (a count beyond 24 bits)
                if (COUNT) my_seeds++;
                if (rr > 0 && rr < (uint64_t) thres) ss_append(s_tot, s_rec, s_q, cap_pp, ph, q, k, rr);
            }
        };
        auto step = [&]() {
            j += 256u; j0 += 256u;
            q += dq; ph += dph;
            if (ph >= np) { ++q; ph -= np; }
        };
        if (j0 < lim) {
            const uint32_t left = (lim - j0 + 255u) >> 8;                                          // iterations with a position below lim
            const uint32_t n_it = left < (uint32_t) (SS_ITEMS / 256) ? left : (uint32_t) (SS_ITEMS / 256);
            if (FILT) {
                // Behind the bitmap a position goes through THREE steps: look (as above, but what it starts is the load of the
                // bitmap word), fetch (with the word in hand, the line fetch: sd_issue_filtered) and take.  Per iteration for
                // position j: the word load of j + 512 leaves, the word of j + 256 is waited for and its line fetch leaves, the
                // line of j is waited for and searched.  Loads retire in the order they were issued, and at either wait two
                // younger ones are out, so both waits are for "all but two".  The words land in two registers and the lines in two
                // sets that change roles, as above; keys and codes are carried from step to step by moves, which wait for nothing.
                // (the two offsets of the 32-bit form, pinned in registers before the loop: left to itself the compiler copies
                //  a scalar into a register in front of every select)
                uint32_t piece = (tid & 3u) * 16u, zpiece = (64u << ixs.sd_bits) + piece;
                if (OFF32) asm volatile("" : "+v"(piece), "+v"(zpiece));
                auto fetch = [&](Look f) {
                    if (OFF32) sd_issue_filtered32(ixs, f.real, f.word, f.bit, f.line, piece, zpiece, f.a, f.b);
                    else sd_issue_filtered(ixs, f.key, f.real, f.word, f.bit, f.a, f.b);
                    __builtin_amdgcn_sched_barrier(0);
                    return f;
                };
                Look pa = look(true, j, j0), pb = look(1 < n_it, j + 256u, j0 + 256u);
                Look ga = fetch(pa), gb;
                uint32_t it = 0;
#pragma unroll 1
                do {
                    pa = look(it + 2 < n_it, j + 512u, j0 + 512u);
                    gb = fetch(pb);
                    take(ga);
                    step();
                    pb = look(it + 3 < n_it, j + 512u, j0 + 512u);
                    ga = fetch(pa);
                    if (it + 1 < n_it) take(gb);
                    step();
                    it += 2;
                } while (it < n_it);
            } else if (SD48) {
                Look fa = look(true, j, j0), fb;
                uint32_t it = 0;
#pragma unroll 1
                do {
                    fb = look(it + 1 < n_it, j + 256u, j0 + 256u);
                    take(fa);
                    step();
                    fa = look(it + 2 < n_it, j + 256u, j0 + 256u);
                    if (it + 1 < n_it) take(fb);
                    step();
                    it += 2;
                } while (it < n_it);
            } else {
                // The other table forms (two 16-byte requests per fetch, 6-byte slots) keep one fetch in flight: on the
                // GRCh38-sized text two were 0.8 % slower in the bench (profiles/r13, section 6).
#pragma unroll 1
                for (uint32_t it = 0; it < n_it; ++it) {
                    const Look f = look(true, j, j0);
                    take(f);
                    step();
                }
            }
        }
    } else {
    const uint32_t np_inv_g = 0xFFFFFFFFu / np;
#pragma unroll 1
    for (uint32_t it = 0; it < SS_ITEMS / 256; ++it) {
        const uint32_t item = chunk * SS_ITEMS + it * 256 + tid;
        uint32_t q = __umulhi(item, np_inv_g), ph = item - q * np;             // item / np, item % np without a division
        if (ph >= np) { ++q; ph -= np; }
        if (ph >= np) { ++q; ph -= np; }
        uint64_t W[6] = {0, 0, 0, 0, 0, 0};
        uint32_t jw = 0;                                                       // first base of W[0]
        if (dense_lanes) {
            const uint32_t item0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) (item & ~63u));   // lane 0's item
            const uint32_t q0 = item0 / np;
            if (q0 < cap_q) {
                const uint32_t j0 = (uint32_t) phase_lo + item0 % np + q0 * (uint32_t) P;
                const uint64_t *wp = words + (j0 >> 5);                        // wave-uniform address
                jw = j0 & ~31u;
#pragma unroll
                for (int e = 0; e < 6; ++e) W[e] = wp[e];
            }
        }
        if (q >= cap_q) break;
        const uint32_t j = (uint32_t) phase_lo + ph + q * (uint32_t) P;        // < 2^32: cap_q * P <= max_len + P
        if (j >= jl) continue;
        uint64_t win, k, l;
        if (dense_lanes) {
            const uint32_t rel = j - jw, wi = rel >> 5, sh = (rel & 31u) * 2u;  // rel <= 31 + 63 + 4: wi in 0..3
            const uint64_t lo = wi == 0 ? W[0] : wi == 1 ? W[1] : wi == 2 ? W[2] : wi == 3 ? W[3] : W[4];
            const uint64_t hi = wi == 0 ? W[1] : wi == 1 ? W[2] : wi == 2 ? W[3] : wi == 3 ? W[4] : W[5];
            win = (lo >> sh) | ((hi << 1) << (63 - sh));
        } else {
            win = read_window(words, j);
        }
        const uint64_t rr = seed_one(ix, win, seed_len, j, k, l, COUNT ? my_cnt : nullptr);
        if (COUNT) my_seeds++;
        if (rr > 0 && rr < (uint64_t) thres) ss_append(s_tot, s_rec, s_q, cap_pp, ph, q, k, rr);
    }
    }
    if (COUNT) { atomicAdd(&s_traffic[0], my_seeds); atomicAdd(&s_traffic[1], my_cnt[0]); atomicAdd(&s_traffic[2], my_cnt[1]); }
    __syncthreads();
    if (COUNT && tid < 3) atomicAdd(&counters->seed_traffic[tid], (unsigned long long) s_traffic[tid]);
    if (tid < np) {
        const uint64_t tot = s_tot[tid];                                   // survivors | sum of rr << 32
        const uint32_t c = (uint32_t) tot;
        if (c) {
            const uint64_t id = read * (uint64_t) P + (uint64_t) (phase_lo + (int) tid);
            s_base[tid] = atomicAdd(&gcnt[id], c);
            atomicAdd(&ghits[id], (uint32_t) (tot >> 32));
        }
    }
    __syncthreads();
    // Write-out by phase: a wavefront takes whole lists, so a list's length, its place in LDS and its place in the global
    // list are the same for all 64 lanes (scalar registers), and a lane copies slots lane, lane + 64, ... with nothing per
    // entry but two LDS reads and two stores.  Lane ph keeps count and global base of phase ph (np <= 64).  With fewer than
    // four lists (np = 1: up to SS_ITEMS entries in one) the four wavefronts share every list instead.
    const uint32_t lane = tid & 63u, wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (tid >> 6));
    const uint32_t cnt_l = lane < np ? (uint32_t) s_tot[lane] : 0u;
    const uint32_t base_l = lane < np && cnt_l ? s_base[lane] : 0u;
    const bool share = np < 4u;
    for (uint32_t ph = share ? 0u : wave; ph < np; ph += share ? 1u : 4u) {
        const uint32_t c = (uint32_t) __builtin_amdgcn_readlane((int) cnt_l, (int) ph);
        const uint64_t o = (read * (uint64_t) P + (uint64_t) (phase_lo + (int) ph)) * cap_q + (uint32_t) __builtin_amdgcn_readlane((int) base_l, (int) ph);
        uint64_t *rec_o = rec + o;
        uint32_t *recq_o = recq + o;
        const uint32_t lb = ph * cap_pp;
        for (uint32_t sl = share ? tid : lane; sl < c; sl += share ? 256u : 64u) {
            rec_o[sl] = s_rec[lb + sl];
            recq_o[sl] = s_q[lb + sl];
        }
    }
}

// debug tap: full (j, rr, k, l) per seed of one read, in (iter, q) order
__global__ __launch_bounds__(256) void seed_search_debug_kernel(LrmIndexView ix, const uint64_t *__restrict__ words,
                                                                uint32_t len, int seed_len, uint32_t cap_q,
                                                                int32_t *j_out, uint64_t *rr_out, uint64_t *k_out,
                                                                uint64_t *l_out) {
    const int P = seed_len + 1;
    uint32_t item = blockIdx.x * 256 + threadIdx.x;
    uint32_t iter = item / cap_q, q = item % cap_q;
    if (iter >= (uint32_t) P) return;
    uint32_t jl = len > (uint32_t) seed_len ? len - (uint32_t) seed_len : 0;
    uint64_t j = (uint64_t) iter + (uint64_t) q * (uint64_t) P;
    uint64_t o = (uint64_t) iter * cap_q + q;
    if (j >= jl) { j_out[o] = -1; return; }
    uint64_t win = read_window(words, (uint32_t) j);
    uint64_t k, l;
    uint64_t rr = seed_one(ix, win, seed_len, (uint32_t) j, k, l);
    j_out[o] = (int32_t) j; rr_out[o] = rr; k_out[o] = k; l_out[o] = l;
}


// ----------------------------------------------------------------------------------------
// decide: replay of alnmain.c:371-403 over the per-phase vote results.
//   mode 0 : phase 0 only -- mark reads whose phase-0 vote passes (they are final)
//   mode 1 : all phases, for reads not marked in mode 0
//   mode 2 : all phases for every read (single-round launches); counts the reads mode 0 would have marked
// phase_out (optional, every mode): the phase at which the loop broke, P - 1 when it ran out -- the evidence phases of
// the mapping-quality vote (mapq_kernels.hip).
// (double)v/num_seeds > 0.6  <=>  5v > 3*num_seeds for every feasible size.
// ----------------------------------------------------------------------------------------
#define MAX_PHASES 40
__global__ __launch_bounds__(256) void decide_kernel(const LrmPhaseRes *__restrict__ phase_res,
                                                     const uint32_t *__restrict__ lens, uint64_t n,
                                                     int seed_len, int mode, uint8_t *__restrict__ decided,
                                                     lrm_entry *__restrict__ best, LrmDevCounters *counters,
                                                     uint8_t *__restrict__ phase_out) {
    uint64_t read = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (read >= n) return;
    const int P = seed_len + 1;
    const uint64_t num_seeds = lens[read] / (uint32_t) P;          // alnmain.c:371
    const LrmPhaseRes *pr = phase_res + read * (uint64_t) P;
    if (mode == 0) {
        uint8_t d = 0;
        if (num_seeds > 0 && P > 1) {       // a break on the LAST phase is undone (alnmain.c:400): P==1 never final here
            LrmPhaseRes r0 = pr[0];
            uint64_t v = r0.val1 + r0.val2;
            if (5 * v > 3 * num_seeds) {
                d = 1;
                lrm_entry e = {r0.key1, r0.val1, r0.bucket1};
                best[read] = e;
                if (phase_out) phase_out[read] = 0;
                atomicAdd(&counters->decided_phase0, 1ull);
            }
        }
        decided[read] = d;
        return;
    }
    if (mode == 1 && decided[read]) return;
    // ot_iter_histo (alnmain.c:340,386-388,400-403): at most P entries
    uint64_t ot_key[MAX_PHASES], ot_val[MAX_PHASES], ot_bucket[MAX_PHASES];
    int ot_n = 0;
    lrm_entry out = {0, 0, 0};
    int iter;
    for (iter = 0; iter < P; ++iter) {
        if (num_seeds > 0) {
            LrmPhaseRes r = pr[iter];
            uint64_t v = r.val1 + r.val2;
            if (5 * v > 3 * num_seeds) {
                out.key = r.key1; out.val = r.val1; out.bucket = r.bucket1;
                if (mode == 2 && iter == 0 && P > 1) atomicAdd(&counters->decided_phase0, 1ull);
                break;
            } else if (r.val1 != 0) {
                uint64_t key = r.key1, bucket = key >> 4;
                bool found = false;
                for (int t = 0; t < ot_n; ++t) {
                    if (ot_bucket[t] == bucket) {
                        found = true;
                        ot_val[t] += 1;
                        if (key < ot_key[t]) ot_key[t] = key;
                    }
                }
                if (!found) { ot_key[ot_n] = key; ot_val[ot_n] = 1; ot_bucket[ot_n] = bucket; ot_n++; }
            }
        }
    }
    if (iter >= P - 1) {       // ran out, or broke on the last phase: winner comes from ot_iter_histo
        lrm_entry t1 = {0, 0, 0};
        for (int t = 0; t < ot_n; ++t)
            if (t1.val < ot_val[t]) { t1.key = ot_key[t]; t1.val = ot_val[t]; t1.bucket = ot_bucket[t]; }
        out = t1;
    }
    best[read] = out;
    if (phase_out) phase_out[read] = (uint8_t) (iter < P ? iter : P - 1);      // the deciding phase (docs/GACT_SPEC.md, "Mapping quality")
}

// ----------------------------------------------------------------------------------------
// host launchers
// ----------------------------------------------------------------------------------------

int lrm_launch_seed(lrm_index *idx, lrm_workspace *ws, const char *d_reads, uint64_t stride,
                    const uint32_t *d_lens, uint64_t n, uint32_t seed_len,
                    uint32_t thres, lrm_entry *d_best, const LrmMapTune &mt, void *stream_, uint8_t *d_phase_out) {
    hipStream_t stream = (hipStream_t) stream_;
    if (n == 0) return 0;
    // from here on the survivor lists are no batch's (a call that fails half-way leaves them so); set again at the end
    ws->seeded_best = nullptr; ws->seeded_n = 0; ws->seeded_phase = 0;
    const int P = (int) seed_len + 1;
    const uint32_t cap_q = ws->cap_q;
    const uint64_t wpr = ws->words_per_read;

    HIPCHK(hipMemsetAsync(ws->d_counters, 0, sizeof(LrmDevCounters), stream));
    HIPCHK(hipMemsetAsync(ws->d_hcount, 0, n * (uint64_t) P * 4, stream));
    HIPCHK(hipMemsetAsync(ws->d_cnt, 0, n * (uint64_t) P * 4, stream));
    ws->n_last = n;
    {
        uint64_t bpr = wpr * 8;
        uint32_t cpr = (uint32_t) ((bpr / 4 + 255) / 256);
        uint32_t grid;
        if (lrm_grid_1d(n * cpr, "pack2bit", &grid)) return -1;
        lrm_time_begin(ws, LRM_K_PACK2BIT, stream);
        hipLaunchKernelGGL(pack2bit_kernel, dim3(grid), dim3(256), 0, stream, d_reads, stride,
                           d_lens, (uint8_t *) ws->d_reads2, bpr, cpr, n);
        lrm_time_end(ws, stream);
    }
    uint32_t tbits = 1;
    while ((1u << tbits) < thres && tbits < 31) tbits++;
    if (((uint64_t) cap_q << tbits) > 0xffffffffull) {
        lrm_set_error("read too long for the vote order key: cap_q %u << %u bits exceeds 32 bits", cap_q, tbits);
        return -1;
    }
    // Rounds.  Phase 0 alone first, then phases 1..s for the reads it did not decide, saves 20/21 of the work on clean
    // reads; on noisy reads phase 0 decides nothing and the split only costs a second set of launches whose phase-0
    // wavefronts hold seeds 21 positions apart (no shared fate).  The workspace remembers how many reads the previous
    // batch decided in phase 0 (copied back asynchronously, never waited for): below 2 % the next batch runs ALL phases
    // in one round.  Speculative evaluation is exact, so the results do not depend on the choice.  lrm_map_options.seed_rounds.
    bool single = false;
    {
        const volatile uint64_t *hist = reinterpret_cast<const volatile uint64_t *>(ws->h_err + 2);
        const uint64_t d0 = *hist;
        if (ws->hist_n >= 64 && d0 * 50 < ws->hist_n) single = true;
        if (mt.seed_rounds == 1 || mt.seed_rounds == 2) single = mt.seed_rounds == 1;
        if (P == 1) single = true;
    }
    for (int round = single ? 1 : 0; round < 2; ++round) {
        int lo = round == 0 || single ? 0 : 1;
        int hi = round == 0 ? 0 : P - 1;
        if (lo > hi) break;
        int np = hi - lo + 1;
        const uint8_t *dec = round == 0 || single ? nullptr : ws->d_decided;
        const uint32_t ss_items = mt.ss_items;
        uint32_t bpr = (uint32_t) (((uint64_t) np * cap_q + ss_items - 1) / ss_items);
        uint32_t grid;
        if (lrm_grid_1d(n * bpr, "seed_search", &grid)) return -1;
        lrm_time_begin(ws, LRM_K_SEED_SEARCH, stream);
        const LrmIndexView &v = idx->view;
        const bool sd48 = lrm_sd48_form(v);
        const bool filt = sd48 && v.sd_filt;
        const bool off32 = filt && lrm_sd_off32(v);               // (the bench text: 2^25 lines)
        auto sk = ws->counting ? seed_search_kernel<2048, true, false>
                  : off32 ? (ss_items == 1024u ? seed_search_kernel<1024, false, true, true, true> : ss_items == 4096u ? seed_search_kernel<4096, false, true, true, true> : seed_search_kernel<2048, false, true, true, true>)
                  : filt ? (ss_items == 1024u ? seed_search_kernel<1024, false, true, true> : ss_items == 4096u ? seed_search_kernel<4096, false, true, true> : seed_search_kernel<2048, false, true, true>)
                  : sd48 ? (ss_items == 1024u ? seed_search_kernel<1024, false, true> : ss_items == 4096u ? seed_search_kernel<4096, false, true> : seed_search_kernel<2048, false, true>)
                         : (ss_items == 1024u ? seed_search_kernel<1024, false, false> : ss_items == 4096u ? seed_search_kernel<4096, false, false> : seed_search_kernel<2048, false, false>);
        if (ws->counting) bpr = (uint32_t) (((uint64_t) np * cap_q + 2047) / 2048);
        if (ws->counting) grid = (uint32_t) (n * bpr);
        // (mt.ss_lds_pad: extra dynamic LDS per workgroup, i.e. fewer resident workgroups per CU -- see DESIGN 5)
        hipLaunchKernelGGL(sk, dim3(grid), dim3(256), mt.ss_lds_pad, stream, idx->view,
                           ws->d_reads2, wpr, d_lens, dec, n, (int) seed_len, thres, lo, hi, cap_q, bpr,
                           ws->d_rec, ws->d_recq, ws->d_cnt, ws->d_hcount, ws->d_counters);
        lrm_time_end(ws, stream);
        const LrmVoteLaunch vl = {dec, n, seed_len, lo, hi, tbits, round, &mt};
        if (lrm_launch_vote(idx, ws, vl, stream)) return -1;
        lrm_time_begin(ws, LRM_K_DECIDE, stream);
        hipLaunchKernelGGL(decide_kernel, dim3((uint32_t) ((n + 255) / 256)), dim3(256), 0, stream, ws->d_phase,
                           d_lens, n, (int) seed_len, single ? 2 : round, ws->d_decided, d_best, ws->d_counters, d_phase_out);
        lrm_time_end(ws, stream);
    }
    HIPCHK(hipMemcpyAsync((void *) (ws->h_err + 2), &ws->d_counters->decided_phase0, 8, hipMemcpyDeviceToHost, stream));
    ws->hist_n = n;
    HIPCHK(hipGetLastError());
    ws->seeded_best = d_best; ws->seeded_n = n;
    ws->seeded_phase = d_phase_out != nullptr && d_phase_out == ws->d_mq_phase;     // (what mapq and rival read is d_mq_phase)
    return 0;
}

int lrm_launch_debug_seed(lrm_index *idx, const char *d_read, uint32_t len, uint32_t seed_len,
                          uint64_t *d_reads2, uint64_t words, int32_t *d_j, uint64_t *d_rr,
                          uint64_t *d_k, uint64_t *d_l, uint64_t cap, void *stream_) {
    hipStream_t stream = (hipStream_t) stream_;
    const uint32_t P = seed_len + 1;
    uint32_t jl = len > seed_len ? len - seed_len : 0;
    uint32_t cap_q = (jl + P - 1) / P;
    if (cap_q == 0) cap_q = 1;
    if ((uint64_t) cap_q * P > cap) { lrm_set_error("debug seed buffer too small"); return -1; }
    uint64_t bpr = words * 8;
    uint32_t cpr = (uint32_t) ((bpr / 4 + 255) / 256);
    uint32_t *d_len1 = (uint32_t *) (d_reads2 + words);     // caller reserves one extra word for the length
    HIPCHK(hipMemcpyAsync(d_len1, &len, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(pack2bit_kernel, dim3(cpr), dim3(256), 0, stream, d_read, (uint64_t) 0, d_len1,
                       (uint8_t *) d_reads2, bpr, cpr, (uint64_t) 1);
    uint32_t items = cap_q * P;
    hipLaunchKernelGGL(seed_search_debug_kernel, dim3((items + 255) / 256), dim3(256), 0, stream, idx->view,
                       d_reads2, len, (int) seed_len, cap_q, d_j, d_rr, d_k, d_l);
    HIPCHK(hipGetLastError());
    return (int) cap_q;
}
