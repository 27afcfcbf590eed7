// seed_index_dev.h -- the device-side contract of the index tables: what the builders (index_tables.hip) write and the
// seed search (seed_kernels.hip) reads.  seed_one is here because the seed table is built THROUGH it: sd_build_kernel
// searches every S-mer of the text as a seed would be, through the tables the handle already has.
#pragma once
#include "lrm_hip_util.h"

// A/a=0 C/c=1 G/g=2 T/t=3 ; other bytes are fenced (UB in the reference, lchash.c:38-44)
__device__ __forceinline__ uint32_t base_code(uint32_t c) { return ((c >> 1) ^ (c >> 2)) & 3u; }

// (the LF step occ_lf_of, sa_locate and sa_of_unique live in lrm_hip_util.h: the mapping-quality vote gathers the same rows)
// the two LF values of one backward step; after the table lookup most intervals are a handful of rows,
// so k-1 and l usually fall into the same 64-row block and ONE 16-byte request serves both
// (returns the number of 16-byte requests it made: 1 or 2 -- only the counting build of seed_search looks at it)
__device__ __forceinline__ uint32_t occ_lf2(const LrmIndexView &ix, uint32_t c, uint64_t loc_a, uint64_t loc_b,
                                            uint64_t &ra, uint64_t &rb) {
    const ulonglong2 eb = *reinterpret_cast<const ulonglong2 *>(&ix.occ[loc_b >> 6].sym[c]);
    ulonglong2 ea = eb;
    const bool two = (loc_a >> 6) != (loc_b >> 6);
    if (two) ea = *reinterpret_cast<const ulonglong2 *>(&ix.occ[loc_a >> 6].sym[c]);
    ra = occ_lf_of(ea, loc_a);
    rb = occ_lf_of(eb, loc_b);
    return two ? 2u : 1u;
}

// lc_access (lchash.c:12-16) on the 8-byte device entries
__device__ __forceinline__ void lc_lookup(const LrmIndexView &ix, uint64_t code, uint64_t &k, uint64_t &l) {
    const uint64_t e = ix.lc[code];
    k = e & ((1ull << 40) - 1ull);
    const uint64_t cnt = e >> 40;
    l = k + cnt - 1;
    if (e == 0) { k = 0; l = 0; }                                // absent hlen-mer
    else if (cnt == 0xFFFFFFull) {                               // interval too long for 24 bits: side table
        uint64_t lo = 0, hi = ix.n_lcx;
        while (lo < hi) { uint64_t mid = (lo + hi) >> 1; if (ix.lcx[3 * mid] < code) lo = mid + 1; else hi = mid; }
        k = ix.lcx[3 * lo + 1];
        l = ix.lcx[3 * lo + 2];
    }
}

// ----------------------------------------------------------------------------------------
// SEED table: the whole of lc_aln + fmi_aln for a seed of sd_len bases in ONE memory line that the seeds of sd_f
// neighbouring read positions share.
//   The seeds at read positions p0 .. p0 + F - 1 (p0 a multiple of F = sd_f) share the CORE [p0 + F - 1, p0 + S): S - F + 1
//   bases.  A bijective hash of the core gives the line (its top sd_bits bits) and a residue (the rest); a slot of the line
//   is { k, count, tag } with tag = the seed's role r = p - p0, its F - 1 bases outside the core and the residue -- so a tag
//   names one S-mer exactly, and a lookup that finds no slot with its tag has proved the S-mer absent from the text
//   (rr = 0), which is how most seeds of a noisy read end.  Every distinct S-mer of the text is entered once per role with
//   the (k, l - k + 1) a real search gave for it (sd_build_kernel), so the table IS the reference's result, also where the
//   reference has a quirk (the '$' row).
//   8-byte slots (eight per line): k in the low sd_kbits bits, the count above, bit 63 - tagbits of slot 0 = "line
//   overflowed", the tag in the top bits.  6-byte slots (ten per line, texts of >= 2^32 rows): k | count << kbits | tag
//   << (48 - tagbits), the last four bytes of the line count its entries (> 10: overflowed).
//   Entries that found no room, and counts of all ones, are in a side hash table keyed by the S-mer.
// ----------------------------------------------------------------------------------------
struct SdKey { uint64_t line; uint64_t tag; uint32_t tb; };
// (The kernel that looks seeds up here is bound by its VECTOR INSTRUCTIONS once a seed costs a quarter of a line -- 3.95 G
//  wave-instructions per Gbp in 8.0 ms with a 64-bit multiplicative hash, 64-bit tag compares and a division per seed --
//  so the hash is ONE 32-bit multiply: the low 32 bits of the core times an odd constant (a bijection of those bits whose
//  TOP bits depend on all of them: they index the line), the bits of the core above 32 xor-ed with low bits of the product.)
__device__ __forceinline__ SdKey sd_key_of(const LrmIndexView &ix, uint64_t code, uint32_t r) {
    const uint32_t lf = ix.sd_f == 4 ? 2u : 1u, F = 1u << lf, lo_n = F - 1u - r;
    const uint32_t CL2 = 2u * ((uint32_t) ix.sd_len - F + 1u), wlo = CL2 < 32u ? CL2 : 32u;
    const uint64_t core = (code >> (2u * lo_n)) & ((1ull << CL2) - 1ull);
    const uint32_t extra = (uint32_t) (code & ((1ull << (2u * lo_n)) - 1ull)) | ((uint32_t) (code >> (2u * lo_n + CL2)) << (2u * lo_n));
    uint32_t m = (uint32_t) core * 0x9E3779B1u;
    if (wlo < 32u) m &= (1u << wlo) - 1u;
    const uint32_t chi = ((uint32_t) (core >> 32) ^ m) & ((1u << (CL2 - wlo)) - 1u);          // (0 when the core has <= 32 bits)
    const uint32_t rb = CL2 - (uint32_t) ix.sd_bits;                                          // < 32: sd_plan keeps sd_bits > CL2 - 32
    SdKey key;
    key.line = ((uint64_t) chi << (wlo - rb)) | (uint64_t) (m >> rb);
    key.tb = lf + 2u * (F - 1u) + rb;
    key.tag = (uint64_t) (r | (extra << lf)) | ((uint64_t) (m & ((1u << rb) - 1u)) << (lf + 2u * (F - 1u)));
    return key;
}
__device__ __forceinline__ uint32_t sd_filter_bit(uint32_t tag) { return (((tag * 0x9E3779B1u) >> 27) * 24u) >> 5; }   // 0 .. 23
// side table: true + entry (k | count << 40) when the S-mer is there
__device__ __forceinline__ bool sd_side_lookup(const LrmIndexView &ix, uint64_t code, uint64_t &e) {
    uint64_t slot = (code * 0x9E3779B97F4A7C15ull) >> 20 & ix.sdx_mask;
    for (;;) {
        const ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(ix.sdx + 2 * slot);
        if (x.x == code + 1) { e = x.y; return true; }
        if (x.x == 0) return false;
        slot = (slot + 1) & ix.sdx_mask;
    }
}
// search of a fetched line.  0: absent (rr = 0); 1: k, c set; 2: take the other tables (a count beyond 24 bits)
// Slots fill from the front and an empty slot is all zeros, so the search runs from the LAST slot to the first with
// `e = match ? slot : e`: an empty slot can only "match" a tag of zero, a real entry before it overrides it, and e == 0 in
// the end means "not there".  The tag sits in the top bits of a slot: 32-bit compares on the high dword (8-byte slots, tags
// of <= 32 bits) or on the third halfword (6-byte slots, tags of <= 16 bits: the 2^31-line table of a GRCh38-sized text).
// sd_answer: what the slot found (e, 0 for none) and the line's overflow mark say -- 0: absent (rr = 0); 1: k, c set; 2: take
// the other tables.  The second half of sd_search; seed_search's loop behind the bitmap finds e in its own way.
__device__ __forceinline__ int sd_answer(const LrmIndexView &ix, uint64_t code, uint64_t e, bool ovf, uint64_t &k, uint64_t &c, uint32_t *cnt);
__device__ __forceinline__ int sd_search(const LrmIndexView &ix, const SdKey &key, uint64_t code, const uint64_t (&W)[8],
                                         uint64_t &k, uint64_t &c, uint32_t *cnt) {
    uint64_t e = 0;
    bool ovf;
    if (ix.sd_slot == 8) {
        if (key.tb <= 32u) {
            const uint32_t sh = 32u - key.tb, t32 = (uint32_t) key.tag;
            uint32_t elo = 0, ehi = 0;
#pragma unroll
            for (int i = 7; i >= 0; --i) {
                const uint32_t hi = (uint32_t) (W[i] >> 32);
                const bool m = (hi >> sh) == t32;
                elo = m ? (uint32_t) W[i] : elo;
                ehi = m ? hi : ehi;
            }
            e = (uint64_t) elo | ((uint64_t) ehi << 32);
        } else {
#pragma unroll
            for (int i = 7; i >= 0; --i)
                if ((W[i] >> (64u - key.tb)) == key.tag) e = W[i];
        }
        ovf = (W[0] >> (63u - key.tb)) & 1ull;
    } else {
        uint32_t D[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) { D[2 * i] = (uint32_t) W[i]; D[2 * i + 1] = (uint32_t) (W[i] >> 32); }
        if (key.tb <= 16u) {
            const uint32_t sh = 16u - key.tb, t32 = (uint32_t) key.tag;
            uint32_t elo = 0, ehi = 0;
#pragma unroll
            for (int i = 9; i >= 0; --i) {
                const int h2 = 3 * i + 2;                                              // the slot's third halfword: tag on top
                const uint32_t hw = (h2 & 1) ? D[h2 >> 1] >> 16 : D[h2 >> 1] & 0xFFFFu;
                const uint32_t lo = (i & 1) ? __builtin_amdgcn_alignbit(D[(3 * i + 1) >> 1], D[(3 * i) >> 1], 16) : D[(3 * i) >> 1];
                const bool m = (hw >> sh) == t32;
                elo = m ? lo : elo;
                ehi = m ? hw : ehi;
            }
            e = (uint64_t) elo | ((uint64_t) ehi << 32);
        } else {
#pragma unroll
            for (int i = 9; i >= 0; --i) {
                const int w = (48 * i) >> 6, off = (48 * i) & 63;
                uint64_t v = W[w] >> off;
                if (off > 16) v |= W[w + 1] << (64 - off);
                v &= (1ull << 48) - 1ull;
                if ((v >> (48u - key.tb)) == key.tag) e = v;
            }
        }
        // the line's last word: entry count in the low byte; above it a 24-bit filter of the tags that found no room -- a seed
        // the text does not hold (most seeds of a noisy read) goes on to the side table only when its filter bit is set
        ovf = (D[15] & 0xFFu) > 10u && ((D[15] >> (8u + sd_filter_bit((uint32_t) key.tag))) & 1u);
    }
    return sd_answer(ix, code, e, ovf, k, c, cnt);
}
__device__ __forceinline__ int sd_answer(const LrmIndexView &ix, uint64_t code, uint64_t e, bool ovf, uint64_t &k, uint64_t &c, uint32_t *cnt) {
    const uint64_t cmax = (1ull << ix.sd_cbits) - 1ull;
    if (e != 0) {
        k = e & ((1ull << ix.sd_kbits) - 1ull);
        c = (e >> ix.sd_kbits) & cmax;
        if (c == 0) { k |= LRM_LOCATED_BIT; c = 1; return 1; }        // a unique S-mer: the field is SA[k], not k (sa_of_unique)
        if (c != cmax) return 1;
    } else if (!ovf) {
        return 0;
    }
    uint64_t se;
    if (cnt) cnt[0] += 2;
    if (!sd_side_lookup(ix, code, se)) return e != 0 ? 2 : 0;           // (a saturated count without a side entry: never)
    if ((se >> 40) == 0xFFFFFFull) return 2;
    k = se & ((1ull << 40) - 1ull);
    c = se >> 40;
    return 1;
}
// a lane on its own: the whole line in ONE round trip (four independent 16-byte requests), searched in registers
__device__ __forceinline__ int sd_lookup(const LrmIndexView &ix, uint64_t win, uint32_t jpar, uint64_t &k, uint64_t &c, uint32_t *cnt) {
    const uint64_t code = win & ((1ull << (2 * ix.sd_len)) - 1ull);
    const SdKey key = sd_key_of(ix, code, jpar & (uint32_t) (ix.sd_f - 1));
    const uint64_t *line = ix.sd + key.line * 8;
    const ulonglong2 x0 = *reinterpret_cast<const ulonglong2 *>(line), x1 = *reinterpret_cast<const ulonglong2 *>(line + 2);
    const ulonglong2 x2 = *reinterpret_cast<const ulonglong2 *>(line + 4), x3 = *reinterpret_cast<const ulonglong2 *>(line + 6);
    if (cnt) cnt[0] += 1;
    const uint64_t W[8] = {x0.x, x0.y, x1.x, x1.y, x2.x, x2.y, x3.x, x3.y};
    return sd_search(ix, key, code, W, k, c, cnt);
}

// lc_aln (lchash.c:89-104) + fmi_aln (fmidx.c:295-313) on the packed read.
// win: bases j.. of the read, 2 bits each, LSB first.  Returns rr; k,l as the reference
// leaves them (also on failure).
// jpar: parity of the seed's read position (only the pair-line layout of the long table looks at it).
// cnt (counting build only): cnt[0] += 8-byte table lookups, cnt[1] += 16-byte rank requests of this seed.
__device__ __forceinline__ uint64_t seed_one(const LrmIndexView &ix, uint64_t win, int seed_len, uint32_t jpar,
                                             uint64_t &k, uint64_t &l, uint32_t *cnt = nullptr) {
    int left = seed_len - ix.hlen;
    bool looked_up = false;
    if (ix.sd && seed_len == ix.sd_len) {
        uint64_t c;
        const int st = sd_lookup(ix, win, jpar, k, c, cnt);
        if (st == 0) { k = 0; l = 0; return 0; }                          // the text does not hold this seed
        if (st == 1) { l = k + c - 1; return c; }
    }
    if (ix.core && seed_len >= 16) {
        // CORE table (small texts): the 16-mers of read positions p0 .. p0 + 3 (p0 a multiple of 4) share the 13 bases
        // [p0 + 3, p0 + 16) of their windows; the line of that 13-mer holds the entries of the text's 16-mers around it
        // (eight 8-byte slots: k | count << 40 | tag << 56, tag = the window's role r = p & 3 and its 3 bases outside
        // the core), so the four lanes read ONE line.  Slots fill from a tag-dependent home pair onwards (no deletions:
        // an empty slot ends the search); a line that would need more than eight slots is all ones: such 16-mers take
        // the pair-line table below.
        const int left2 = seed_len - 16;
        const uint64_t W = (win >> (2 * left2)) & 0xFFFFFFFFull;                        // the seed's last 16 bases, first base lowest
        const uint32_t r = jpar & 3u;
        const uint64_t corec = (W >> (2 * (3 - r))) & ((1ull << 26) - 1ull);
        const uint32_t extra = (uint32_t) (W & ((1ull << (2 * (3 - r))) - 1ull)) | ((uint32_t) (W >> (2 * (16 - r))) << (2 * (3 - r)));
        const uint32_t tag = r | (extra << 2);
        const uint64_t *line = ix.core + corec * 8;
        // The whole line in ONE round trip (four independent 16-byte requests to one 64-byte line), searched in registers.
        // (Measured on the bench workload, ms per Gbp: no core table 15.4-15.7; a search walking the line pair by pair
        //  from a tag-dependent home pair 17.3 -- every step is a dependent round trip for the whole wavefront; the first
        //  half of the line, the second only when the first is full of other 16-mers 14.2 -- the repeat family's lines
        //  are, and some lane of nearly every wavefront sits in one; the whole line at once 13.2.)
        const ulonglong2 x0 = *reinterpret_cast<const ulonglong2 *>(line), x1 = *reinterpret_cast<const ulonglong2 *>(line + 2);
        const ulonglong2 x2 = *reinterpret_cast<const ulonglong2 *>(line + 4), x3 = *reinterpret_cast<const ulonglong2 *>(line + 6);
        if (cnt) cnt[0] += 1;
        const uint64_t sl[8] = {x0.x, x0.y, x1.x, x1.y, x2.x, x2.y, x3.x, x3.y};
        uint64_t e = 0;
        int state = x0.x == ~0ull ? 3 : 2;                               // (an overflowed line is all ones)
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (sl[i] != 0 && sl[i] != ~0ull && (uint32_t) (sl[i] >> 56) == tag) { e = sl[i]; state = 1; }
        if (state != 3) {
            if (state != 1) { k = 0; l = 0; return 0; }                  // dead by its 16th base
            k = e & ((1ull << 40) - 1ull);
            l = k + ((e >> 40) & 0xFFFFull) - 1;
            left = left2;
            looked_up = true;
        }
    }
    if (!looked_up && ix.lcl && seed_len >= ix.hl) {
        // Long table: entry[hl-mer] = lc[hlen-mer] followed by hl - hlen backward steps, precomputed on the device
        // (lcl_build_kernel) -- the same (k, l) the reference reaches after those steps, for one memory request
        // instead of 1 + 2(hl - hlen).  The kernel is bound by the number of requests, and most seeds of a noisy
        // read die inside their last hl bases.
        const int left2 = seed_len - ix.hl;
        uint64_t at = (win >> (2 * left2)) & ((1ull << (2 * ix.hl)) - 1ull);          // the seed's last hl bases, first base lowest
        if (ix.lcl_pair) {
            // PAIR-LINE layout: one 64-byte line per (hl-1)-mer S holds the entries of its four left extensions a.S and
            // of its four right extensions S.b.  The seed at an even read position j looks its hl-mer up as a.S, the seed
            // at j + 1 as S.b with the SAME S (its hl-mer without its last base = the hl-mer of j without its first):
            // the two lanes of neighbouring positions read one line, and the texture path merges them into one request.
            const uint64_t smask = (1ull << (2 * (ix.hl - 1))) - 1ull;
            at = (jpar & 1u) ? ((at & smask) << 3) + 4u + (at >> (2 * (ix.hl - 1)))
                             : ((at >> 2) << 3) + (at & 3u);
        }
        uint64_t e;
        if (ix.lcl_kbits) {
            // 5-byte entries (pair-line layout only: 40 bytes per (hl-1)-mer): k in the low kbits bits, the count above;
            // a count of all ones sends the hl-mer to the side hash table (an 8-byte entry per such hl-mer)
            uint64_t v;
            __builtin_memcpy(&v, reinterpret_cast<const uint8_t *>(ix.lcl) + at * 5, 8);     // one unaligned 8-byte request
            v &= (1ull << 40) - 1ull;
            const uint64_t c5 = v >> ix.lcl_kbits, cmax = (1ull << (40 - ix.lcl_kbits)) - 1ull;
            e = v == 0 ? 0ull : (v & ((1ull << ix.lcl_kbits) - 1ull)) | (c5 << 40);
            if (c5 == cmax) {
                const uint64_t code = (win >> (2 * left2)) & ((1ull << (2 * ix.hl)) - 1ull);
                uint64_t slot = (code * 0x9E3779B97F4A7C15ull) >> 20 & ix.lclx_mask;
                for (;;) {                                                // the hl-mer is in the table: the packer put it there
                    const ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(ix.lclx + 2 * slot);
                    if (x.x == code + 1) { e = x.y; break; }
                    if (x.x == 0) { e = 0xFFFFFFull << 40; break; }       // (never: defensive, takes the reference's path)
                    slot = (slot + 1) & ix.lclx_mask;
                }
                if (cnt) cnt[0] += 1;
            }
        } else {
            e = ix.lcl[at];
        }
        if (cnt) cnt[0] += 1;
        if ((e >> 40) != 0xFFFFFFull) {                               // (marker: interval too long for 24 bits)
            if (e == 0) { k = 0; l = 0; return 0; }                   // dead by its hl-th base; k, l are dead values then
            k = e & ((1ull << 40) - 1ull);
            l = k + (e >> 40) - 1;
            left = left2;
            looked_up = true;
        }
    }
    if (!looked_up) {
        if (left >= 0) {
            lc_lookup(ix, (win >> (2 * left)) & ((1ull << (2 * ix.hlen)) - 1ull), k, l);
            if (cnt) cnt[0] += 1;
        } else {
            k = 1;
            l = ix.length - 1;
        }
        if (k == 0 && l == 0) return 0;
    }
    for (int i = left - 1; i >= 0; --i) {
        uint32_t c = (uint32_t) (win >> (2 * i)) & 3u;
        uint64_t ra, rb;
        const uint32_t nreq = occ_lf2(ix, c, k - 1, l, ra, rb);
        if (cnt) cnt[1] += nreq;
        k = ra + 1;
        l = rb;
        if (k > l) break;
    }
    return k > l ? 0 : l - k + 1;
}
