// pileup_call_step.h -- the call rule of the pileup (docs/GACT_SPEC.md, "Pileup calls"): from the record of one position and
// its text byte to the kinds of site it is, its strongest non-reference base and its consensus letter.  Read by
// pileup_kernels.hip (pileup_call_kernel, pileup_sites_kernel) and, as plain C++, by lrm_pileup_sites_host (pileup.hip) and
// tests/models/pileup_call_harness.cpp: the host rule and the CPU tests run the kernels' own source.  All arithmetic is integer.
#pragma once
#include <stdint.h>
#include "pileup_step.h"                 // pile_base_class: the class of a byte, case folded

#define LRM_CALL_MIN_DEPTH_DEFAULT 8u
#define LRM_CALL_MIN_COUNT_DEFAULT 4u
#define LRM_CALL_MIN_PCT_DEFAULT 25u

// the options with every zero field replaced by its default (the refusals are the entry points': lrm_pileup_call_check)
struct PileCallRule { uint32_t min_depth, min_count, min_pct; };
LRM_OP_FN PileCallRule pile_call_rule(uint32_t min_depth, uint32_t min_count, uint32_t min_pct) {
    PileCallRule r;
    r.min_depth = min_depth ? min_depth : LRM_CALL_MIN_DEPTH_DEFAULT;
    r.min_count = min_count ? min_count : LRM_CALL_MIN_COUNT_DEFAULT;
    r.min_pct = min_pct ? min_pct : LRM_CALL_MIN_PCT_DEFAULT;
    return r;
}

// n reads of `depth` are enough to be called: the depth, the count and the percentage, the last in 64 bits
LRM_OP_FN bool pile_call_passes(const PileCallRule &r, uint32_t depth, uint32_t n) {
    return depth >= r.min_depth && n >= r.min_count && 100ull * (uint64_t) n >= (uint64_t) r.min_pct * (uint64_t) depth;
}

// what the rule says of one position; kinds == 0: no site
struct PileCall { uint32_t kinds, n_alt; uint8_t alt, cons; };

// c: the position's record, byte: its text byte as stored.  Selects only, in the fixed order A, C, G, T: a strict `>`
// keeps the earlier of two equal counts.
LRM_OP_FN PileCall pile_call(const PileCallRule &r, uint32_t depth, uint32_t n_eq, uint32_t x_a, uint32_t x_c, uint32_t x_g, uint32_t x_t,
                               uint32_t n_del, uint32_t n_ins, uint32_t byte) {
    const uint32_t rc = pile_base_class(byte);
    const uint32_t x[4] = {x_a, x_c, x_g, x_t};
    const char letter[4] = {'A', 'C', 'G', 'T'};
    PileCall out;
    out.kinds = 0;
    out.n_alt = 0;
    out.alt = (uint8_t) '.';
    // the consensus starts at the reference class (nothing for a text byte of class `other`): it wins every tie
    uint32_t best = 0;
    uint8_t cons = (uint8_t) 'N';
    for (uint32_t k = 0; k < 4u; ++k) {
        best = k == rc ? x[k] + n_eq : best;
        cons = k == rc ? (uint8_t) letter[k] : cons;
    }
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t allele = x[k] + (k == rc ? n_eq : 0u);
        if (k != rc) {
            if (pile_call_passes(r, depth, allele)) out.kinds |= LRM_CALL_SNV;
            if (allele > out.n_alt) { out.n_alt = allele; out.alt = (uint8_t) letter[k]; }
            if (allele > best) { best = allele; cons = (uint8_t) letter[k]; }
        }
    }
    if (n_del > best) { best = n_del; cons = (uint8_t) '-'; }
    if (pile_call_passes(r, depth, n_del)) out.kinds |= LRM_CALL_DEL;
    if (pile_call_passes(r, depth, n_ins)) out.kinds |= LRM_CALL_INS;
    out.cons = (depth < r.min_depth || best == 0u) ? (uint8_t) 'N' : cons;
    return out;
}

// the site record of text position pos as the four words of its two halves (lrm_pileup_site: pos, depth, n_ref | n_alt,
// n_del, n_ins, the four bytes ref, alt, cons, kinds)
LRM_OP_FN void pile_call_site_words(const PileCall &c, uint64_t pos, uint32_t depth, uint32_t n_eq, uint32_t n_del, uint32_t n_ins,
                                      uint32_t byte, uint32_t (&w)[8]) {
    w[0] = (uint32_t) pos; w[1] = (uint32_t) (pos >> 32); w[2] = depth; w[3] = n_eq;
    w[4] = c.n_alt; w[5] = n_del; w[6] = n_ins;
    w[7] = (byte & 0xFFu) | ((uint32_t) c.alt << 8) | ((uint32_t) c.cons << 16) | (c.kinds << 24);
}

// ---- the rule on the host (lrm_pileup_sites_host) ----
// cols[k], content[k]: the record and the text byte of text position pos0 + k.  Sites into out[0 .. cap) in ascending
// position, cons (may be null) gets count letters; returns the number of sites, whether or not they fit.
static inline uint64_t pile_host_sites(const lrm_pileup_col *cols, const char *content, uint64_t pos0, uint64_t count, const PileCallRule &r,
                                       lrm_pileup_site *out, uint64_t cap, uint8_t *cons) {
    uint64_t total = 0;
    for (uint64_t k = 0; k < count; ++k) {
        const lrm_pileup_col &c = cols[k];
        const uint32_t byte = (uint8_t) content[k];
        const PileCall call = pile_call(r, c.depth, c.n_eq, c.x_a, c.x_c, c.x_g, c.x_t, c.n_del, c.n_ins, byte);
        if (cons) cons[k] = call.cons;
        if (!call.kinds) continue;
        if (total < cap) {
            uint32_t w[8];
            pile_call_site_words(call, pos0 + k, c.depth, c.n_eq, c.n_del, c.n_ins, byte, w);
            lrm_pileup_site s;
            s.pos = pos0 + k; s.depth = w[2]; s.n_ref = w[3]; s.n_alt = w[4]; s.n_del = w[5]; s.n_ins = w[6];
            s.ref = (uint8_t) w[7]; s.alt = (uint8_t) (w[7] >> 8); s.cons = (uint8_t) (w[7] >> 16); s.kinds = (uint8_t) (w[7] >> 24);
            out[total] = s;
        }
        ++total;
    }
    return total;
}
