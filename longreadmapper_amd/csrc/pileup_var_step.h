// pileup_var_step.h -- the variant rule of the pileup (docs/GACT_SPEC.md, "Pileup variants and VCF"): from the kinds of the
// call rule, position by position, to variant records -- adjacent deleted positions merged into one run, the inserted
// allele inside the record, a genotype on every record.  Read by pileup_kernels.hip (pileup_var_count_kernel,
// pileup_var_ext_kernel, pileup_var_write_kernel) and, as plain C++, by lrm_pileup_variants_host (pileup.hip) and
// tests/models/pileup_var_harness.cpp: the host rule and the CPU tests run the kernels' own source.  All arithmetic is integer.
#pragma once
#include <stdint.h>
#include <initializer_list>
#include "pileup_ins_step.h"             // PileInsAllele, pile_ins_allele; pileup_call_step.h: the kinds, PileCallRule

#define LRM_VAR_HOM_PCT_DEFAULT 70u

// the call rule plus the genotype threshold, every zero field replaced by its default (the refusals are the entry points')
struct PileVarRule { PileCallRule call; uint32_t hom_pct; };
LRM_OP_FN PileVarRule pile_var_rule(const PileCallRule &call, uint32_t hom_pct) {
    PileVarRule r;
    r.call = call;
    r.hom_pct = hom_pct ? hom_pct : LRM_VAR_HOM_PCT_DEFAULT;
    return r;
}

// 2: the alternative is hom_pct percent of the depth or more (64-bit products), 1: it is less
LRM_OP_FN uint32_t pile_var_gt(uint32_t hom_pct, uint32_t n_alt, uint32_t depth) {
    return 100ull * (uint64_t) n_alt >= (uint64_t) hom_pct * (uint64_t) depth ? 2u : 1u;
}

// The records of one position, in their order DEL, SNV, INS, as a mask of LRM_CALL_*: a deleted position gives a record only
// where a run starts -- at the range's first position, or behind a position that is not deleted.  prev_del: position g - 1
// lies inside the range and has LRM_CALL_DEL.
LRM_OP_FN uint32_t pile_var_emits(uint32_t kinds, bool prev_del) {
    return (kinds & (LRM_CALL_SNV | LRM_CALL_INS)) | ((kinds & LRM_CALL_DEL) && !prev_del ? LRM_CALL_DEL : 0u);
}
LRM_OP_FN uint32_t pile_var_count(uint32_t emits) {
    return ((emits >> 1) & 1u) + (emits & 1u) + ((emits >> 2) & 1u);
}

// The 48-byte record (lrm_pileup_variant) as the twelve words of its three 16-byte parts: pos, len, depth | n_ref, n_alt,
// n_col0, the four bytes kind, ref, alt, gt | bases[8], ins_flags and seven bytes of zero padding.
LRM_OP_FN void pile_var_words(uint64_t pos, uint32_t len, uint32_t depth, uint32_t n_ref, uint32_t n_alt, uint32_t n_col0, uint32_t kind,
                                uint32_t ref, uint32_t alt, uint32_t gt, uint64_t bases, uint32_t ins_flags, uint32_t (&w)[12]) {
    w[0] = (uint32_t) pos; w[1] = (uint32_t) (pos >> 32); w[2] = len; w[3] = depth;
    w[4] = n_ref; w[5] = n_alt; w[6] = n_col0;
    w[7] = (kind & 0xFFu) | ((ref & 0xFFu) << 8) | ((alt & 0xFFu) << 16) | (gt << 24);
    w[8] = (uint32_t) bases; w[9] = (uint32_t) (bases >> 32); w[10] = ins_flags & 0xFFu; w[11] = 0u;
}
// the three records of a position, one at a time: `kind` is exactly one of LRM_CALL_DEL / _SNV / _INS.  run: the length of
// the deleted run that starts here (DEL only); a: the inserted allele of the position, all zero on a plain accumulator (INS only)
LRM_OP_FN void pile_var_record(const PileVarRule &r, uint32_t kind, uint64_t pos, uint32_t depth, uint32_t n_eq, uint32_t n_del, uint32_t n_ins,
                                 uint32_t byte, const PileCall &call, uint32_t run, const PileInsAllele &a, uint32_t (&w)[12]) {
    if (kind == LRM_CALL_DEL)
        pile_var_words(pos, run, depth, n_eq, n_del, 0u, kind, byte, 0u, pile_var_gt(r.hom_pct, n_del, depth), 0ull, 0u, w);
    else if (kind == LRM_CALL_SNV)
        pile_var_words(pos, 1u, depth, n_eq, call.n_alt, 0u, kind, byte, call.alt, pile_var_gt(r.hom_pct, call.n_alt, depth), 0ull, 0u, w);
    else
        pile_var_words(pos, a.len, depth, n_eq, n_ins, a.n_col0, kind, byte, 0u, pile_var_gt(r.hom_pct, n_ins, depth), a.bases, a.flags, w);
}

// ---- the deleted runs across tiles (pileup_var_ext_kernel) ----
// The summary of a stretch of positions: `len` leading positions are deleted, `full` says that these are all of them.  Two
// adjacent stretches combine into the summary of both: associative, identity {0, true}.
struct PileVarLead { uint32_t len; bool full; };
LRM_OP_FN PileVarLead pile_var_lead_join(const PileVarLead &near, const PileVarLead &far) {
    PileVarLead o;
    o.len = near.len + (near.full ? far.len : 0u);
    o.full = near.full && far.full;
    return o;
}
// a tile's summary in one word: bit 31 is `full`, the length is below 2^31 (3 * count < 2^32)
#define LRM_VAR_LEAD_FULL 0x80000000u
LRM_OP_FN uint32_t pile_var_lead_word(const PileVarLead &l) { return l.len | (l.full ? LRM_VAR_LEAD_FULL : 0u); }
LRM_OP_FN PileVarLead pile_var_lead_of(uint32_t word) {
    PileVarLead l;
    l.len = word & ~LRM_VAR_LEAD_FULL;
    l.full = (word & LRM_VAR_LEAD_FULL) != 0u;
    return l;
}

// ---- the rule on the host (lrm_pileup_variants_host; tests/models/pileup_var_harness.cpp) ----
// cols[k], content[k] and ins_words + 4 * K * k: the record, the text byte and the position-major insertion words of text
// position pos0 + k (K == 0: a plain accumulator, ins_words is not read).  The range is [0, count): runs are cut at its
// ends.  Records into out[0 .. cap) as 48-byte groups of twelve words; returns their number whether or not they fit.
static inline uint64_t pile_host_variants(const lrm_pileup_col *cols, const uint32_t *ins_words, uint32_t K, const char *content, uint64_t pos0,
                                          uint64_t count, const PileVarRule &r, uint32_t *out, uint64_t cap) {
    uint64_t total = 0, run_end = 0;                                   // run_end: the end of the last run found
    bool prev_del = false;
    for (uint64_t g = 0; g < count; ++g) {
        const lrm_pileup_col &c = cols[g];
        const uint32_t byte = (uint8_t) content[g];
        const PileCall call = pile_call(r.call, c.depth, c.n_eq, c.x_a, c.x_c, c.x_g, c.x_t, c.n_del, c.n_ins, byte);
        const uint32_t emits = pile_var_emits(call.kinds, prev_del);
        prev_del = (call.kinds & LRM_CALL_DEL) != 0u;
        if (emits & LRM_CALL_DEL) {                                    // every position is looked at once more, as part of one run
            for (run_end = g + 1; run_end < count; ++run_end) {
                const lrm_pileup_col &n = cols[run_end];
                if (!(pile_call(r.call, n.depth, n.n_eq, n.x_a, n.x_c, n.x_g, n.x_t, n.n_del, n.n_ins, (uint8_t) content[run_end]).kinds & LRM_CALL_DEL)) break;
            }
        }
        for (const uint32_t kind : {LRM_CALL_DEL, LRM_CALL_SNV, LRM_CALL_INS}) {
            if (!(emits & kind)) continue;
            if (total < cap) {
                PileInsAllele a = {0u, 0u, 0u, 0ull};
                if (kind == LRM_CALL_INS && K != 0u) a = pile_ins_allele(r.call, c.depth, c.n_ins, ins_words + 4ull * K * g, 1u, K);
                uint32_t w[12];
                pile_var_record(r, kind, pos0 + g, c.depth, c.n_eq, c.n_del, c.n_ins, byte, call, (uint32_t) (run_end - g), a, w);
                for (int k = 0; k < 12; ++k) out[12u * total + (uint64_t) k] = w[k];
            }
            ++total;
        }
    }
    return total;
}
