// SPDX-License-Identifier: MIT
// Secondary alignments (docs/GACT_SPEC.md, "Secondary alignments"): the arithmetic that turns the fullest rival pair of the
// mapping-quality vote into a locus -- the candidate test on a read's lrm_mapq record, the offset of a hit inside its pair,
// the sub-bucket, the key of an offset.  Like mapq_rule.h the file compiles for the device (secondary_kernels.hip), for the
// host (lrm_api.hip) and as plain C, so tests/test_rival_cpu.py checks on the CPU the very source the kernel runs.
#ifndef LRM_RIVAL_RULE_H
#define LRM_RIVAL_RULE_H
#include "mapq_rule.h"

#define RV_MIN_HITS_DEFAULT 8        // H: min_hits == 0
#define RV_RATIO_PCT_DEFAULT 50      // pct: ratio_pct == 0
#define RV_SUB_BUCKETS 2048          // the most sub-buckets a pair has: 2 R >> s

// H and pct from the caller's words; 0: outside 1 .. 65535 / 1 .. 100
MQ_FN uint32_t rv_min_hits(uint32_t min_hits) { return min_hits == 0 ? RV_MIN_HITS_DEFAULT : min_hits <= 65535u ? min_hits : 0u; }
MQ_FN uint32_t rv_ratio_pct(uint32_t ratio_pct) { return ratio_pct == 0 ? RV_RATIO_PCT_DEFAULT : ratio_pct <= 100u ? ratio_pct : 0u; }

// a read is a candidate: it has a locus, its record did not overflow, the fullest rival pair holds at least H hits and at
// least pct per cent of the winner's.  flags: lrm_mapq.flags; bit 0 is LRM_MAPQ_OVERFLOW.  "It has a locus" is best.val > 0 in
// the spec and n1 > 0 here, on the record alone: best.key is a hit inside its own window, so best.val > 0 gives n1 >= 1, and
// a read without a locus has an all-zero record.
MQ_FN int rv_candidate(uint32_t n1, uint32_t n2, uint32_t flags, uint32_t H, uint32_t pct) {
    return n1 > 0 && !(flags & 1u) && n2 >= H && 100ull * n2 >= (uint64_t) pct * n1;
}

// s: sub-buckets are 2^s diagonals wide -- 16 up to r = 14 (reads of up to 131072 bases), then 2 R / 2048
MQ_FN uint32_t rv_sub_shift(uint32_t r) { return r > 14 ? r - 10 : 4; }

// off of a hit inside ITS pair of histogram h: (key + h R) - (bucket << (r + 1)) mod 2^64, which lies in [0, 2 R) -- the low
// r + 1 bits of key + h R
MQ_FN uint32_t rv_off(uint64_t key, uint32_t r, uint32_t h) {
    return (uint32_t) ((key + (h ? 1ull << r : 0ull)) & ((2ull << r) - 1ull));
}

// the key at offset off of the pair whose table word is tag (mq_tag).  tag >> 1 is the low 31 bits of the bucket; the word
// of a wrapped bucket has bit 30 of them set (mapq_rule.h) and that bucket's bits from 31 on are all ones, as are the bits
// 32 .. 63 of key + h R.
MQ_FN uint64_t rv_key_of(uint32_t tag, uint32_t r, uint32_t off) {
    const uint32_t low = tag >> 1;
    uint64_t v = ((uint64_t) low << (r + 1)) | off;
    if (low & 0x40000000u) v |= ~0ull << (r + 32);
    return v - ((tag & 1u) ? 1ull << r : 0ull);
}

#endif
