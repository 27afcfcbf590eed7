/* tests/test_rival_cpu.py: longreadmapper_amd/csrc/rival_rule.h -- the arithmetic rival_locus_kernel compiles -- as plain C */
#include "../../longreadmapper_amd/csrc/rival_rule.h"

uint32_t rvh_min_hits(uint32_t v) { return rv_min_hits(v); }
uint32_t rvh_ratio_pct(uint32_t v) { return rv_ratio_pct(v); }
int rvh_candidate(uint32_t n1, uint32_t n2, uint32_t flags, uint32_t H, uint32_t pct) { return rv_candidate(n1, n2, flags, H, pct); }
uint32_t rvh_sub_shift(uint32_t r) { return rv_sub_shift(r); }
uint32_t rvh_off(uint64_t key, uint32_t r, uint32_t h) { return rv_off(key, r, h); }
uint64_t rvh_key_of(uint32_t tag, uint32_t r, uint32_t off) { return rv_key_of(tag, r, off); }
uint32_t rvh_tag(uint64_t key, uint32_t r, uint32_t h) { return mq_tag(key, r, h); }
uint32_t rvh_sub_buckets(void) { return RV_SUB_BUCKETS; }
