/* tests/test_mapq_cpu.py: longreadmapper_amd/csrc/mapq_rule.h -- the arithmetic mapq_vote_kernel compiles -- as plain C */
#include "../../longreadmapper_amd/csrc/mapq_rule.h"

uint32_t mqh_radius_log2(uint32_t len) { return mq_radius_log2(len); }
uint32_t mqh_radius(uint32_t len) { return mq_radius(len); }
int mqh_inside(uint64_t key, uint64_t best, uint32_t r) { return mq_inside(key, best, r); }
uint64_t mqh_bucket(uint64_t key, uint32_t r, uint32_t h) { return mq_bucket(key, r, h); }
uint32_t mqh_tag(uint64_t key, uint32_t r, uint32_t h) { return mq_tag(key, r, h); }
uint32_t mqh_tag_empty(void) { return MQ_TAG_EMPTY; }
uint32_t mqh_value(uint32_t n1, uint32_t n2) { return mq_value(n1, n2); }
