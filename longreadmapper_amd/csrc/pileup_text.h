// pileup_text.h -- the text form of pileup records (pileup_text.cpp; docs/GACT_SPEC.md, "Pileup"): one tab-separated line
// per position, straight into the caller's buffer
#pragma once
#include <cstdint>
#include "../../include/lrm_accel.h"

// the most bytes one line can take: the name, twelve tabs and the newline, a 20-digit position, the base, nine 10-digit counts
static inline uint64_t pileup_line_room(uint64_t name_len) { return name_len + 13u + 20u + 1u + 9u * 10u; }
// one line at dst (room for pileup_line_room bytes); returns its length
int pileup_put_line(char *dst, const char *name, uint64_t name_len, uint64_t pos1, char base, const lrm_pileup_col &c);

// ... and of site records (docs/GACT_SPEC.md, "Pileup calls"): the name, ten tabs and the newline, a 20-digit position, ref,
// alt, three kind letters, five 10-digit counts, cons
static inline uint64_t pileup_site_line_room(uint64_t name_len) { return name_len + 11u + 20u + 2u + 3u + 5u * 10u + 1u; }
int pileup_put_site_line(char *dst, const char *name, uint64_t name_len, uint64_t pos1, const lrm_pileup_site &s);
