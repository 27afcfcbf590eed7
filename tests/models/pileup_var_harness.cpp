// pileup_var_harness.cpp -- a stand-alone program over pileup_var_step.h (docs/GACT_SPEC.md, "Pileup variants and VCF"),
// built with -fsanitize=address,undefined by tests/test_pileup_var_cpu.py and run as a child process: the host rule on
// records, words, text bytes and an output table that sit in heap blocks of exactly their size, so that a byte read or
// written at or behind any end is an error.
//
//   pileup_var_harness <input file> <output file>
// input file:  u32 K, u64 count, u64 cap, u64 pos0, u32 min_depth, u32 min_count, u32 min_pct, u32 hom_pct, then count
//              lrm_pileup_col records, count * 4 * K words (position-major), count text bytes
// output file: u64 total, then min(total, cap) 48-byte records
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "pileup_var_step.h"

template <typename T>
static bool take(FILE *f, T *v) { return fread(v, sizeof(T), 1, f) == 1; }
// a heap block of exactly n bytes read from the file (a block of one byte stands for an empty one: nothing of it is touched)
static uint8_t *block(FILE *f, uint64_t n) {
    uint8_t *p = (uint8_t *) malloc(n ? n : 1);
    if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short file\n"); exit(2); }
    return p;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s input output\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *w = fopen(argv[2], "wb");
    if (!w) { perror(argv[2]); return 2; }
    uint32_t K, o[4];
    uint64_t count, cap, pos0;
    if (!take(f, &K) || K > LRM_PILEUP_INS_COLS_LIMIT || !take(f, &count) || !take(f, &cap) || !take(f, &pos0) || !take(f, &o[0]) || !take(f, &o[1]) ||
        !take(f, &o[2]) || !take(f, &o[3])) { fprintf(stderr, "bad header\n"); return 2; }
    lrm_pileup_col *cols = (lrm_pileup_col *) block(f, count * sizeof(lrm_pileup_col));
    uint32_t *words = (uint32_t *) block(f, count * 16ull * K);
    char *content = (char *) block(f, count);
    uint32_t *out = (uint32_t *) malloc(cap ? cap * 48u : 1);
    const PileVarRule rule = pile_var_rule(pile_call_rule(o[0], o[1], o[2]), o[3]);
    const uint64_t total = pile_host_variants(cols, words, K, content, pos0, count, rule, out, cap);
    const uint64_t kept = total < cap ? total : cap;
    if (fwrite(&total, 8, 1, w) != 1 || (kept && fwrite(out, 48, kept, w) != kept)) { perror(argv[2]); return 2; }
    free(cols); free(words); free(content); free(out);
    fclose(f);
    if (fclose(w) != 0) { perror(argv[2]); return 2; }
    return 0;
}
