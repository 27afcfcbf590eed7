// pileup_call_harness.cpp -- a stand-alone program over pileup_call_step.h (docs/GACT_SPEC.md, "Pileup calls"), built with
// -fsanitize=address,undefined by tests/test_pileup_call_cpu.py and run as a child process: the rule and the host walk on
// records, text bytes, a site table and a cons buffer that sit in heap blocks of exactly their size, so that a byte read or
// written at or behind any end is an error.
//
//   pileup_call_harness <input file> <output file>
// input file:  u64 pos0, u64 count, u64 cap, u32 min_depth, u32 min_count, u32 min_pct, then count lrm_pileup_col records,
//              then count text bytes
// output file: u64 total, then min(total, cap) lrm_pileup_site records, then count cons bytes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "pileup_call_step.h"

template <typename T>
static bool take(FILE *f, T *v) { return fread(v, sizeof(T), 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s input output\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t pos0, count, cap;
    uint32_t o[3];
    if (!take(f, &pos0) || !take(f, &count) || !take(f, &cap) || !take(f, &o[0]) || !take(f, &o[1]) || !take(f, &o[2])) { fprintf(stderr, "bad header\n"); return 2; }
    // (a block of one byte stands for an empty one: the walk touches nothing of it)
    lrm_pileup_col *cols = (lrm_pileup_col *) malloc(count ? count * sizeof(lrm_pileup_col) : 1);
    char *content = (char *) malloc(count ? count : 1);
    lrm_pileup_site *out = (lrm_pileup_site *) malloc(cap ? cap * sizeof(lrm_pileup_site) : 1);
    uint8_t *cons = (uint8_t *) malloc(count ? count : 1);
    if ((count && fread(cols, sizeof(lrm_pileup_col), count, f) != count) || (count && fread(content, 1, count, f) != count)) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    const uint64_t total = pile_host_sites(cols, content, pos0, count, pile_call_rule(o[0], o[1], o[2]), out, cap, cons);
    const uint64_t kept = total < cap ? total : cap;
    FILE *w = fopen(argv[2], "wb");
    if (!w || fwrite(&total, 8, 1, w) != 1 || (kept && fwrite(out, sizeof(lrm_pileup_site), kept, w) != kept) ||
        (count && fwrite(cons, 1, count, w) != count) || fclose(w) != 0) { perror(argv[2]); return 2; }
    printf("%llu positions, %llu sites, %llu kept\n", (unsigned long long) count, (unsigned long long) total, (unsigned long long) kept);
    free(cols); free(content); free(out); free(cons);
    return 0;
}
