// pileup_ins_harness.cpp -- a stand-alone program over pileup_ins_step.h (docs/GACT_SPEC.md, "Pileup insertions and the
// polished consensus"), built with -fsanitize=address,undefined by tests/test_pileup_ins_cpu.py and run as a child process:
// the host walk, the allele rule and the polish on op bytes, read bytes, planes, records, words and an output buffer that
// sit in heap blocks of exactly their size, so that a byte read or written at or behind any end is an error.
//
//   pileup_ins_harness <input file> <output file>
// input file:  u32 mode.
//   mode 0 (add):    u32 K, u64 lo, u64 hi, u64 rows, then per row u64 loc, u32 n_ops, u32 read_len, the op bytes, the read bytes
//                    output: the 4 * K * (hi - lo) words of the insertion planes
//   mode 1 (polish): u32 K, u64 count, u64 cap, u32 min_depth, u32 min_count, u32 min_pct, then count lrm_pileup_col records,
//                    count * 4 * K words (position-major), count text bytes
//                    output: u64 total, min(total, cap) bytes, then count 16-byte allele records
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "pileup_ins_step.h"

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
    uint32_t mode, K;
    if (!take(f, &mode) || !take(f, &K) || K > LRM_PILEUP_INS_COLS_LIMIT) { fprintf(stderr, "bad header\n"); return 2; }
    if (mode == 0) {
        uint64_t lo, hi, rows;
        if (!take(f, &lo) || !take(f, &hi) || !take(f, &rows) || lo >= hi || K == 0) { fprintf(stderr, "bad header\n"); return 2; }
        const uint64_t words = LRM_PILEUP_INS_WORDS(hi - lo, K);
        uint32_t *planes = (uint32_t *) calloc(words, 4);
        for (uint64_t r = 0; r < rows; ++r) {
            uint64_t loc;
            uint32_t n_ops, read_len;
            if (!take(f, &loc) || !take(f, &n_ops) || !take(f, &read_len)) { fprintf(stderr, "bad row\n"); return 2; }
            uint8_t *ops = block(f, n_ops), *read = block(f, read_len);
            if (n_ops) pile_ins_host_add(ops, n_ops, read, read_len, loc, lo, hi, K, planes);
            free(ops); free(read);
        }
        if (fwrite(planes, 4, words, w) != words) { perror(argv[2]); return 2; }
        free(planes);
    } else {
        uint64_t count, cap;
        uint32_t o[3];
        if (!take(f, &count) || !take(f, &cap) || !take(f, &o[0]) || !take(f, &o[1]) || !take(f, &o[2])) { fprintf(stderr, "bad header\n"); return 2; }
        lrm_pileup_col *cols = (lrm_pileup_col *) block(f, count * sizeof(lrm_pileup_col));
        uint32_t *words = (uint32_t *) block(f, count * 16ull * K);
        char *content = (char *) block(f, count);
        uint8_t *out = (uint8_t *) malloc(cap ? cap : 1);
        const PileCallRule rule = pile_call_rule(o[0], o[1], o[2]);
        const uint64_t total = pile_host_polish(cols, words, K, content, count, rule, out, cap);
        const uint64_t kept = total < cap ? total : cap;
        if (fwrite(&total, 8, 1, w) != 1 || (kept && fwrite(out, 1, kept, w) != kept)) { perror(argv[2]); return 2; }
        for (uint64_t g = 0; g < count && K; ++g) {
            uint32_t rec[4];
            pile_ins_allele_words(pile_ins_allele(rule, cols[g].depth, cols[g].n_ins, words + 4ull * K * g, 1u, K), rec);
            if (fwrite(rec, 4, 4, w) != 4) { perror(argv[2]); return 2; }
        }
        free(cols); free(words); free(content); free(out);
    }
    fclose(f);
    if (fclose(w) != 0) { perror(argv[2]); return 2; }
    return 0;
}
