// pileup_host_harness.cpp -- a stand-alone program over pileup_step.h (docs/GACT_SPEC.md, "Pileup"), built with
// -fsanitize=address,undefined by tests/test_pileup_cpu.py and run as a child process: the word step and the host walk on rows
// whose op bytes and read bytes sit in heap blocks of exactly their size, so that a byte read at or behind either end is an error.
//
//   pileup_host_harness <rows file> <records file>
// rows file:    u64 lo, u64 hi, u32 n, then per row: u64 loc, u32 n_ops, u32 read_len, n_ops op bytes, read_len read bytes
// records file: the hi - lo lrm_pileup_col records of the window after every row was added
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pileup_step.h"

template <typename T>
static bool take(FILE *f, T *v) { return fread(v, sizeof(T), 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s rows records\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t lo, hi;
    uint32_t n;
    if (!take(f, &lo) || !take(f, &hi) || !take(f, &n) || lo >= hi) { fprintf(stderr, "bad header\n"); return 2; }
    const uint64_t W = hi - lo;
    std::vector<uint32_t> planes(LRM_PILEUP_WORDS(W), 0u);
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t loc;
        uint32_t n_ops, read_len;
        if (!take(f, &loc) || !take(f, &n_ops) || !take(f, &read_len)) { fprintf(stderr, "row %u: short file\n", i); return 2; }
        uint8_t *ops = (uint8_t *) malloc(n_ops ? n_ops : 1), *read = (uint8_t *) malloc(read_len ? read_len : 1);
        if ((n_ops && fread(ops, 1, n_ops, f) != n_ops) || (read_len && fread(read, 1, read_len, f) != read_len)) { fprintf(stderr, "row %u: short file\n", i); return 2; }
        // (a block of one byte stands for an empty one: the walk reads nothing of it)
        uint8_t *ops_exact = n_ops ? ops : nullptr, *read_exact = read_len ? read : nullptr;
        if (n_ops) pile_host_add(ops_exact, n_ops, read_exact, read_len, loc, lo, hi, planes.data());
        free(ops);
        free(read);
    }
    fclose(f);
    std::vector<lrm_pileup_col> cols(W);
    pile_host_cols(planes.data(), W, 0, W, cols.data());
    FILE *o = fopen(argv[2], "wb");
    if (!o || fwrite(cols.data(), sizeof(lrm_pileup_col), W, o) != W || fclose(o) != 0) { perror(argv[2]); return 2; }
    printf("%u rows, %llu positions\n", n, (unsigned long long) W);
    return 0;
}
