// SPDX-License-Identifier: MIT
// C entry points over longreadmapper_amd/csrc/anchor_clip.h for tests/test_clip_cpu.py: the header is the source
// anchor_clip_kernel compiles.  A row is cut the way the kernel cuts it -- lane pieces of 16 columns, 64 of them to a
// wavefront step of 1024 -- except that the FIRST piece may be shorter (first = 1 .. 16), so that the seams between
// pieces fall on every position of the row.
#include <string.h>
#include "../../longreadmapper_amd/csrc/anchor_clip.h"

static struct AcSeg fold_piece(const uint8_t *ops, uint32_t cols, uint32_t P) {
    uint8_t buf[16];
    uint32_t w[4];
    memset(buf, '=', sizeof(buf));                 // what lies beyond the row must not matter: the worst byte there
    memcpy(buf, ops, cols);
    memcpy(w, buf, sizeof(w));
    return ac_fold16(w, cols, P);
}

// -> keep; out[0 .. 3) = columns of the kept prefix other than '=', 'I', 'D'; out[3] = best score + 2^31, out[4] = sum + 2^31
uint32_t acl_clip_row(const uint8_t *ops, uint32_t m, uint32_t P, uint32_t B, uint32_t first, uint32_t *out) {
    struct AcSeg row = ac_empty();
    uint32_t at = 0, piece = first < 1 || first > 16 ? 16 : first;
    while (at < m) {                               // one wavefront step: 64 lane pieces, merged at their place in the step
        struct AcSeg step = ac_empty();
        const uint32_t step_at = at;
        for (int lane = 0; lane < 64; ++lane) {    // (a lane past the end of the row takes part as in the kernel: no columns)
            const uint32_t cols = m - at < piece ? m - at : piece;
            step = ac_merge(step, at - step_at, fold_piece(ops + at, cols, P));
            at += cols;
            piece = 16;
        }
        row = ac_merge(row, step_at, step);
    }
    const uint32_t keep = ac_keep(row, m, B);
    out[0] = out[1] = out[2] = 0;
    for (uint32_t o = 0; o < keep; o += 16) {
        const uint32_t cols = keep - o < 16 ? keep - o : 16;
        uint8_t buf[16];
        uint32_t w[4];
        memset(buf, 0, sizeof(buf));
        memcpy(buf, ops + o, cols);
        memcpy(w, buf, sizeof(w));
        out[0] += ac_count_not(w, cols, '=');
        out[1] += ac_count_not(w, cols, 'I');
        out[2] += ac_count_not(w, cols, 'D');
    }
    out[3] = (uint32_t) ac_key_score(row.key) + AC_BIAS;
    out[4] = (uint32_t) row.sum + AC_BIAS;
    return keep;
}
