// SPDX-License-Identifier: MIT
// C entry points over longreadmapper_amd/csrc/base_words.h for tests/test_base_words_cpu.py: the header is the source
// the byte kernels compile, evaluated here with its software byte permute.  Every entry point takes n words and writes
// the word form's result and the result put together from the per-byte definition.
#include "../../longreadmapper_amd/csrc/base_words.h"

#define BYTE(x, e) (((x) >> (8 * (e))) & 0xFFu)

void bwh_codes4(const uint32_t *x, int n, uint32_t *got, uint32_t *want) {
    for (int i = 0; i < n; ++i) {
        got[i] = codes4(x[i]);
        want[i] = 0;
        for (int e = 0; e < 4; ++e) want[i] |= bw_code1(BYTE(x[i], e)) << (8 * e);
    }
}

void bwh_letters4(const uint32_t *x, int n, uint32_t *got, uint32_t *want) {       // of the codes of x
    for (int i = 0; i < n; ++i) {
        got[i] = letters4(codes4(x[i]));
        want[i] = 0;
        for (int e = 0; e < 4; ++e) want[i] |= bw_letter1(bw_code1(BYTE(x[i], e))) << (8 * e);
    }
}

void bwh_not_acgt4(const uint32_t *x, int n, uint32_t *got, uint32_t *want) {      // as a 0 / 1 answer
    for (int i = 0; i < n; ++i) {
        got[i] = not_acgt4(x[i]) != 0;
        want[i] = 0;
        for (int e = 0; e < 4; ++e) want[i] |= bw_not_acgt1(BYTE(x[i], e));
    }
}

void bwh_pack8(const uint32_t *x, int n, uint32_t *got, uint32_t *want) {          // of the codes of x
    for (int i = 0; i < n; ++i) {
        got[i] = pack8(codes4(x[i]));
        want[i] = 0;
        for (int e = 0; e < 4; ++e) want[i] |= bw_code1(BYTE(x[i], e)) << (2 * e);
    }
}

// the kernels' use of comp4: the word form where the case-folded word holds letters only, the byte-exact path otherwise;
// took_word[i] says which one ran
void bwh_comp4(const uint32_t *x, int n, uint32_t *got, uint32_t *want, uint32_t *took_word) {
    for (int i = 0; i < n; ++i) {
        took_word[i] = not_letter4(x[i]) == 0;
        want[i] = 0;
        for (int e = 0; e < 4; ++e) want[i] |= bw_comp1(BYTE(x[i], e)) << (8 * e);
        got[i] = took_word[i] ? comp4(x[i]) : want[i];
    }
}

void bwh_revcomp4(const uint32_t *x, int n, uint32_t *got, uint32_t *want, uint32_t *took_word) {
    for (int i = 0; i < n; ++i) {
        took_word[i] = not_letter4(x[i]) == 0;
        want[i] = 0;
        for (int e = 0; e < 4; ++e) want[i] |= bw_comp1(BYTE(x[i], 3 - e)) << (8 * e);
        got[i] = took_word[i] ? revcomp4_letters(x[i]) : bw_revcomp4_exact(x[i]);
    }
}

// four columns whose first nv (0 .. 4) are coded and the rest 'I'
void bwh_ops4(const uint32_t *c8, int n, uint32_t nv, uint32_t *got, uint32_t *want) {
    for (int i = 0; i < n; ++i) {
        got[i] = nv >= 4 ? ops4(c8[i]) : ops4_tail(ops4(c8[i]), bw_keep(nv));
        want[i] = 0;
        for (uint32_t e = 0; e < 4; ++e) want[i] |= (e < nv ? bw_op1((c8[i] >> (2 * e)) & 3u) : (uint32_t) 'I') << (8 * e);
    }
}

uint32_t bwh_perm(uint32_t s0, uint32_t s1, uint32_t sel) { return BW_PERM(s0, s1, sel); }
