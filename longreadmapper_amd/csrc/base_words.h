// SPDX-License-Identifier: MIT
// base_words.h -- four bases, or four CIGAR columns, per instruction: the word forms of the per-byte helpers that the
// byte kernels around the extension stage run (bs_pack_reads, revcomp, the row gathers and the anchored job rows through seq_bytes.h, bs_expand).
// A table of four bytes is looked up for four bytes at once by v_perm_b32.  The file compiles for the device (hipcc)
// and as plain C for the host (the permute in software), so tests/test_base_words_cpu.py checks on the CPU the very
// source the kernels run, against the per-byte definitions that stand next to each word form.
#ifndef LRM_BASE_WORDS_H
#define LRM_BASE_WORDS_H
#include <stdint.h>

#if defined(__HIPCC__)
#define BW_FN __device__ __forceinline__
// v_perm_b32: byte e of the result is byte sel[e] of the eight bytes {s0, s1} (0 .. 3: s1, 4 .. 7: s0)
#define BW_PERM(s0, s1, sel) __builtin_amdgcn_perm((s0), (s1), (sel))
// a table or a fixed selector: kept in a scalar register (v_perm_b32 takes no literal; the compiler would spend a
// vector register on each)
static __device__ __forceinline__ uint32_t bw_const(uint32_t t) { asm("" : "+s"(t)); return t; }
#else
#define BW_FN static inline
// v_perm_b32 by the ISA's description: selector 0 .. 7 a byte of {s0, s1}; 8 .. 11 the sign of its byte 1, 3, 5, 7
// spread over the byte; 12 the byte 0x00; 13 and above the byte 0xFF
static inline uint32_t bw_perm_eval(uint32_t s0, uint32_t s1, uint32_t sel) {
    const uint64_t data = ((uint64_t) s0 << 32) | (uint64_t) s1;
    uint32_t r = 0;
    for (int e = 0; e < 4; ++e) {
        const uint32_t s = (sel >> (8 * e)) & 0xFFu;
        uint32_t b;
        if (s >= 13u) b = 0xFFu;
        else if (s == 12u) b = 0x00u;
        else if (s >= 8u) b = ((data >> (16 * (s - 8u) + 15)) & 1u) ? 0xFFu : 0x00u;
        else b = (uint32_t) (data >> (8 * s)) & 0xFFu;
        r |= b << (8 * e);
    }
    return r;
}
#define BW_PERM(s0, s1, sel) bw_perm_eval((s0), (s1), (sel))
static inline uint32_t bw_const(uint32_t t) { return t; }
#endif

#define BW_LETTERS 0x54474341u        // byte c: the letter with code c (A, C, G, T)
#define BW_COMPS 0x41434754u          // byte c: the complement of the letter with code c (T, G, C, A)
#define BW_OPS 0x44493d58u            // byte c: the CIGAR byte of column code c ('X', '=', 'I', 'D')
#define BW_ALL_I 0x49494949u

// ---- the per-byte definitions ----------------------------------------------------------
BW_FN uint32_t bw_code1(uint32_t c) { return ((c >> 1) ^ (c >> 2)) & 3u; }          // base_code: A 0, C 1, G 2, T 3
BW_FN uint32_t bw_letter1(uint32_t code) { return (BW_LETTERS >> (8 * (code & 3u))) & 0xFFu; }
BW_FN uint32_t bw_not_acgt1(uint32_t c) { return !(c == 'A' || c == 'C' || c == 'G' || c == 'T'); }
BW_FN uint32_t bw_comp1(uint32_t c) {                                               // comp_base (seq_bytes.h)
    const uint32_t u = c & 0xDFu;
    return u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N';
}
BW_FN uint32_t bw_op1(uint32_t code) { return (BW_OPS >> (8 * (code & 3u))) & 0xFFu; }

// ---- the word forms --------------------------------------------------------------------
// byte e: bw_code1 of byte e of x.  (The shifts bring bits of the next byte in above bit 5 only.)
BW_FN uint32_t codes4(uint32_t x) { return ((x >> 1) ^ (x >> 2)) & 0x03030303u; }

// byte e: bw_letter1 of byte e of code4 (codes 0 .. 3)
BW_FN uint32_t letters4(uint32_t code4) { return BW_PERM(0u, bw_const(BW_LETTERS), code4); }

// non-zero exactly when some byte has bw_not_acgt1: a byte outside ACGT never equals the letter of its own code, a
// byte inside always does
BW_FN uint32_t not_acgt4(uint32_t x) { return letters4(codes4(x)) ^ x; }

// not_acgt4 of the case-folded word: non-zero exactly when some byte is none of ACGTacgt (bit 5, the case, is not
// among the bits that make the code, so the codes of x and of the folded x are the same)
BW_FN uint32_t not_letter4(uint32_t x) { return letters4(codes4(x)) ^ (x & 0xDFDFDFDFu); }

// bits 2e, 2e + 1: byte e of code4 (codes 0 .. 3).  (pack2bit_kernel does not use it: with pack8(codes4()) it issued
// 40 % fewer vector instructions and ran 2.5 % SLOWER, profiles/r10 -- the kernel waits for memory either way.)
BW_FN uint32_t pack8(uint32_t code4) {
    const uint32_t u = code4 | (code4 >> 6);                  // bits 0 .. 3: codes 0, 1; bits 16 .. 19: codes 2, 3
    return (u | (u >> 12)) & 0xFFu;
}

// byte e: bw_comp1 of byte e of x, where x holds letters of ACGTacgt only (the caller asks not_acgt4 of the
// case-folded word and takes the byte-exact path otherwise)
BW_FN uint32_t comp4(uint32_t x) { return BW_PERM(0u, bw_const(BW_COMPS), codes4(x)); }

// byte e: bw_comp1 of byte 3 - e of x: reversed and complemented, by the byte-exact path where a byte is no letter
BW_FN uint32_t bw_revcomp4_exact(uint32_t x) {
    uint32_t o = 0;
    for (int e = 0; e < 4; ++e) o |= bw_comp1((x >> (8 * (3 - e))) & 0xFFu) << (8 * e);
    return o;
}
BW_FN uint32_t revcomp4_letters(uint32_t x) {                // x: letters of ACGTacgt only
    return BW_PERM(0u, bw_const(BW_COMPS), BW_PERM(0u, codes4(x), bw_const(0x00010203u)));
}

// byte e: bw_op1 of bits 2e, 2e + 1 of c8 (four column codes)
BW_FN uint32_t ops4(uint32_t c8) {
    const uint32_t u = c8 | (c8 << 6);                         // bits 0, 1: code 0; bits 8, 9: code 1
    const uint32_t sel = (u | (u << 12)) & 0x03030303u;        // c8 | c8 << 6 | c8 << 12 | c8 << 18: a code per byte
    return BW_PERM(0u, bw_const(BW_OPS), sel);
}

// the first nv bytes (0 .. 4 and above) of a dword
BW_FN uint32_t bw_keep(uint32_t nv) { return nv >= 4u ? 0xFFFFFFFFu : ((1u << (8u * nv)) - 1u); }

// four CIGAR bytes of a row whose columns under keep are coded (op4 = ops4 of their codes) and the rest are 'I'
BW_FN uint32_t ops4_tail(uint32_t op4, uint32_t keep) { return (op4 & keep) | (BW_ALL_I & ~keep); }

#endif
