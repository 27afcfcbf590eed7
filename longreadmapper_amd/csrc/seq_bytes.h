// seq_bytes.h -- byte-level base helpers shared by the extension-stage kernels (device code only)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "base_words.h"

// alnmain.c:31-52: A/a -> T, C/c -> G, G/g -> C, T/t -> A, anything else -> N.  Branch-free on purpose: a `switch`
// compiles to a cascade of divergent branches per byte (the first revcomp kernel spent 1.5 ms per Gbp in them).
__device__ __forceinline__ char comp_base(char c) {
    const uint32_t u = (uint32_t) (uint8_t) c & 0xDFu;            // fold case
    uint32_t r = 'N';
    r = u == 'A' ? 'T' : r;
    r = u == 'C' ? 'G' : r;
    r = u == 'G' ? 'C' : r;
    r = u == 'T' ? 'A' : r;
    return (char) r;
}

__device__ __forceinline__ uint32_t bytes_equal(uint32_t x, uint32_t c4) {     // 0xFF in every byte of x equal to c4's
    const uint32_t z = x ^ c4;
    const uint32_t t = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu);  // 0x80 where the byte of z is zero
    return (t >> 7) * 0xFFu;
}

__device__ __forceinline__ uint32_t revcomp4_exact(uint32_t w) {       // 4 bytes: reversed, comp_base of each
    const uint32_t x = w & 0xDFDFDFDFu;
    const uint32_t a = bytes_equal(x, 0x41414141u), c = bytes_equal(x, 0x43434343u);
    const uint32_t g = bytes_equal(x, 0x47474747u), t = bytes_equal(x, 0x54545454u);
    const uint32_t o = (a & 0x54545454u) | (c & 0x47474747u) | (g & 0x43434343u) | (t & 0x41414141u) |
                       (~(a | c | g | t) & 0x4E4E4E4Eu);
    return __builtin_bswap32(o);
}

// 4 bases: reversed and complemented.  Four letters of ACGTacgt take the word form (base_words.h: a code per byte, then
// two byte permutes -- the reversal and the table T, G, C, A); a word with any other byte takes revcomp4_exact.
__device__ __forceinline__ uint32_t revcomp4(uint32_t w) {
    return not_letter4(w) == 0 ? revcomp4_letters(w) : revcomp4_exact(w);
}

// 16 bases reversed and complemented; word(e), e = 0 .. 3: the four dwords in memory order (a callable, so that each
// dword is formed right before its use, as the reverse-complement kernel's schedule wants it)
template <typename F>
__device__ __forceinline__ uint4 revcomp16(F word) {
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[3 - e] = revcomp4(word(e));
    return make_uint4(o[0], o[1], o[2], o[3]);
}
