// seq_bytes.h -- byte-level base helpers shared by the extension-stage kernels (device code only): the base map, four and
// sixteen bases reversed and complemented, and the 16-byte step of a row move, straight and mirrored
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

// ---- the 16-byte step of a row move: the destination is 16-byte aligned, the source is not (the row gathers of
// compact_rows.h, the job rows of anchor_kernels.hip) ----
// the bytes src[0 .. cnt), cnt in 1 .. 16, as two 64-bit words (o0: bytes 0 .. 7); src at any byte: the lane loads the two
// aligned 16-byte words that hold its bytes -- the second only when its bytes reach into it -- and realigns them in registers
// (one 64-bit select for the word offset, one funnel shift for the byte offset).  Bytes from cnt on are whatever follows.
__device__ __forceinline__ void sp_load16(const char *src, uint32_t cnt, uint64_t &o0, uint64_t &o1) {
    const uint32_t off = (uint32_t) ((uintptr_t) src & 15u);
    const uint4 *a = reinterpret_cast<const uint4 *>(src - off);
    const uint4 lo = a[0];
    const uint4 hi = off + cnt > 16 ? a[1] : make_uint4(0, 0, 0, 0);       // only when the lane's bytes reach into it
    uint64_t w0 = lo.x | ((uint64_t) lo.y << 32), w1 = lo.z | ((uint64_t) lo.w << 32);
    uint64_t w2 = hi.x | ((uint64_t) hi.y << 32);
    const uint64_t w3 = hi.z | ((uint64_t) hi.w << 32);
    if (off & 8u) { w0 = w1; w1 = w2; w2 = w3; }
    const uint32_t sh = (off & 7u) * 8;
    o0 = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
    o1 = sh ? (w1 >> sh) | (w2 << (64 - sh)) : w1;
}
// zeros from byte cnt on (cnt < 16)
__device__ __forceinline__ void sp_keep_bytes(uint32_t cnt, uint64_t &o0, uint64_t &o1) {
    o0 &= cnt >= 8 ? ~0ull : (1ull << (8 * cnt)) - 1;
    o1 &= cnt > 8 ? (1ull << (8 * (cnt - 8))) - 1 : 0ull;
}
// the same 16 bytes with ONE unaligned access through a packed struct.  anchor_jobs_kernel alone takes it (PACKED = true in the
// steps below): there the realigned pair measured 1.3 to 1.6 % of the kernel's slot slower than this (profiles/r12/); in
// revcomp_kernel this form measured the slowest of three (locus_kernels.hip [r2]), and the row gathers never had it
struct __attribute__((packed, aligned(1))) SpPacked16 { uint64_t lo, hi; };
__device__ __forceinline__ void sp_load16_packed(const char *src, uint64_t &o0, uint64_t &o1) {
    const SpPacked16 v = *reinterpret_cast<const SpPacked16 *>(src);
    o0 = v.lo; o1 = v.hi;
}
// the straight step: src[0 .. cnt) as the 16 bytes of one aligned store, zeros behind them (PACKED: cnt == 16 only)
template <bool PACKED = false>
__device__ __forceinline__ uint4 sp_row16(const char *src, uint32_t cnt) {
    uint64_t o0, o1;
    if (PACKED) sp_load16_packed(src, o0, o1);
    else sp_load16(src, cnt, o0, o1);
    if (cnt < 16) sp_keep_bytes(cnt, o0, o1);
    return make_uint4((uint32_t) o0, (uint32_t) (o0 >> 32), (uint32_t) o1, (uint32_t) (o1 >> 32));
}
// the mirrored step: comp_base(end[-1 - k]), k in 0 .. cnt, as the 16 bytes of one aligned store, zeros behind them.
// 16 bytes: one realigned load reversed and complemented in registers; fewer (the source span's first bytes): one by one
template <bool PACKED = false>
__device__ __forceinline__ uint4 sp_row16_mirrored(const char *end, uint32_t cnt) {
    if (cnt == 16) {
        uint64_t o0, o1;
        if (PACKED) sp_load16_packed(end - 16, o0, o1);
        else sp_load16(end - 16, 16u, o0, o1);
        const uint32_t w[4] = {(uint32_t) o0, (uint32_t) (o0 >> 32), (uint32_t) o1, (uint32_t) (o1 >> 32)};
        return revcomp16([&](int e) { return w[e]; });
    }
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < cnt; ++k) w[k >> 2] |= (uint32_t) (uint8_t) comp_base(end[-1 - (int) k]) << (8 * (k & 3u));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
