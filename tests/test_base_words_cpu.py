"""The word forms of the byte kernels (longreadmapper_amd/csrc/base_words.h: four bases or four CIGAR columns per
instruction) on the CPU: the header is compiled with gcc, its v_perm_b32 written out in software from the ISA's
description, and every word function is compared with the per-byte definition it replaces -- the one next to it in the
header and the same definition restated here (base_code, comp_base, the ACGT test of the planar pack, the CIGAR byte of
a column code) -- on

  * every byte value 0 .. 255 in each of the four positions, the other three held at 'A', at 't' and at 'N';
  * the 4^4 words of ACGT only;
  * 10^5 seeded random words;
  * for ops4: all 256 code bytes with 0, 1, 2, 3 and 4 coded columns in the dword."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "base_words_harness.c")
HDR = os.path.join(HERE, "..", "longreadmapper_amd", "csrc", "base_words.h")
LIB = os.path.join(HERE, "models", "libbase_words_harness.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", LIB, SRC])
    so = C.CDLL(LIB)
    for name in ("bwh_codes4", "bwh_letters4", "bwh_not_acgt4", "bwh_pack8"):
        getattr(so, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        getattr(so, name).restype = None
    for name in ("bwh_comp4", "bwh_revcomp4"):
        getattr(so, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(so, name).restype = None
    so.bwh_ops4.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    so.bwh_ops4.restype = None
    so.bwh_perm.argtypes = [C.c_uint32] * 3
    so.bwh_perm.restype = C.c_uint32
    return so


# ---------------------------------------------------------------------------------------------------------
# the per-byte definitions, as tables over the 256 byte values
# ---------------------------------------------------------------------------------------------------------
B = np.arange(256, dtype=np.uint32)
CODE = ((B >> 1) ^ (B >> 2)) & 3                                        # base_code
IS_ACGT = np.isin(B, [ord(c) for c in "ACGT"])
COMP = np.full(256, ord("N"), dtype=np.uint32)                          # comp_base: case folded, anything else -> N
for a, b in zip("ACGTacgt", "TGCATGCA"):
    COMP[ord(a)] = ord(b)
LETTER = np.array([ord(c) for c in "ACGT"], dtype=np.uint32)            # the letter of a code
OP = np.array([ord(c) for c in "X=ID"], dtype=np.uint32)                # the CIGAR byte of a column code


def _bytes(x):
    return np.stack([(x >> (8 * e)) & 0xFF for e in range(4)], axis=1)


def _word(b):
    return (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)).astype(np.uint32)


def _words():
    out = []
    for fill in "AtN":                                 # every byte value in every position
        for pos in range(4):
            b = np.full((256, 4), ord(fill), dtype=np.uint32)
            b[:, pos] = B
            out.append(_word(b))
    acgt = np.array([ord(c) for c in "ACGT"], dtype=np.uint32)
    g = np.stack(np.meshgrid(acgt, acgt, acgt, acgt, indexing="ij"), axis=-1).reshape(-1, 4)
    out.append(_word(g))                               # the 4^4 words of ACGT only
    rng = np.random.default_rng(1010)
    out.append(rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64).astype(np.uint32))
    lo = rng.choice(np.array([ord(c) for c in "ACGTacgtNn"], dtype=np.uint32), size=(20_000, 4))
    out.append(_word(lo))                              # mostly letters: the words that take the word form of comp4
    return np.ascontiguousarray(np.concatenate(out))


WORDS = _words()


def _run(fn, x, *extra, n_out=2):
    outs = [np.zeros(len(x), dtype=np.uint32) for _ in range(n_out)]
    fn(x.ctypes.data, len(x), *extra, *[o.ctypes.data for o in outs])
    return outs


def _same(got, want_c, want_py, x):
    bad = np.nonzero((got != want_py) | (want_c != want_py))[0]
    assert bad.size == 0, "word 0x%08x: word form 0x%08x, header's per-byte form 0x%08x, definition 0x%08x" % (
        x[bad[0]], got[bad[0]], want_c[bad[0]], want_py[bad[0]])


def test_software_perm_follows_the_isa(lib):
    s0, s1 = 0xB7A6F5E4, 0x83C2D1F0            # bytes 0 .. 3 of {s0, s1} are s1's
    assert lib.bwh_perm(s0, s1, 0x03020100) == s1
    assert lib.bwh_perm(s0, s1, 0x07060504) == s0
    assert lib.bwh_perm(s0, s1, 0x00010203) == 0xF0D1C283          # the byte swap
    assert lib.bwh_perm(s0, s1, 0x0C0D0EFF) == 0x00FFFFFF          # 12: 0x00, 13 and above: 0xFF
    # 8 .. 11: the sign of bytes 1, 3, 5, 7 of {s0, s1}: 0xD1 (set), 0x83 (set), 0xF5 (set), 0xB7 (set)
    assert lib.bwh_perm(s0, s1, 0x0B0A0908) == 0xFFFFFFFF
    assert lib.bwh_perm(0x37A675E4, 0x03C251F0, 0x0B0A0908) == 0x00000000
    assert lib.bwh_perm(0x37A6F5E4, 0x83C251F0, 0x0B0A0908) == 0x00FFFF00


def test_codes4(lib):
    got, want = _run(lib.bwh_codes4, WORDS)
    _same(got, want, _word(CODE[_bytes(WORDS)]), WORDS)
    assert [int(CODE[ord(c)]) for c in "ACGT"] == [0, 1, 2, 3]


def test_letters4(lib):
    got, want = _run(lib.bwh_letters4, WORDS)
    _same(got, want, _word(LETTER[CODE[_bytes(WORDS)]]), WORDS)


def test_not_acgt4(lib):
    got, want = _run(lib.bwh_not_acgt4, WORDS)
    ref = (~IS_ACGT[_bytes(WORDS)]).any(axis=1).astype(np.uint32)
    _same(got, want, ref, WORDS)
    assert ref.sum() > 0 and (ref == 0).sum() >= 256


def test_pack8(lib):
    got, want = _run(lib.bwh_pack8, WORDS)
    c = CODE[_bytes(WORDS)]
    _same(got, want, (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint32), WORDS)


def test_comp4_with_its_byte_exact_path(lib):
    got, want, took = _run(lib.bwh_comp4, WORDS, n_out=3)
    b = _bytes(WORDS)
    _same(got, want, _word(COMP[b]), WORDS)
    letters = np.isin(b, [ord(c) for c in "ACGTacgt"]).all(axis=1)
    assert np.array_equal(took != 0, letters)          # the word form runs exactly on the words of letters
    assert letters.sum() > 5_000 and (~letters).sum() > 5_000           # both paths are well represented


def test_revcomp4_with_its_byte_exact_path(lib):
    got, want, took = _run(lib.bwh_revcomp4, WORDS, n_out=3)
    b = _bytes(WORDS)
    _same(got, want, _word(COMP[b[:, ::-1]]), WORDS)
    assert np.array_equal(took != 0, np.isin(b, [ord(c) for c in "ACGTacgt"]).all(axis=1))


@pytest.mark.parametrize("nv", [0, 1, 2, 3, 4])
def test_ops4_all_code_bytes(lib, nv):
    c8 = np.arange(256, dtype=np.uint32)
    got, want = _run(lambda p, n, *o: lib.bwh_ops4(p, n, nv, *o), c8)
    cols = np.stack([OP[(c8 >> (2 * e)) & 3] if e < nv else np.full(256, ord("I"), dtype=np.uint32) for e in range(4)], axis=1)
    _same(got, want, _word(cols), c8)
