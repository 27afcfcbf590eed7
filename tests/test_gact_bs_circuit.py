"""The lane-local arithmetic of the bit-sliced GACT kernel, on the CPU: longreadmapper_amd/csrc/gact_bs_circuit.h is
compiled with gcc (its truth tables evaluated bit by bit instead of by v_bitop3_b32) and checked against the
definitions it implements:

  * the difference circuit against X = max(s, u-1, w-1), V = X - u, H = X - w and the spec's tie order
    (DIAG iff s >= u-1 and s >= w-1, else INS iff u >= w), with and without the free-exit / band masks;
  * the walk's bookkeeping (na, nb, ns, the stopped bit, codes in 32-bit halves, the score counted from the code
    words) against the plain form: a, b, score and `running` updated step by step."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "gact_bs_circuit_harness.c")
HDR = os.path.join(HERE, "..", "longreadmapper_amd", "csrc", "gact_bs_circuit.h")
LIB = os.path.join(HERE, "models", "libgact_bs_circuit_harness.so")
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", LIB, SRC])
    so = C.CDLL(LIB)
    so.bsc_half.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    so.bsc_half.restype = None
    so.bsc_walk_block.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    so.bsc_walk_block.restype = C.c_uint64
    return so


# ---------------------------------------------------------------------------------------------------------
# the difference circuit
# ---------------------------------------------------------------------------------------------------------
def _point(match, u, w):
    """One lattice point from the arithmetic definition: codes are value + 1."""
    s, uv, wv = (1 if match else -1), u - 1, w - 1
    x = max(s, uv - 1, wv - 1)
    diag = s >= uv - 1 and s >= wv - 1
    n = 0 if diag else 1
    g = (1 if match else 0) if diag else (1 if uv < wv else 0)      # N ? deletion : match
    return x - uv + 1, x - wv + 1, n, g


def _half_ref(words, bound):
    u1, u0, w1, w0, ql, qh, dl, dh, bm, band = [int(x) for x in words]
    out = [0] * 6
    for bit in range(32):
        b = lambda x: (x >> bit) & 1
        match = b(ql) == b(dl) and b(qh) == b(dh)
        v, h, n, g = _point(match, 2 * b(u1) + b(u0), 2 * b(w1) + b(w0))
        assert 0 <= v <= 3 and 0 <= h <= 3
        if bound:
            if not b(band):
                v = h = 0            # outside the band: -1, the value that never wins
            elif b(bm):
                v = h = 1            # free exit: V = H = 0
        for i, val in enumerate((v >> 1, v & 1, h >> 1, h & 1, n, g)):
            out[i] |= val << bit
    return out


def _half(lib, words, bound, track):
    a = np.array(words, dtype=np.uint32)
    o = np.zeros(6, dtype=np.uint32)
    lib.bsc_half(bound, track, a.ctypes.data, o.ctypes.data)
    return [int(x) for x in o]


@pytest.mark.parametrize("bound", [0, 1])
def test_circuit_all_input_combinations(lib, bound):
    full = lambda bit: M32 if bit else 0
    for match in (0, 1):
        for u in range(4):
            for w in range(4):
                for q in range(4):                       # every base pair that gives this `match`
                    d = q if match else (q + 1 + (u + w) % 3) % 4
                    masks = [(0, M32)] if not bound else [(0, M32), (M32, M32), (0, 0), (M32, 0), (0x0F0F00FF, 0x33CC0FF0)]
                    for bm, band in masks:
                        words = [full(u >> 1), full(u & 1), full(w >> 1), full(w & 1), full(q & 1), full(q >> 1),
                                 full(d & 1), full(d >> 1), bm, band]
                        want = _half_ref(words, bound)
                        got = _half(lib, words, bound, 1)
                        assert got == want, (match, u, w, q, d, bm, band)
                        assert _half(lib, words, bound, 0)[:4] == want[:4]


@pytest.mark.parametrize("bound", [0, 1])
def test_circuit_random_words(lib, bound):
    rng = np.random.default_rng(20 + bound)
    for _ in range(1500):
        words = [int(x) for x in rng.integers(0, 1 << 32, size=10, dtype=np.uint64)]
        assert _half(lib, words, bound, 1) == _half_ref(words, bound)


# ---------------------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------------------
def _walk_ref(planes, nblocks, K, amax, bmax, smax, act):
    """The plain form: a, b, score, running; one 64-bit code word per block."""
    a = b = score = 0
    running = act
    out = []
    for c in range(nblocks):
        out.append(None)
        start_running = running
        bw, e2 = 0, 0
        for k in range(K):
            on = running and a + b == K * c + k
            dd = (b - a + 64) & M32
            up = dd >= 64
            n_pl, g_pl = planes[c][k]
            nbit = ((n_pl >> 32 if up else n_pl & M32) >> ((dd >> 1) & 31)) & 1
            gbit = ((g_pl >> 32 if up else g_pl & M32) >> ((dd >> 1) & 31)) & 1
            if on:
                code = 2 * nbit + gbit
                bw |= code << e2
                e2 += 2
                score += code != 1
                a += code != 3
                b += code != 2
            running = running and a < amax and b < bmax and a + b < smax
        out[c] = (start_running, bw, e2, a, b, score, running)
    return out


def _walk_new(lib, planes, nblocks, K, amax, bmax, lim2, act, score0=0):
    st = np.array([-amax if act else 0, -bmax if act else 0, -lim2 if act else 0, score0], dtype=np.int32)
    out = []
    running = C.c_int(1 if act else 0)
    for c in range(nblocks):
        start_running = bool(running.value)
        pl = np.zeros(4 * K, dtype=np.uint32)
        for k in range(K):
            n_pl, g_pl = planes[c][k]
            pl[4 * k:4 * k + 4] = [n_pl & M32, n_pl >> 32, g_pl & M32, g_pl >> 32]
        e2 = C.c_uint32()
        bw = lib.bsc_walk_block(st.ctypes.data, pl.ctypes.data, K * c, lim2, bmax - (K // 2) * c + 32, C.byref(e2),
                                C.byref(running))
        out.append((start_running, int(bw), e2.value, int(st[0]) + amax if act else 0, int(st[1]) + bmax if act else 0,
                    int(st[3]), bool(running.value)))
    return out


def _planes(rng, nblocks, K, p_gap, p_g=0.5):
    bits = lambda p: int(np.packbits(rng.random(64) < p, bitorder="little").view(np.uint64)[0])
    return [[(bits(p_gap), bits(p_g)) for _ in range(K)] for _ in range(nblocks)]


def _check_walk(lib, planes, T, O, tq, tt, last, act=True):
    K = lib.bsc_block_steps()
    cap = T - O
    lim2 = 2 * cap
    nblocks = (lim2 + K - 1) // K
    amax = tq if last else min(tq, cap)
    bmax = tt if last else min(tt, cap)
    smax = lim2 if last else 0x7fffffff
    want = _walk_ref(planes, nblocks, K, amax, bmax, smax, act)
    got = _walk_new(lib, planes, nblocks, K, amax, bmax, lim2, act)
    assert got == want, (T, O, tq, tt, last)
    return want


def test_walk_random_planes(lib):
    K = lib.bsc_block_steps()
    rng = np.random.default_rng(7)
    for it in range(300):
        T, O = [(320, 120), (512, 120), (128, 32), (64, 16), (33, 7), (100, 99), (512, 0)][it % 7]
        nblocks = (2 * (T - O) + K - 1) // K
        last = bool(it % 3 == 0)
        tq = int(rng.integers(1, T + 1)) if it % 2 else T
        tt = int(rng.integers(1, T + 1)) if it % 5 else T
        p_gap = [0.0, 0.05, 0.3, 0.6, 1.0][it % 5]
        _check_walk(lib, _planes(rng, nblocks, K, p_gap, [0.5, 0.1, 0.9][it % 3]), T, O, tq, tt, last, act=it % 11 != 10)


def test_walk_stops_at_all_three_limits_in_one_step(lib):
    K = lib.bsc_block_steps()
    T, O = 320, 120
    nblocks = (2 * (T - O) + K - 1) // K
    diag = [[(0, 0xFFFFFFFFFFFFFFFF)] * K for _ in range(nblocks)]           # '=' everywhere
    for tq, tt, last in [(200, 200, True), (320, 320, True), (320, 320, False), (1, 1, True), (1, 300, False), (300, 1, True),
                         (201, 199, True), (199, 201, True)]:
        res = _check_walk(lib, diag, T, O, tq, tt, last)
        assert res[-1][3] == res[-1][4] == min(tq, tt, T - O)
    # the walk may pass anti-diagonal 2(T-O) with a diagonal step from the one below it: 399 -> 401
    odd = [[(0xFFFFFFFFFFFFFFFF if (c, k) == (0, 0) else 0, 0)] * 1 for c in range(nblocks) for k in range(K)]
    odd = [[odd[c * K + k][0] for k in range(K)] for c in range(nblocks)]
    res = _check_walk(lib, odd, T, O, 320, 320, True)
    assert res[-1][3] + res[-1][4] == 2 * (T - O) + 1


def test_walk_crosses_the_plane_halves(lib):
    """A path that alternates insertions and deletions around the main diagonal changes between bit 31 and bit 32 of
    the planes, and one that only inserts (or only deletes) leaves the main diagonal by one bit every second step."""
    K = lib.bsc_block_steps()
    T, O = 320, 120
    nblocks = (2 * (T - O) + K - 1) // K
    ones = 0xFFFFFFFFFFFFFFFF
    zig = [[(ones, ones if k % 2 else 0) for k in range(K)] for _ in range(nblocks)]
    zag = [[(ones, 0 if k % 2 else ones) for k in range(K)] for _ in range(nblocks)]
    ins = [[(ones, 0)] * K for _ in range(nblocks)]
    dele = [[(ones, ones)] * K for _ in range(nblocks)]
    for planes in (zig, zag, ins, dele):
        for tq, tt, last in [(320, 320, True), (320, 320, False), (40, 320, True), (320, 40, True)]:
            _check_walk(lib, planes, T, O, tq, tt, last)
    rng = np.random.default_rng(11)
    for _ in range(40):                        # gaps only where the path is within a few bits of the boundary
        band = ((1 << 36) - 1) ^ ((1 << 28) - 1)
        planes = [[(int(rng.integers(0, 1 << 63)) & band, int(rng.integers(0, 1 << 63))) for _ in range(K)]
                  for _ in range(nblocks)]
        _check_walk(lib, planes, T, O, 320, 320, True)
