"""The bit-sliced GACT kernel's traceback block on a 32-point window, on the CPU: longreadmapper_amd/csrc/gact_bs_circuit.h
is compiled with gcc and one block is recomputed and walked twice from the same checkpoint and stream words -- in full
width (64 lattice points per anti-diagonal, the form the kernel keeps for blocks with a free-exit point or a narrow
band) and on the window of the lane's entry point (bs_win_origin / bs_win_cut_* / bs_win_block / bs_walk_block_win):

  * every decision bit a walk from the entry point could read is the same in both forms, for every entry bit 0..63,
    entry on the block's first or second anti-diagonal, random and constant checkpoints and sequences;
  * walks that pin the window's edges (31 / 32 insertions or deletions in a row, alternating, all diagonal) read the
    same bits through the window as through the full planes;
  * recompute + walk end to end: equal code words, code counts, na / nb / ns, score and `running`, including walks
    that stop inside the block, blocks across anti-diagonal 2(T-O), and lanes that do not walk."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "gact_bs_window_harness.c")
HDR = os.path.join(HERE, "..", "longreadmapper_amd", "csrc", "gact_bs_circuit.h")
LIB = os.path.join(HERE, "models", "libgact_bs_window_harness.so")
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
T, O = 320, 120
LIM2 = 2 * (T - O)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", LIB, SRC])
    so = C.CDLL(LIB)
    so.bsw_block_full.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    so.bsw_block_full.restype = None
    so.bsw_block_win.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    so.bsw_block_win.restype = C.c_uint32
    so.bsw_walk_full.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    so.bsw_walk_full.restype = C.c_uint64
    so.bsw_walk_win.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    so.bsw_walk_win.restype = C.c_uint64
    assert so.bsw_block_steps() == 32
    return so


K = 32


def _reach(k, t0):
    """Plane bits of anti-diagonal k of the block that a walk entering at bit t0 of k = 0 (or bit t0 - 1 of k = 1) can be on."""
    lo, hi = (t0 - k // 2, t0 + k // 2) if k % 2 == 0 else (t0 - (k + 1) // 2, t0 + (k - 1) // 2)
    return max(lo, 0), min(hi, 63)


def _inputs(rng, kind):
    """A checkpoint (8 words) and the stream words of the four sequence planes (12 words)."""
    ck = rng.integers(0, 1 << 32, size=8, dtype=np.uint64).astype(np.uint32)
    seq = rng.integers(0, 1 << 32, size=12, dtype=np.uint64).astype(np.uint32)
    if kind == "match":                        # one base everywhere: every lattice point a match
        seq[:] = 0
    elif kind == "mismatch":
        seq[:6] = 0
        seq[6:] = M32
    elif kind == "zero_state":                 # every difference -1 (code 0), the value out-of-band points have
        ck[:] = 0
    elif kind == "tile_start":                 # the state pass 1 starts a tile from: V = H = 0 (code 1)
        ck[:] = [0, 0, M32, M32, 0, 0, M32, M32]
    elif kind == "mostly_match":               # text = read shifted: long diagonals with a gap here and there
        seq[6:] = seq[:6] ^ (rng.integers(0, 1 << 32, size=6, dtype=np.uint64).astype(np.uint32) &
                              rng.integers(0, 1 << 32, size=6, dtype=np.uint64).astype(np.uint32) &
                              rng.integers(0, 1 << 32, size=6, dtype=np.uint64).astype(np.uint32))
    return ck, seq


KINDS = ["random", "match", "mismatch", "zero_state", "tile_start", "mostly_match"]


def _full(lib, ck, seq):
    pl = np.zeros(4 * K, dtype=np.uint32)
    lib.bsw_block_full(ck.ctypes.data, seq.ctypes.data, pl.ctypes.data)
    n = [int(pl[4 * k]) | (int(pl[4 * k + 1]) << 32) for k in range(K)]
    g = [int(pl[4 * k + 2]) | (int(pl[4 * k + 3]) << 32) for k in range(K)]
    return pl, n, g


def _win(lib, ck, seq, t0):
    pl = np.zeros(2 * K, dtype=np.uint32)
    o = lib.bsw_block_win(ck.ctypes.data, seq.ctypes.data, t0, pl.ctypes.data)
    return pl, o


def test_origin_keeps_the_window_inside_the_plane_and_over_the_reach(lib):
    pl = np.zeros(2 * K, dtype=np.uint32)
    ck, seq = _inputs(np.random.default_rng(1), "random")
    for t0 in list(range(-70, 140)) + [-(1 << 31), (1 << 31) - 1, -(1 << 30), 1 << 30]:      # any nb a dead lane may hold
        o = lib.bsw_block_win(ck.ctypes.data, seq.ctypes.data, t0, pl.ctypes.data)
        assert 0 <= o <= 32
        if 0 <= t0 <= 64:
            assert o == min(max(t0 - 16, 0), 32)
            for k in range(K):
                lo, hi = _reach(k, t0)
                assert o <= lo and hi <= o + 31, (t0, k)
    assert _reach(31, 32) == (16, 47) and _reach(30, 32) == (17, 47)          # 32 of 32 bits on the last anti-diagonal


@pytest.mark.parametrize("kind", KINDS)
def test_window_decisions_equal_full_width_on_every_reachable_point(lib, kind):
    rng = np.random.default_rng(100 + KINDS.index(kind))
    for it in range(40 if kind in ("random", "mostly_match") else 6):
        ck, seq = _inputs(rng, kind)
        _, n64, g64 = _full(lib, ck, seq)
        for t0 in range(0, 65):                 # 64: entry on bit 63 of the block's second anti-diagonal
            pl, o = _win(lib, ck, seq, t0)
            for k in range(K):
                lo, hi = _reach(k, t0)
                if lo > hi:
                    continue
                mask = ((1 << (hi - lo + 1)) - 1) << lo
                assert (int(pl[2 * k]) << o) & mask == n64[k] & mask, (kind, it, t0, k, "N")
                assert (int(pl[2 * k + 1]) << o) & mask == g64[k] & mask, (kind, it, t0, k, "G")


# ---------------------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------------------
def _state(c, t0, parity, amax=T, bmax=T, score=0):
    """A lane standing on plane bit t0 of anti-diagonal K*c (parity 0), or on bit t0 - 1 of K*c + 1 (parity 1)."""
    b = t0 + (K // 2) * c - 32
    a = K * c + parity - b
    return np.array([a - amax, b - bmax, a + b - LIM2, score], dtype=np.int32), bmax - (K // 2) * c + 32


def _walk_both(lib, full_pl, win_pl, o, st, c, boff):
    sf, sw = st.copy(), st.copy()
    ef, ew, rf, rw = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
    bf = lib.bsw_walk_full(sf.ctypes.data, full_pl.ctypes.data, K * c, LIM2, boff, C.byref(ef), C.byref(rf))
    bw = lib.bsw_walk_win(sw.ctypes.data, win_pl.ctypes.data, K * c, LIM2, boff, o, C.byref(ew), C.byref(rw))
    got = (int(bw), ew.value, [int(x) for x in sw], rw.value)
    want = (int(bf), ef.value, [int(x) for x in sf], rf.value)
    return got, want


def _cut(n64, g64, o):
    pl = np.zeros(2 * K, dtype=np.uint32)
    for k in range(K):
        pl[2 * k] = (n64[k] >> o) & M32
        pl[2 * k + 1] = (g64[k] >> o) & M32
    return pl


def _pack(n64, g64):
    pl = np.zeros(4 * K, dtype=np.uint32)
    for k in range(K):
        pl[4 * k:4 * k + 4] = [n64[k] & M32, n64[k] >> 32, g64[k] & M32, g64[k] >> 32]
    return pl


def _codes(bw, e2):
    return [(bw >> (2 * i)) & 3 for i in range(e2 // 2)]


def test_walks_that_pin_the_window(lib):
    """Constant decision planes: the walk's own bit arithmetic through the window against the full planes."""
    ins = ([M64] * K, [0] * K)                                              # 'I' everywhere: down one bit every second step
    dele = ([M64] * K, [M64] * K)                                           # 'D': up one bit every second step
    zig = ([M64] * K, [M64 if k % 2 else 0 for k in range(K)])
    zag = ([M64] * K, [0 if k % 2 else M64 for k in range(K)])
    diag = ([0] * K, [M64] * K)
    miss = ([0] * K, [0] * K)
    for name, (n64, g64), t0s in [("ins", ins, range(16, 65)), ("del", dele, range(0, 49)), ("zig", zig, range(1, 64)),
                                  ("zag", zag, range(1, 64)), ("diag", diag, range(0, 65)), ("miss", miss, range(0, 65))]:
        full_pl = _pack(n64, g64)
        for c in (4, 5, 11, 12):
            for parity in (0, 1):
                for t0 in t0s:
                    if parity == 1 and t0 == 0:
                        continue
                    o = min(max(t0 - 16, 0), 32)
                    st, boff = _state(c, t0, parity)
                    got, want = _walk_both(lib, full_pl, _cut(n64, g64, o), o, st, c, boff)
                    assert got == want, (name, c, parity, t0)
                    if c < 11 and name in ("ins", "del"):                    # 32 in a row from the first, 31 from the second
                        assert want[1] == 2 * (K - parity) and set(_codes(*want[:2])) == {2 if name == "ins" else 3}
                    if c < 11 and name in ("diag", "miss"):
                        assert want[1] == K


def test_block_end_to_end(lib):
    rng = np.random.default_rng(5)
    n_cases = stopped = 0
    for it in range(36):
        kind = KINDS[it % len(KINDS)]
        ck, seq = _inputs(rng, kind)
        full_pl, n64, g64 = _full(lib, ck, seq)
        c = (4, 5, 11, 12)[it % 4]                                          # 12: the block that holds anti-diagonal 2(T-O)
        for parity in (0, 1):
            for t0 in range(parity, 64 + parity):
                win_pl, o = _win(lib, ck, seq, t0)
                variants = [dict(), dict(score=int(rng.integers(0, 5000)))]
                st0, _ = _state(c, t0, parity)
                a0, b0 = int(st0[0]) + T, int(st0[1]) + T
                variants.append(dict(amax=a0 + int(rng.integers(1, 12))))    # stops inside the block: read exhausted
                variants.append(dict(bmax=b0 + int(rng.integers(1, 12))))    # text exhausted
                for v in variants:
                    st, boff = _state(c, t0, parity, **v)
                    got, want = _walk_both(lib, full_pl, win_pl, o, st, c, boff)
                    assert got == want, (kind, it, c, parity, t0, v)
                    n_cases += 1
                    # the decision bits along the walk, read from both sets of planes
                    a, b = int(st[0]) + v.get("amax", T), int(st[1]) + v.get("bmax", T)
                    for code in _codes(*want[:2]):
                        s = a + b
                        k = s - K * c
                        t = b - (s // 2 - 32 + (s & 1))
                        assert 0 <= k < K and 0 <= t <= 63 and 0 <= t - o <= 31
                        assert ((n64[k] >> t) & 1, (g64[k] >> t) & 1) == (code >> 1, code & 1)
                        assert ((int(win_pl[2 * k]) >> (t - o)) & 1, (int(win_pl[2 * k + 1]) >> (t - o)) & 1) == (code >> 1, code & 1)
                        a += code != 3
                        b += code != 2
                    assert want[3] == int(a < v.get("amax", T) and b < v.get("bmax", T) and a + b < LIM2)
                    stopped += not want[3]
                # a walk that stopped in an earlier block, and a lane that holds no read: nothing moves, whatever the window
                for dead in (np.array([st0[0], st0[1], int(st0[2]) & ~0x40000000, 7], dtype=np.int32),
                             np.array([0, 0, 0, 0], dtype=np.int32)):
                    boff = T - (K // 2) * c + 32
                    od = min(max(int(dead[1]) + boff - 16, 0), 32)
                    wpl, o2 = _win(lib, ck, seq, int(dead[1]) + boff)
                    assert o2 == od
                    got, want = _walk_both(lib, full_pl, wpl, od, dead, c, boff)
                    assert got == want and want[:2] == (0, 0) and want[2] == [int(x) for x in dead]
    assert n_cases > 15000 and stopped > 5000                             # most of the short walks did stop inside
