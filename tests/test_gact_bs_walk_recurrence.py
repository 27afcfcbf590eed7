"""The walk through a traceback block of the bit-sliced GACT kernel, on the CPU: longreadmapper_amd/csrc/gact_bs_circuit.h
is compiled as C and bs_walk_block / bs_walk_block_win (`on` by recurrence from one comparison per block, the stop rule
inside the block on na, nb and the entry ns, ns brought up to date once behind the block) are compared with the step they
replaced, kept as a reference inside tests/models/gact_bs_walk_harness.c (ns == anti-diagonal compared, ns advanced and
the stop rule applied on every step).  Equal must be: na, nb, ns, score, the code word, e2 and `running`.

  * every entry bit of the plane, entry on the block's first and on its second anti-diagonal;
  * random, all-gap (insertions, deletions, alternating) and all-diagonal (match, mismatch) decision planes;
  * walks that stop inside the block at a = amax, at b = bmax, and at anti-diagonal 2(T-O), reached by a gap and passed
    over by a diagonal, in a block that holds BS_WALK_NO_STEP steps (2(T-O) not a multiple of 32);
  * lanes that never walk, and lanes whose walk stopped in an earlier block by each of the three rules;
  * whole tiles block after block from the anchor, where every entry state is one the walk itself produced."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "gact_bs_walk_harness.c")
HDR = os.path.join(HERE, "..", "longreadmapper_amd", "csrc", "gact_bs_circuit.h")
LIB = os.path.join(HERE, "models", "libgact_bs_walk_harness.so")
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
K = 32
STOPPED = 0x40000000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-shared", "-fPIC", "-o", LIB, SRC])
    so = C.CDLL(LIB)
    for f in (so.bswk_walk_ref, so.bswk_walk_full):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        f.restype = C.c_uint64
    so.bswk_walk_win.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    so.bswk_walk_win.restype = C.c_uint64
    assert so.bswk_block_steps() == K
    return so


def _pack(n64, g64):
    pl = np.zeros(4 * K, dtype=np.uint32)
    for k in range(K):
        pl[4 * k:4 * k + 4] = [n64[k] & M32, n64[k] >> 32, g64[k] & M32, g64[k] >> 32]
    return pl


def _planes(rng, kind):
    if kind == "random":
        p_gap = [0.5, 0.1, 0.9][int(rng.integers(0, 3))]
        # gaps only on bits 4 .. 59: a path that starts inside the plane stays inside it, so the full-width and the
        # windowed walk read the same bits
        n64 = [int(sum(1 << b for b in range(4, 60) if rng.random() < p_gap)) for _ in range(K)]
        g64 = [int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(0, 2)) for _ in range(K)]
        return n64, g64
    return {"ins": ([M64] * K, [0] * K), "del": ([M64] * K, [M64] * K),
            "zig": ([M64] * K, [M64 if k % 2 else 0 for k in range(K)]),
            "zag": ([M64] * K, [0 if k % 2 else M64 for k in range(K)]),
            "match": ([0] * K, [M64] * K), "mismatch": ([0] * K, [0] * K)}[kind]


CONST = ["ins", "del", "zig", "zag", "match", "mismatch"]


def _state(c, t0, parity, lim2, amax, bmax, score=0):
    """A lane on plane bit t0 of anti-diagonal K*c (parity 0), or on bit t0 - 1 of K*c + 1 (parity 1)."""
    b = t0 + (K // 2) * c - 32
    a = K * c + parity - b
    return np.array([a - amax, b - bmax, a + b - lim2, score], dtype=np.int32), bmax - (K // 2) * c + 32


def _three(lib, pl, st, c, lim2, boff, win):
    """(code word, e2, [na, nb, ns, score], running) of the reference, the full-width walk and (win) the windowed one."""
    out = []
    for f in (lib.bswk_walk_ref, lib.bswk_walk_full) + ((lib.bswk_walk_win,) if win else ()):
        s = st.copy()
        e2, run, o = C.c_uint32(), C.c_int(), C.c_uint32()
        extra = (C.byref(o),) if f is lib.bswk_walk_win else ()
        bw = f(s.ctypes.data, pl.ctypes.data, K * c, lim2, boff, C.byref(e2), C.byref(run), *extra)
        out.append((int(bw), e2.value, [int(x) for x in s], run.value))
    return out


def _check(lib, pl, st, c, lim2, boff, tag, win=True):
    res = _three(lib, pl, st, c, lim2, boff, win)
    for got in res[1:]:
        assert got == res[0], (tag, [int(x) for x in st], c, lim2, boff)
    return res[0]


# lim2 = 2(T-O): 400 (the default T=320 O=120; block 12 holds 16 steps at or above it), 406 (22), 192 (T=128 O=32: a multiple of 32)
@pytest.mark.parametrize("lim2", [400, 406, 192])
def test_every_entry_bit_and_both_entry_anti_diagonals(lib, lim2):
    rng = np.random.default_rng(lim2)
    T = lim2                                                   # amax = bmax = T: out of the way
    cs = (0, lim2 // K // 2, (lim2 - 1) // K)                  # the last one holds 2(T-O) - 1, and NO_STEP steps unless lim2 % 32 == 0
    n_stop = 0
    for kind in CONST + ["random"] * 6:
        n64, g64 = _planes(rng, kind)
        pl = _pack(n64, g64)
        for c in cs:
            for parity in (0, 1):
                for t0 in range(parity, 64 + parity):
                    st, boff = _state(c, t0, parity, lim2, T, T, score=int(rng.integers(0, 3000)))
                    if int(st[0]) + T < 0 or int(st[1]) + T < 0:
                        continue                               # a or b below the anchor: no lane stands there
                    ref = _check(lib, pl, st, c, lim2, boff, (kind, parity, t0))
                    if c == cs[-1]:
                        assert not ref[3] and ref[2][2] in (0, 1)      # stopped at 2(T-O), or one above after a diagonal
                        n_stop += 1
                    elif kind in ("ins", "del"):
                        assert ref[1] == 2 * (K - parity)
                    elif kind in ("match", "mismatch"):
                        assert ref[1] == K
    assert n_stop > 1000


def test_stops_by_read_end_and_text_end_inside_the_block(lib):
    rng = np.random.default_rng(3)
    lim2, T = 400, 320
    by_a = by_b = 0
    for kind in CONST + ["random"] * 10:
        n64, g64 = _planes(rng, kind)
        pl = _pack(n64, g64)
        for c in (3, 8):
            for parity in (0, 1):
                for t0 in range(8 + parity, 57):
                    st0, _ = _state(c, t0, parity, lim2, T, T)
                    a0, b0 = int(st0[0]) + T, int(st0[1]) + T
                    for lim in (1, 2, 5, 11, 16):
                        st, boff = _state(c, t0, parity, lim2, a0 + lim, T)            # the read ends lim bases on
                        ref = _check(lib, pl, st, c, lim2, boff, (kind, "amax", lim, parity, t0))
                        by_a += ref[2][0] == 0
                        st, boff = _state(c, t0, parity, lim2, T, b0 + lim)            # the text does
                        ref = _check(lib, pl, st, c, lim2, boff, (kind, "bmax", lim, parity, t0))
                        by_b += ref[2][1] == 0
                        st, boff = _state(c, t0, parity, lim2, a0 + lim, b0 + lim)     # both in one step on a diagonal
                        _check(lib, pl, st, c, lim2, boff, (kind, "both", lim, parity, t0))
    assert by_a > 3000 and by_b > 3000


def test_lanes_that_do_not_walk(lib):
    rng = np.random.default_rng(4)
    lim2, T = 400, 320
    for kind in ["random", "ins", "del", "match"]:
        n64, g64 = _planes(rng, kind)
        pl = _pack(n64, g64)
        for c in (0, 1, 5, 12):
            boff = T - (K // 2) * c + 32
            s = K * c
            dead = [[0, 0, 0, 0],                                                      # never had a tile
                    [0, -40, (s - 7 - lim2) & ~STOPPED, 11],                           # read end, seven anti-diagonals back
                    [-40, 0, (s - 1 - lim2) & ~STOPPED, 12],                           # text end on the last one of the block before
                    [0, 0, (s - 2 - lim2) & ~STOPPED, 13],
                    [-3, -5, 0, 14], [-3, -5, 1, 15],                                  # anti-diagonal 2(T-O), and one above
                    [-3, -5, (s - lim2) & ~STOPPED, 16],                               # on this block's first anti-diagonal, bit cleared
                    [-3, -5, (s + 1 - lim2) & ~STOPPED, 17]]
            for d in dead:
                st = np.array([x - (1 << 32) if x >= (1 << 31) else x for x in d], dtype=np.int64).astype(np.int32)
                ref = _check(lib, pl, st, c, lim2, boff, (kind, "dead", d))
                assert ref[:2] == (0, 0) and ref[2] == [int(x) for x in st] and not ref[3]


@pytest.mark.parametrize("T,O", [(320, 120), (128, 32), (323, 120)])
def test_whole_tiles_block_after_block(lib, T, O):
    """From the anchor through every block, as the kernel walks a tile: each block entered in the state the one before left,
    the blocks behind the stop included."""
    rng = np.random.default_rng(T)
    cap = T - O
    lim2 = 2 * cap
    nblocks = (lim2 + K - 1) // K
    ends = {"a": 0, "b": 0, "s": 0}
    for it in range(120):
        last = it % 3 == 0
        tq = int(rng.integers(1, T + 1)) if it % 2 else T
        tt = int(rng.integers(1, T + 1)) if it % 4 >= 2 else T
        amax, bmax = (tq, tt) if last else (min(tq, cap), min(tt, cap))
        act = it % 13 != 12
        kind = "random" if it % 4 else CONST[(it // 4) % len(CONST)]
        sts = [np.array([-amax, -bmax, -lim2, 0] if act else [0, 0, 0, 0], dtype=np.int32) for _ in range(3)]
        for c in range(nblocks):
            n64, g64 = _planes(rng, kind)
            pl = _pack(n64, g64)
            boff = bmax - (K // 2) * c + 32
            t0 = int(sts[0][1]) + boff
            win = 0 <= t0 <= 64
            outs = []
            fs = (lib.bswk_walk_ref, lib.bswk_walk_full, lib.bswk_walk_win)
            for f, s in zip(fs, sts):
                if f is lib.bswk_walk_win and not win:
                    s[:] = sts[0]
                    continue
                e2, run, o = C.c_uint32(), C.c_int(), C.c_uint32()
                extra = (C.byref(o),) if f is lib.bswk_walk_win else ()
                bw = f(s.ctypes.data, pl.ctypes.data, K * c, lim2, boff, C.byref(e2), C.byref(run), *extra)
                outs.append((int(bw), e2.value, [int(x) for x in s], run.value))
            for got in outs[1:]:
                assert got == outs[0], (T, O, it, c, kind)
            if kind in ("ins", "del") and act and outs[0][3]:
                break                                          # a run of gaps leaves the band; the kernel's planes stop it before
        if act:
            na, nb, ns = (int(x) for x in sts[0][:3])
            ends["a"] += na == 0
            ends["b"] += nb == 0
            ends["s"] += ns in (0, 1)
    assert min(ends.values()) > 5, ends
