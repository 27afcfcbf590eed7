"""A model of gact_bs_kernel's control flow: which path every pass-1 pair and every pass-2 block of a launch takes, from
the tiles its lanes hold.  Written from the stream-word formulas of gact_bs_kernels.hip, not from its output; the module
docstring of tests/test_gpu_gact_bs_counters.py states the rules.  Nothing here runs an aligner: which tiles a read runs
(tq, tt, and the anti-diagonal of the walk's last step) comes from the reference alignment, tests/gact_ref.py's trace
(`tile_rows`), so a pair with m != n needs no rule of its own.

    _model(tiles, fenced, waves, gact, record=None) -> the counters of the launch (capi.BS_COUNTERS, gact_tiles,
                                                       blocks_per_tile_sum)
    record: a list that gains one dict per wave-tile, in the order the wavefront runs them --
        lanes    {lane: (read, index of the read's tile, (tq, tt, last_step))} of the lanes that have a tile
        S0       the anti-diagonal pass 1 starts at
        masked, plain      pass-1 pairs
        blocks   one letter per pass-2 block that ran: "F" full width, "W" on the 32-point window
        skipped  blocks left out because no lane still walked
"""
import functools

from gact_cases import BS_K
from longreadmapper_amd import capi


def tile_rows(ops, trace):
    """[(tq, tt, anti-diagonal of the walk's last step)] per tile of one alignment of gact_ref."""
    at, row = 0, []
    for t in trace:
        a = b = 0
        while (a, b) != t["stop"]:
            last_step = a + b
            op = ops[at]
            at += 1
            a, b = a + (op != ord("D")), b + (op != ord("I"))
        row.append((t["tq"], t["tt"], last_step))
    assert at + trace.tail == len(ops)
    return row


def _holds(q_words, d_words, tqs, tts):
    return any(0 <= a - tq < 32 for a in q_words for tq in tqs) or any(0 <= tt - b < 32 for b in d_words for tt in tts)


@functools.lru_cache(maxsize=1 << 16)
def _paths(tqs, tts, S0, gact):
    """What a wave-tile's paths depend on -- the tq and the tt its lanes hold and where pass 1 starts:
    -> (masked pairs, plain pairs, per pass-2 block: full width?)"""
    T_, O_, W_ = gact
    narrow = W_ < 128
    nblk = (2 * (T_ - O_) + BS_K - 1) // BS_K
    nb = min(nblk, S0 // BS_K)
    A0 = (S0 + 64) >> 1
    B0 = S0 - A0
    qw, qnext = [A0, A0 - 32, A0 - 64], A0 - 96
    dw, dnext = [B0 - 31, B0 + 1, B0 + 33], B0 - 63
    shq, shd = 0, 31
    hb = narrow or _holds(qw, dw, tqs, tts)
    s = S0
    pairs = [0, 0]
    while True:
        pairs[0 if hb else 1] += 1
        if s == BS_K:
            break
        shq += 1
        if shq == 32:
            qw, qnext, shq = [qw[1], qw[2], qnext], qnext - 32, 0
            hb = narrow or _holds(qw, dw, tqs, tts)
        if shd == 0:
            dw, dnext, shd = [dnext, dw[0], dw[1]], dnext - 32, 32
            hb = narrow or _holds(qw, dw, tqs, tts)
        shd -= 1
        s -= 2
    # (where the walk's last block stays 32 bases short of T: T = 320, O = 120 does, O = 0 does not)
    only_full_tiles = tqs == {T_} and tts == {T_} and BS_K // 2 * nblk + 63 < T_
    full = []
    for c in range(nb):
        a_hi, b_lo = BS_K // 2 * (c + 1) + 31, BS_K // 2 * c - 32
        full.append(narrow or _holds([a_hi, a_hi - 32, a_hi - 64], [b_lo, b_lo + 32, b_lo + 64], tqs, tts))
        assert narrow or not (full[c] and only_full_tiles), "a wave-tile of whole tiles has no free-exit point in pass 2"
    return pairs[0], pairs[1], tuple(full)


def _tile(cnt, lanes, gact, rec=None):
    """One wave-tile.  lanes: (tq, tt, last_step) of the lanes that have a tile."""
    S0 = (max(l[0] + l[1] for l in lanes) + BS_K - 1) // BS_K * BS_K
    masked, plain, full = _paths(frozenset(l[0] for l in lanes), frozenset(l[1] for l in lanes), S0, tuple(gact))
    cnt["bs_pass1_pairs_masked"] += masked
    cnt["bs_pass1_pairs_plain"] += plain
    nb, last, blocks, skipped = len(full), max(l[2] for l in lanes), "", 0
    for c in range(nb):
        if last < BS_K * c:                   # no lane's walk has a step at or beyond this block
            skipped = nb - c
            break
        cnt["bs_blocks_full" if full[c] else "bs_blocks_windowed"] += 1
        blocks += "F" if full[c] else "W"
    cnt["bs_blocks_skipped"] += skipped
    cnt["blocks_per_tile_sum"] += nb
    if rec is not None:
        rec.update(S0=S0, blocks=blocks, skipped=skipped, masked=masked, plain=plain)


def _wave(cnt, take, n_reads, tiles, fenced, gact, record=None):
    """One wavefront to its end.  take(k) -> first of k queue tickets."""
    lane = [None] * 64                        # [read, next tile] of a lane that has a read
    exhausted = [False] * 64
    while True:
        for l in range(64):
            if lane[l] and lane[l][1] == len(tiles[lane[l][0]]):
                lane[l] = None
        while True:
            need = [l for l in range(64) if lane[l] is None and not exhausted[l]]
            if not need:
                break
            cnt["bs_refill_rounds"] += 1
            base = take(len(need))
            for k, l in enumerate(need):
                r = base + k
                if r >= n_reads:
                    exhausted[l] = True
                elif r not in fenced:
                    lane[l] = [r, 0]
        live = [l for l in range(64) if lane[l]]
        if not live:
            return
        cnt["bs_wave_tiles"] += 1
        cnt["gact_tiles"] += len(live)
        rec = None
        if record is not None:
            rec = dict(lanes={l: (lane[l][0], lane[l][1], tiles[lane[l][0]][lane[l][1]]) for l in live})
            record.append(rec)
        _tile(cnt, [tiles[lane[l][0]][lane[l][1]] for l in live], gact, rec)
        for l in live:
            lane[l][1] += 1


def _model(tiles, fenced, waves, gact, record=None):
    """The whole launch.  One wavefront: the queue is its own.  More (the batch must fit the grid and hold no fenced read):
    each takes one run of 64 tickets, whichever comes first, and finds the queue empty afterwards."""
    n = len(tiles)
    cnt = dict.fromkeys(capi.BS_COUNTERS + ("gact_tiles", "blocks_per_tile_sum"), 0)
    if waves == 1:
        head = [0]

        def take(k):
            head[0] += k
            return head[0] - k
        _wave(cnt, take, n, tiles, fenced, gact, record)
    else:
        assert not fenced and n <= 64 * waves
        for w in range(waves):
            first = [64 * w]
            _wave(cnt, lambda k: first.pop() if first else n, n, tiles, fenced, gact, record)
    return cnt
