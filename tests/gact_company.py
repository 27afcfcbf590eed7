"""Companies for the constructed alignments of tests/gact_cases.py: job tables that put a case into a wavefront whose
other lanes hold tiles of their own, because gact_bs_kernel decides per WAVEFRONT where pass 1 starts, which pairs run
masked and which blocks run in full width, and gact3_kernel shares a register and a sweep between the two reads of one.

Nothing here runs an aligner: the module only builds inputs.  A company is a dict --
    kind, name, gact = (T, O, W)
    pairs        [(q, d)] job k is q against d (flagged reads as they go to the device)
    cases        {job: name of the gact_cases case it holds}
    text, toffs  the targets laid out in one text; d_k = text[toffs[k] : toffs[k] + len(d_k)]
    store_stride op bytes per row
    flagged      jobs whose read holds a byte other than ACGT: the bit-sliced kernel leaves them to the byte kernel
    fenced       jobs with meta_r = 0
    pred         pred(tiles, record) -> bool.  tiles[k]: bs_flow.tile_rows of job k's reference alignment; record: what
                 bs_flow._model recorded for the table on ONE wavefront (job k in lane k) -- None for the packed kernel's
                 pairs, whose predicates read the tiles alone.  A company that stops forcing its decision after a
                 constant changes fails its predicate instead of going quiet.
The builders that need to know how long a case lives take `lives`: {case name: tiles of its reference alignment}.

    groups(max_w)                       {(T, O, W): [case]} of gact_cases.cases()
    whole(cases, gact, lives)           the case among 63 clean square reads whose tiles are whole while it lives
    staircase(cases, gact, lives)       ... among clean square reads that end in its wave-tile with tq = tt = 32, 64, ..
                                        -> (companies, names of the cases left out)
    ragged(cases, gact)                 the cases of one (T, O, W), 64 to a table, two shuffles, flagged and fenced jobs
    pairs(cases, gact, lives)           gact3_kernel: the case in either half of a wavefront, next to four partners
"""
import zlib

import numpy as np

import gact_cases
from gact_cases import BS_K, rnd

LANES = 64
STAIR_MAX_TILES = 8
DISTINCT = 7                  # different clean reads among a case's 63 whole-tile companions (neighbouring lanes differ)
PARTNERS = ("whole", "one", "self", "neighbour")


def groups(max_w=128):
    out = {}
    for c in gact_cases.cases():
        if max_w is None or c["W"] <= max_w:
            out.setdefault((c["T"], c["O"], c["W"]), []).append(c)
    return out


def packed_plan(gact):
    """lrm_gact_plan: gact_impl = 3 runs gact3_kernel (W <= 128 and at most 32 traceback words)."""
    T, O, W = gact
    return W <= 128 and ((2 * (T - O) - 1) >> 4) + 1 <= 32


def whole_len(gact, life):
    """The length of a clean square read whose first `life` tiles are whole: it keeps T - O bases per tile."""
    T, O, _ = gact
    return (life - 1) * (T - O) + T


def clean(n, *key):
    s = rnd(n, "company", *key)
    return s, s


def _rng(*key):
    return np.random.default_rng([zlib.crc32(repr(key).encode())])


def _layout(pairs, residues, tag, share=False):
    """One text holding every target; target k starts at a position = residues[k] mod 64 (None: wherever the text stands).
    What follows a target shorter than its read is the read's own continuation -- an alignment that ran past tt would find
    matches there -- then random bases.  share: equal targets are laid out once."""
    text, toffs, seen = bytearray(rnd(7, tag, "head")), [], {}
    for k, (q, d) in enumerate(pairs):
        if share and d in seen:
            toffs.append(seen[d])
            continue
        if residues is not None:
            text += rnd((residues[k] - len(text)) % 64, tag, "gap", k)
        toffs.append(len(text))
        seen[d] = len(text)
        text += d
        text += bytes(c for c in q[len(d):len(d) + 40] if c in b"ACGT")
    text += rnd(50, tag, "tail")
    return bytes(text), toffs


def _company(kind, name, gact, pairs, cases, residues, stride_mod=0, pred=None, flagged=(), fenced=(), share=False, **more):
    text, toffs = _layout(pairs, residues, name, share)
    stride = (max(len(q) + len(d) for q, d in pairs) + 15) // 16 * 16 + stride_mod
    assert all(text[o:o + len(d)] == d for o, (_, d) in zip(toffs, pairs))
    return dict(kind=kind, name=name, gact=gact, pairs=pairs, cases=cases, text=text, toffs=toffs, store_stride=stride,
                flagged=frozenset(flagged), fenced=frozenset(fenced), pred=pred or (lambda tiles, record: True), **more)


def _s0_whole(T):
    return (2 * T + BS_K - 1) // BS_K * BS_K


# ---------------------------------------------------------------------------------------------------------------------
# gact_bs_kernel: one table = one wavefront (bs_waves = 1), job k in lane k
# ---------------------------------------------------------------------------------------------------------------------
def whole(cases, gact, lives):
    """Per case one table: the case in a lane that moves with its index, 63 clean square reads around it (DISTINCT
    different ones in turn: the reference aligns each once), all of the length that keeps every tile whole for the
    longest life in `cases`.  The wavefront's decisions are then those of a whole tile -- pass 1 starts at 2T, far beyond
    a small tile's corner -- and every free-exit point below T is the case's."""
    T = gact[0]
    n = whole_len(gact, max(lives[c["name"]] for c in cases))
    comp = [clean(n, "whole", gact, k % DISTINCT) for k in range(LANES - 1)]
    out = []
    for idx, c in enumerate(cases):
        lane = (7 * idx + 3) % LANES
        life = lives[c["name"]]

        def pred(tiles, record, lane=lane, life=life):
            return len(record) >= life and all(
                rec["S0"] == _s0_whole(T) and rec["lanes"][lane][1] == t and len(rec["lanes"]) == LANES and
                all(tile[:2] == (T, T) for l, (_, _, tile) in rec["lanes"].items() if l != lane)
                for t, rec in enumerate(record[:life]))
        out.append(_company("whole", "whole/" + c["name"], gact, comp[:lane] + [(c["q"], c["d"])] + comp[lane:], {lane: c["name"]},
                            [(idx + k) % 64 for k in range(LANES)], 4 * (idx % 2), pred))
    return out


def staircase(cases, gact, lives):
    """W = 128.  For tile t of the case, the clean square reads of lengths t (T - O) + 32 k, 32 k <= T: their last tile
    is the wavefront's tile t, with tq = tt = 32 k, so that some stream word of every pass-1 pair and every pass-2 block
    holds a free-exit point -- no pair runs plain and no block on the window, whatever the case's own tile.  The other
    lanes hold whole tiles.  A table covers as many of the case's tiles as it has lanes for; a case of more than
    STAIR_MAX_TILES tiles is left out.  -> (companies, names left out)"""
    T, O, W = gact
    assert W == 128
    steps = [BS_K * k for k in range(1, T // BS_K + 1)]
    per_table = max(1, (LANES - 2) // max(1, len(steps)))
    filler = [clean(whole_len(gact, STAIR_MAX_TILES), "stair-whole", gact, k % 3) for k in range(LANES - 1)]
    out, left = [], []
    for idx, c in enumerate(cases):
        life = lives[c["name"]]
        if life > STAIR_MAX_TILES:
            left.append(c["name"])
            continue
        for first in range(0, life, per_table):
            covers = list(range(first, min(life, first + per_table)))
            comp = [clean(t * (T - O) + s, "stair", gact, t, s) for t in covers for s in steps]
            comp += filler[:LANES - 1 - len(comp)]
            lane = (11 * idx + 5) % LANES

            def pred(tiles, record, covers=covers, lane=lane):
                return all(record[t]["lanes"][lane][1] == t and record[t]["plain"] == 0 and "W" not in record[t]["blocks"]
                           and record[t]["blocks"] for t in covers)
            out.append(_company("staircase", "staircase/%s/%d" % (c["name"], first), gact,
                                comp[:lane] + [(c["q"], c["d"])] + comp[lane:], {lane: c["name"]},
                                [(3 * idx + k) % 64 for k in range(LANES)], 4 * (idx % 2), pred, covers=covers))
    return out, left


def _flag(q, k):
    """q with one byte that is not ACGT: an N or a lower-case base, where k says."""
    q = bytearray(q)
    at = (31 * k) % len(q)
    q[at] = ord("N") if k % 2 else q[at] | 0x20
    return bytes(q)


def _marked(k):
    return k % 9 == 4 or k % 16 == 11


def ragged(cases, gact):
    """The cases of one (T, O, W), 64 to a table, in two fixed shuffles: lanes hold tiles of unequal tq and tt side by
    side.  Every 9th job is flagged (the byte kernel runs it, its lane holds no tile), every 16th of the others fenced;
    the second shuffle puts the cases that were flagged or fenced in the first where they are neither.  The two store
    paths of bs_expand_kernel: store_stride = 0 and 4 mod 16 in turn.  Targets start at every residue mod 64."""
    n = len(cases)
    first = [int(x) for x in _rng("ragged", gact, 0).permutation(n)]
    pos = lambda k: k % LANES                                   # noqa: E731  (the job index in its table decides)
    hit = [c for k, c in enumerate(first) if _marked(pos(k))]
    rest = [c for k, c in enumerate(first) if not _marked(pos(k))]
    rng = _rng("ragged", gact, 1)
    rest = [rest[int(x)] for x in rng.permutation(len(rest))]
    n_marked = sum(_marked(pos(k)) for k in range(n))
    into_marked, others = rest[:n_marked], rest[n_marked:] + hit
    others = [others[int(x)] for x in rng.permutation(len(others))]
    second = [into_marked.pop() if _marked(pos(k)) else others.pop() for k in range(n)]
    out = []
    for shuffle, order in enumerate((first, second)):
        for tb, at in enumerate(range(0, n, LANES)):
            jobs = order[at:at + LANES]
            flagged = [k for k in range(len(jobs)) if k % 9 == 4]
            fenced = [k for k in range(len(jobs)) if k % 16 == 11 and k % 9 != 4]
            pairs = [(_flag(cases[c]["q"], k) if k in flagged else cases[c]["q"], cases[c]["d"]) for k, c in enumerate(jobs)]
            out.append(_company("ragged", "ragged/%d,%d,%d/%d/%d" % (gact + (shuffle, tb)), gact, pairs,
                                {k: cases[c]["name"] for k, c in enumerate(jobs)},
                                [(k + 17 * tb + 29 * shuffle) % 64 for k in range(len(jobs))], 4 * ((tb + shuffle) % 2),
                                flagged=flagged, fenced=fenced))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# gact3_kernel: jobs 2k and 2k + 1 share a wavefront, 16 bits of every register each
# ---------------------------------------------------------------------------------------------------------------------
def pairs(cases, gact, lives):
    """Per partner kind one table: every case as job 2k (low half) beside its partner and as job 2k + 1 (high half)
    beside it.  whole: a clean square read whose tiles are whole while the case lives (the sweep starts far outside a
    small tile); one: a one-base pair (the exit test is on everywhere: s_free < 0); self: a copy of the case (both halves
    carry the same borrows); neighbour: the next case of a fixed shuffle, and the one before it on the other side."""
    T = gact[0]
    n = len(cases)
    big = clean(whole_len(gact, max(lives[c["name"]] for c in cases)), "pair-whole", gact)
    one = (b"C", b"C")
    order = [int(x) for x in _rng("pairs", gact).permutation(n)]
    nxt = {order[k]: order[(k + 1) % n] for k in range(n)}
    prv = {order[k]: order[(k - 1) % n] for k in range(n)}
    out = []
    for kind in PARTNERS:
        jobs, names, partner_of = [], {}, {}
        for idx, c in enumerate(cases):
            me = (c["q"], c["d"])
            lo = {"whole": big, "one": one, "self": me, "neighbour": (cases[nxt[idx]]["q"], cases[nxt[idx]]["d"])}[kind]
            hi = (cases[prv[idx]]["q"], cases[prv[idx]]["d"]) if kind == "neighbour" else lo
            for a, b, mine in ((me, lo, 0), (hi, me, 1)):
                names[len(jobs) + mine] = c["name"]
                partner_of[len(jobs) + mine] = len(jobs) + 1 - mine
                jobs += [a, b]

        def pred(tiles, record, kind=kind, partner_of=partner_of):
            if kind == "whole":
                return all(len(tiles[p]) >= len(tiles[k]) and all(t[:2] == (T, T) for t in tiles[p][:len(tiles[k])])
                           for k, p in partner_of.items())
            if kind == "one":
                return all(tiles[p] == [(1, 1, 0)] for p in partner_of.values())
            return all((k ^ 1) == p for k, p in partner_of.items())
        out.append(_company("pair-" + kind, "pair-%s/%d,%d,%d" % ((kind,) + gact), gact, jobs, names, None, 0, pred, share=True,
                            partner_of=partner_of))
    return out
