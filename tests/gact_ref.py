"""docs/GACT_SPEC.md, executable: the second, independent form of the tiled extension.

Written from the specification's text alone (sections "Inputs, outputs", "Algorithm", "Tile DP"); it imports nothing
from oracle/, tests/orc.py, tests/models/ or the product.  SCORE form: every tile's full R[a][b] as integers with an
explicit minus infinity outside the band, filled one anti-diagonal at a time with numpy, the band a mask on b - a.
No decision is stored: the walk recomputes the three candidate scores at every point it visits and takes the first
maximum in the tie order.  (The oracle goes row by row and stores a predecessor per cell; the kernels and the CPU model
use the difference form.  Two programs that reach the same ops by different routes are the point.)

    align(q, d, T, O, W) -> (score, ops, trace)
    align_many([(q, d), ...], T, O, W) -> [(score, ops, trace), ...]      the same, tiles of equal shape filled together

trace: one dict per tile --
    i, j        anchor: read / text bases consumed before the tile
    tq, tt      tile extent,  last: the tile contains the read's end
    stop        (a, b) where the walk stopped,  rule: frozenset of the stop rules that hold there:
                  "read"   a == tq            "text"  b == tt
                  "keep"   non-final tile, a == T-O or b == T-O
                  "cap"    final tile, a + b == 2(T-O)
    dmin, dmax  smallest / largest b - a on the walk (stop point included)
    V, H        values R[a][b] - R[a+1][b] / R[a][b] - R[a][b+1] took at the walk's points (where both are in the band)
    ties        which candidates held the maximum at the walk's points: subsets of "DIL" (DIAG, INS, DEL) as strings,
                e.g. "D" DIAG alone, "IL" INS and DEL tied above DIAG, "DIL" the three-way tie
    anti        the anti-diagonal a + b of every indel column of the walk (tile-relative, before the move)
trace.tail: length of the trailing 'I' run (text exhausted).

The keyword arguments are the three mistakes the negative controls make on purpose; the defaults are the spec.
Nothing is cached between calls.
"""
import numpy as np

NEG = -(1 << 28)                 # minus infinity: no sum of tile scores comes near it
_CELLS = 1 << 22                # tiles filled together: at most this many lattice points


class Trace(list):
    tail = 0

    def union(self, key):
        out = set()
        for t in self:
            out |= t[key]
        return out


def valid(T, O, W):
    return 0 <= O < T and W >= 2 and W % 2 == 0


def _tiles(Q, D, W, symmetric):
    """R of P tiles of one shape at once, P x (tq + 2) x (tt + 2): row tq / column tt are the free exit, one more row and
    column of minus infinity so that every neighbour of a lattice point exists."""
    (P, tq), tt = Q.shape, D.shape[1]
    a = np.arange(tq + 2, dtype=np.int32)[:, None]
    b = np.arange(tt + 2, dtype=np.int32)[None, :]
    diag = b - a
    band = (diag >= -(W // 2)) & ((diag <= W // 2) if symmetric else (diag < W // 2)) & (a <= tq) & (b <= tt)
    R = np.full((P, tq + 2, tt + 2), NEG, dtype=np.int32)
    R[:, tq, :tt + 1] = 0
    R[:, :tq + 1, tt] = 0
    R[:, ~band] = NEG                                            # a boundary point outside the band is outside the band
    S = np.full((P, tq + 2, tt + 2), -1, dtype=np.int32)
    S[:, :tq, :tt][Q[:, :, None] == D[:, None, :]] = 1
    # anti-diagonal k of a row-major (tq + 2) x (tt + 2) array: flat index a * (tt + 2) + (k - a) = k + a * (tt + 1)
    Rf, Sf, Bf = R.reshape(P, -1), S.reshape(P, -1), band.reshape(-1)
    step, row = tt + 1, tt + 2
    for k in range(tq + tt - 2, -1, -1):
        lo, hi = max(0, k - (tt - 1)), min(tq - 1, k)          # interior points a < tq, b = k - a < tt
        s0, s1 = k + lo * step, k + hi * step + 1
        dg = Rf[:, s0 + row + 1:s1 + row + 1:step] + Sf[:, s0:s1:step]
        ins = Rf[:, s0 + row:s1 + row:step] - 1
        dl = Rf[:, s0 + 1:s1 + 1:step] - 1
        Rf[:, s0:s1:step] = np.where(Bf[s0:s1:step], np.maximum(np.maximum(dg, ins), dl), NEG)
    return R


def _walk(R, q, d, rec, keep, tie_order, keep_inclusive, ops):
    """From (0, 0) while the spec's conditions hold; the decision at every point from the three candidate scores."""
    tq, tt, last = rec["tq"], rec["tt"], rec["last"]
    at = R.item
    a = b = 0
    while a < tq and b < tt and ((a + b < 2 * keep) if last else
                                 ((a <= keep and b <= keep) if keep_inclusive else (a < keep and b < keep))):
        match = q[a] == d[b]
        here, down, right = at(a, b), at(a + 1, b), at(a, b + 1)
        cand = {"D": at(a + 1, b + 1) + (1 if match else -1), "I": down - 1, "L": right - 1}
        best = max(cand.values())
        assert best == here and best > NEG // 2, "the walk left the band"
        rec["ties"].add("".join(c for c in "DIL" if cand[c] == best))
        if down > NEG // 2:
            rec["V"].add(here - down)
        if right > NEG // 2:
            rec["H"].add(here - right)
        move = next(c for c in tie_order if cand[c] == best)
        if move == "D":
            ops.append(61 if match else 88)                     # '=' / 'X'
            a, b = a + 1, b + 1
        else:
            rec["anti"].append(a + b)
            ops.append(73 if move == "I" else 68)               # 'I' / 'D'
            a, b = (a + 1, b) if move == "I" else (a, b + 1)
        rec["dmin"], rec["dmax"] = min(rec["dmin"], b - a), max(rec["dmax"], b - a)
    rule = set()
    if a == tq:
        rule.add("read")
    if b == tt:
        rule.add("text")
    if last and a + b >= 2 * keep:
        rule.add("cap")
    if not last and (a >= keep or b >= keep):
        rule.add("keep")
    rec["stop"], rec["rule"] = (a, b), frozenset(rule)
    assert a + b > 0, "every walk makes at least one move"
    return a, b


def _chunks(shapes):
    for (tq, tt), group in shapes.items():
        per = max(1, _CELLS // ((tq + 2) * (tt + 2)))
        for k in range(0, len(group), per):
            yield (tq, tt), group[k:k + per]


def align_many(pairs, T=320, O=120, W=128, tie_order="DIL", symmetric_band=False, keep_inclusive=False):
    """align() of every (q, d) of `pairs`: in each round the tiles of equal shape are filled together."""
    if not valid(T, O, W):
        return [(-1, b"", Trace()) for _ in pairs]
    keep = T - O
    qs = [np.frombuffer(bytes(q), dtype=np.uint8) for q, _ in pairs]
    ds = [np.frombuffer(bytes(d), dtype=np.uint8) for _, d in pairs]
    state = [[0, 0, bytearray(), Trace()] for _ in pairs]       # i, j, ops, trace
    active = [p for p in range(len(pairs)) if len(qs[p]) and len(ds[p])]
    while active:
        shapes = {}
        for p in active:
            i, j = state[p][:2]
            shapes.setdefault((min(T, len(qs[p]) - i), min(T, len(ds[p]) - j)), []).append(p)
        for (tq, tt), group in _chunks(shapes):
            Q = np.stack([qs[p][state[p][0]:state[p][0] + tq] for p in group])
            D = np.stack([ds[p][state[p][1]:state[p][1] + tt] for p in group])
            R = _tiles(Q, D, W, symmetric_band)
            for g, p in enumerate(group):
                i, j, ops, trace = state[p]
                rec = dict(i=i, j=j, tq=tq, tt=tt, last=i + tq == len(qs[p]), dmin=0, dmax=0, V=set(), H=set(),
                           ties=set(), anti=[])
                a, b = _walk(R[g], Q[g].tolist(), D[g].tolist(), rec, keep, tie_order, keep_inclusive, ops)
                trace.append(rec)
                state[p][0], state[p][1] = i + a, j + b
        active = [p for p in active if state[p][0] < len(qs[p]) and state[p][1] < len(ds[p])]
    out = []
    for p, (i, j, ops, trace) in enumerate(state):
        trace.tail = len(qs[p]) - i
        ops += b"I" * trace.tail
        out.append((len(ops) - ops.count(61), bytes(ops), trace))
    return out


def align(q, d, T=320, O=120, W=128, **rules):
    return align_many([(q, d)], T, O, W, **rules)[0]
