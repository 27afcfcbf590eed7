"""docs/GACT_SPEC.md, "Anchored extension", executable: brute-force anchor (numpy, byte compares), the two jobs through an
`orc_gact`-spec aligner (tests/orc.py: gact, or tests/gact_ref.py: align), and the stitch.

    find_anchor(read, text, L, S, len_s, min_len)      -> (r, delta, j) or None
    extend(read, text, L, S, len_s, gact, min_len, ...) -> dict(ops, n_ops, score, loc, off, anchor fields ...)
    extend_batch(text, mta, reads, lens, meta, meta_r, ...) the same over the outputs of the classic path's locus_resolve

`read` is oriented like the forward strand, `L` is the voted window start inside the sequence [S, S + len_s) whose
reverse complement occupies [S + len_s, S + 2 len_s) of `text`."""
import numpy as np

DIAGS = 64
MIN_DEFAULT = 20
ANCHORED, FALLBACK, NO_LEFT, LEFT_CLIPPED, RIGHT_CLIPPED = 1, 2, 4, 8, 16
_ACGT = np.zeros(256, dtype=bool)
_ACGT[[65, 67, 71, 84]] = True
_COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b


def revcomp(a):
    return _COMP[np.asarray(a, dtype=np.uint8)[::-1]]


def find_anchor(read, text, L, S, len_s, min_len=0):
    """The longest maximal run read[j .. j+r) == text[L+delta+j ...) of ACGT bytes inside the sequence, r >= min_len,
    over delta in [-32, 32); ties: smallest |delta|, then smallest delta, then smallest j."""
    A = min_len or MIN_DEFAULT
    read = np.asarray(read, dtype=np.uint8)
    text = np.asarray(text, dtype=np.uint8)
    n, half = len(read), DIAGS // 2
    if n == 0:
        return None
    pos = L - half + np.arange(n + DIAGS - 1, dtype=np.int64)          # text positions of the diagonals' windows
    inside = (pos >= S) & (pos < S + len_s)
    win = np.where(inside, text[np.clip(pos, 0, len(text) - 1)], 0).astype(np.uint8)
    rows = np.lib.stride_tricks.sliding_window_view(win, n)              # row d: delta = d - 32
    eq = (rows == read[None, :]) & _ACGT[read][None, :]
    edge = np.diff(np.pad(eq, ((0, 0), (1, 1))).astype(np.int8), axis=1)
    starts, ends = np.argwhere(edge == 1), np.argwhere(edge == -1)       # row-major: the k-th start pairs the k-th end
    runs = ends[:, 1] - starts[:, 1]
    best = None
    for k in np.flatnonzero(runs >= A):
        delta, j, r = int(starts[k, 0]) - half, int(starts[k, 1]), int(runs[k])
        key = (r, -abs(delta), -delta, -j)
        if best is None or key > best[0]:
            best = (key, (r, delta, j))
    return best[1] if best else None


def plan(anchor, L, n, S, len_s):
    """The two jobs of an anchored read: (p, right target length, left target start, left target length, flags)."""
    r, delta, j = anchor
    p = L + delta + j
    nr, flags = n - j, ANCHORED
    wr = nr + (nr + 7) // 8
    tr = min(wr, S + len_s - p)
    flags |= RIGHT_CLIPPED if wr > S + len_s - p else 0
    if j == 0:
        return p, tr, 0, 0, flags | NO_LEFT
    wl = j + (j + 7) // 8
    tl = min(wl, p - S)
    flags |= LEFT_CLIPPED if wl > p - S else 0
    return p, tr, 2 * S + 2 * len_s - p, tl, flags


def extend(read, text, L, S, len_s, gact=(320, 120, 128), min_len=0, aligner=None):
    """aligner(q: bytes, d: bytes, T, O, W) -> (score, ops: bytes, ...)."""
    if aligner is None:
        import orc
        aligner = orc.gact
    read = np.asarray(read, dtype=np.uint8)
    text = np.asarray(text, dtype=np.uint8)
    n = len(read)
    a = find_anchor(read, text, L, S, len_s, min_len)
    if a is None:                                                         # extended exactly as without the mode
        score, ops = aligner(bytes(read), bytes(text[L:L + n]), *gact)[:2]
        return dict(ops=ops, n_ops=len(ops), score=score, loc=L, off=L - S, text_pos=L, read_pos=0, len=0, delta=0,
                    left_ops=0, flags=FALLBACK)
    r, delta, j = a
    p, tr, yl, tl, flags = plan(a, L, n, S, len_s)
    sr, ops_r = aligner(bytes(read[j:]), bytes(text[p:p + tr]), *gact)[:2]
    sl, ops_l = (0, b"")
    if j > 0:
        sl, ops_l = aligner(bytes(revcomp(read[:j])), bytes(text[yl:yl + tl]), *gact)[:2]
    ops = ops_l[::-1] + ops_r
    first = p - (len(ops_l) - ops_l.count(b"I"))
    return dict(ops=ops, n_ops=len(ops), score=sl + sr, loc=first, off=first - S, text_pos=p, read_pos=j, len=r,
                delta=delta, left_ops=len(ops_l), flags=flags)


def extend_batch(text, mta, reads, lens, meta, meta_r, gact=(320, 120, 128), min_len=0, aligner=None):
    """One dict per read (None for meta_r == 0) from the oriented reads and the meta the classic path resolved."""
    out = []
    for i in range(len(lens)):
        if not meta_r[i]:
            out.append(None)
            continue
        S, len_s = mta[int(meta["seq_id"][i])]
        out.append(extend(reads[i, :int(lens[i])], text, int(meta["loc"][i]), int(S), int(len_s), gact, min_len, aligner))
    return out


def query_bases(ops):
    return len(ops) - ops.count(b"D")


def edge_indel_runs(ops):
    """Longest run of 'I' or 'D' columns touching either end of the ops."""
    def lead(o):
        k = 0
        while k < len(o) and o[k] in b"ID" and o[k] == o[0]:
            k += 1
        return k
    return max(lead(ops), lead(ops[::-1]))
