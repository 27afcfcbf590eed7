"""docs/GACT_SPEC.md, "End clipping", executable, on top of tests/anchored_ref.py (which stays the reference of the mode
without the step):

    clip_job(ops, P, B)          -> keep: the columns of ONE job's op bytes (extension order: column 0 touches the anchor)
                                    that stay aligned
    extend_clipped(read, ...)    -> the dict of anchored_ref.extend with the step applied, plus clip_left, clip_right
    extend_clipped_batch(...)    -> the same over a batch, like anchored_ref.extend_batch

Written from the spec text; clip_job is quadratic on purpose (every prefix score is summed from scratch)."""
import anchored_ref

P_DEFAULT, B_DEFAULT = 2, 6
SOFT_LEFT, SOFT_RIGHT = 32, 64


def prefix_score(ops, k, P):
    """s[k]: '=' +1, every other column -P, over ops[0 .. k)."""
    return sum(1 if c == ord("=") else -P for c in ops[:k])


def clip_job(ops, P=0, B=0):
    P, B = P or P_DEFAULT, B or B_DEFAULT
    m = len(ops)
    if m > 400:                                   # same definition, the scores carried along instead of summed again
        s, scores = 0, [0]
        for c in ops:
            s += 1 if c == ord("=") else -P
            scores.append(s)
    else:
        scores = [prefix_score(ops, k, P) for k in range(m + 1)]
    best = max(scores)
    k_star = scores.index(best)                   # the SMALLEST k with s[k] == best
    return k_star if best - scores[m] > B else m


def apply_clip(e, n, P=0, B=0):
    """The step on the result `e` of anchored_ref.extend for a read of n bases."""
    e = dict(e, clip_left=0, clip_right=0)
    if not e["flags"] & anchored_ref.ANCHORED:    # unanchored: left exactly as the mode leaves it
        return e
    j, p = e["read_pos"], e["text_pos"]
    left = e["ops"][:e["left_ops"]][::-1]         # both in extension order: outward from the anchor
    right = e["ops"][e["left_ops"]:]
    kl, kr = clip_job(left, P, B), clip_job(right, P, B)
    left, right = left[:kl], right[:kr]
    cl = j - (len(left) - left.count(b"D"))
    cr = (n - j) - (len(right) - right.count(b"D"))
    ops = b"S" * cl + left[::-1] + right + b"S" * cr
    first = p - (len(left) - left.count(b"I"))
    S = e["loc"] - e["off"]
    flags = e["flags"] | (SOFT_LEFT if cl else 0) | (SOFT_RIGHT if cr else 0)
    score = sum(len(x) - x.count(b"=") for x in (left, right))
    return dict(e, ops=ops, n_ops=len(ops), score=score, loc=first, off=first - S, left_ops=cl + kl, flags=flags,
                clip_left=cl, clip_right=cr)


def extend_clipped(read, text, L, S, len_s, gact=(320, 120, 128), min_len=0, aligner=None, P=0, B=0):
    return apply_clip(anchored_ref.extend(read, text, L, S, len_s, gact, min_len, aligner), len(read), P, B)


def extend_clipped_batch(text, mta, reads, lens, meta, meta_r, gact=(320, 120, 128), min_len=0, aligner=None, P=0, B=0):
    base = anchored_ref.extend_batch(text, mta, reads, lens, meta, meta_r, gact, min_len, aligner)
    return [None if e is None else apply_clip(e, int(lens[i]), P, B) for i, e in enumerate(base)]


def aligned_part(e):
    """The op bytes between the two runs of 'S'."""
    return e["ops"][e["clip_left"]:e["n_ops"] - e["clip_right"]]
