"""docs/GACT_SPEC.md, "Alignment summary and PAF", executable: the lrm_aln_summary record of one alignment's op bytes and the
PAF line of one read.  Written from the spec text; the tests compare the library against this file, never against itself.

    summary(ops)            -> dict of the eight fields (all zeros for an empty row)
    record(ops, score, meta_r) -> the same with the rule for a read without an alignment
    paf_line(...)           -> the line of one read, "" for an unmapped one"""
import sam_ref

FIELDS = ("n_eq", "n_x", "n_ins", "n_del", "ins_runs", "del_runs", "clip_left", "clip_right")
ZERO = dict.fromkeys(FIELDS, 0)


def summary(ops: bytes):
    ops = bytes(ops)
    if not ops:
        return dict(ZERO)
    runs = lambda c: sum(1 for i in range(len(ops)) if ops[i] == c and (i == 0 or ops[i - 1] != c))
    other = [i for i, o in enumerate(ops) if o != ord("S")]          # a byte outside "=XIDS" is a column that is not 'S'
    return dict(n_eq=ops.count(b"="), n_x=ops.count(b"X"), n_ins=ops.count(b"I"), n_del=ops.count(b"D"),
                ins_runs=runs(ord("I")), del_runs=runs(ord("D")),
                clip_left=other[0] if other else len(ops), clip_right=len(ops) - 1 - other[-1] if other else 0)


def record(ops, score, meta_r):
    """What the device stage writes for a read: zeros without an alignment (no ops, no locus, score -1)."""
    return dict(ZERO) if (len(ops) == 0 or meta_r == 0 or score == -1) else summary(ops)


def nm(s):
    return s["n_x"] + s["n_ins"] + s["n_del"]


def target_span(s):
    return s["n_eq"] + s["n_x"] + s["n_del"]


def block_len(s):
    return s["n_eq"] + s["n_x"] + s["n_ins"] + s["n_del"]


def paf_line(name, qlen, strand, tname, tlen, off, ops, score, meta_r, mq=None, s=None):
    """mq: (mapq, n1, n2) or None.  s: the record to print (None: summary(ops))."""
    if meta_r == 0 or score == -1:
        return ""
    s = summary(ops) if s is None else s
    cl, cr = s["clip_left"], s["clip_right"]
    qs, qe = (cr, qlen - cl) if strand == 1 else (cl, qlen - cr)
    ev = s["n_x"] + s["ins_runs"] + s["del_runs"]
    den = ev + s["n_eq"]
    cols = [name, qlen, qs, qe, "-" if strand == 1 else "+", tname, tlen, off, off + target_span(s), s["n_eq"], block_len(s),
            mq[0] if mq is not None else 255, "NM:i:%d" % nm(s), "ED:i:%d" % score, "tp:A:P",
            "de:f:%.4f" % (ev / den if den else 0.0), "cg:Z:" + sam_ref.rle(ops)]
    if mq is not None:
        cols += ["v1:i:%d" % mq[1], "v2:i:%d" % mq[2]]
    return "\t".join(str(c) for c in cols) + "\n"
