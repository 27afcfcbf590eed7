"""Python restatement of docs/GACT_SPEC.md, "Split reads": the segment table from the clip counts of a batch, and the SAM
text of a read with supplementary records (lrm_sam_format_split), written from the rule and not from the C code."""
import sam_ref

SEG_RIGHT, SEG_ALIGNED = 1, 2
MIN_DEFAULT = 200


def plan(lens, cl, cr, M=0):
    """-> [(read, start, len, flags)]: reads ascending, left before right; M = 0 is the default."""
    M = M or MIN_DEFAULT
    if not 50 <= M <= 1 << 20:
        raise ValueError("split_min_len outside [50, 2^20]")
    out = []
    for i, n in enumerate(lens):
        n, a, b = int(n), min(int(cl[i]), int(n)), min(int(cr[i]), int(n))
        if a >= M:
            out.append((i, 0, a, 0))
        if b >= M:
            out.append((i, n - b, b, SEG_RIGHT))
    return out


def clip_of_ops(ops: bytes):
    left = len(ops) - len(ops.lstrip(b"S"))
    return left, (len(ops) - len(ops.rstrip(b"S")) if left < len(ops) else 0)


def shape(ops: bytes):
    """aligned query bases, target span, 'S' at the start, 'S' at the end"""
    sl, sr = clip_of_ops(ops)
    core = ops[sl:len(ops) - sr]
    return sum(c in b"=XI" for c in core), sum(c in b"=XD" for c in core), sl, sr


def sa_entry(rname, pos, rev, c5, q, t, c3, ed):
    cg = ("%dS" % c5 if c5 else "") + "%dM" % q + ("%dD" % (t - q) if t > q else "%dI" % (q - t) if q > t else "") + \
         ("%dS" % c3 if c3 else "")
    return "%s,%d,%s,%s,255,%d;" % (rname, pos, "-" if rev else "+", cg, ed)


def records(name, seq, qual, mta, prim, segs):
    """The lines of one read.  prim: dict(ops, score, meta_r, seq_id, off, strand); seq: the read as its primary line prints
    it; qual: as sequenced (None: '*'); segs: the read's segments in table order, dicts (start, len, flags, row, ops, score,
    seq_id, off, strand)."""
    line = sam_ref.record(name, seq, qual, mta, prim["ops"], prim["score"], prim["meta_r"], prim["seq_id"], prim["off"], prim["strand"])
    rep = [g for g in segs if g["flags"] & SEG_ALIGNED]
    if not rep or prim["meta_r"] == 0 or prim["score"] == -1:
        return line
    n, ps = len(seq), prim["strand"]
    pq, pt, psl, psr = shape(prim["ops"])
    p_entry = sa_entry(mta[prim["seq_id"]][0], prim["off"] + 1, ps == 1, psl, pq, pt, psr, prim["score"])
    ent, hard = [], []
    for g in rep:
        a, m, ss = g["start"], g["len"], g["strand"]
        hl, hr = (a, n - a - m) if ss == 0 else (n - a - m, a)
        q, t, sl, sr = shape(g["ops"])
        hard.append((hl, hr))
        ent.append(sa_entry(mta[g["seq_id"]][0], g["off"] + 1, ps != ss, hl + sl, q, t, sr + hr, g["score"]))
    out = line[:-1] + "\tSA:Z:" + "".join(ent) + "\n"
    for k, g in enumerate(rep):
        a, m, ss = g["start"], g["len"], g["strand"]
        rev = ps != ss
        hl, hr = hard[k]
        cigar = ("%dH" % hl if hl else "") + sam_ref.rle(g["ops"]) + ("%dH" % hr if hr else "")
        if qual is None:
            ql = "*"
        else:
            q0 = n - a - m if ps == 1 else a
            ql = qual[q0:q0 + m][::-1] if rev else qual[q0:q0 + m]
        others = "".join(e for j, e in enumerate(ent) if j != k)
        out += "%s\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t%s\tED:I:%d\tSA:Z:%s%s\n" % (
            name, 2048 + (16 if rev else 0), mta[g["seq_id"]][0], g["off"] + 1, cigar, g["row"], ql, g["score"], p_entry, others)
    return out
