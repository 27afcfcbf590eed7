"""Reference for the difference events and MD:Z (docs/GACT_SPEC.md, "Difference events and MD:Z"): a plain walk over the
columns of one alignment.  md() prints MD the way `samtools calmd` does, straight from ops, text and locus -- it never looks
at events; events() lists the event words separately.  Nothing here is shared with the product."""

KIND_X, KIND_D_OPEN, KIND_D_MORE = 0, 1, 2


def aligned(ops, score=0, meta_r=1):
    return len(ops) > 0 and meta_r != 0 and score != -1


def _base(content, pos):
    return content[pos] if 0 <= pos < len(content) else 0


def md(ops, content, loc, score=0, meta_r=1):
    """MD:Z text, or None for a read without an alignment.  A base behind the end of the text prints as chr(0)."""
    if not aligned(ops, score, meta_r):
        return None
    out, run, t, in_del = [], 0, loc, False
    for o in ops:
        c = chr(o)
        if c == "=":
            run += 1
            t += 1
            in_del = False
        elif c == "X":
            out.append("%d%s" % (run, chr(_base(content, t))))
            run = 0
            t += 1
            in_del = False
        elif c == "D":
            if not in_del:
                out.append("%d^" % run)
                run = 0
            out.append(chr(_base(content, t)))
            t += 1
            in_del = True
        else:                          # 'I', 'S', a foreign byte: no target base, and a deletion run ends here
            in_del = False
    out.append("%d" % run)
    return "".join(out)


def events(ops, content, loc, score=0, meta_r=1):
    """The event words of one read, in column order."""
    if not aligned(ops, score, meta_r):
        return []
    out, t, e = [], 0, 0
    for i, o in enumerate(ops):
        c = chr(o)
        if c == "=":
            t += 1
            e += 1
        elif c == "X":
            out.append(_base(content, loc + t) | (KIND_X << 8) | (e << 10))
            t += 1
        elif c == "D":
            kind = KIND_D_OPEN if i == 0 or ops[i - 1] != ord("D") else KIND_D_MORE
            out.append(_base(content, loc + t) | (kind << 8) | (e << 10))
            t += 1
    return out


def nm(ops):
    return sum(ops.count(c) for c in b"XID")


def n_eq(ops):
    return ops.count(b"=")


def m_cigar(ops):
    """[(run, op)] with '=' and 'X' merged to M, as the run-length text prints them."""
    runs = []
    for o in ops:
        c = "M" if chr(o) in "=X" else chr(o)
        if runs and runs[-1][1] == c:
            runs[-1][0] += 1
        else:
            runs.append([1, c])
    return [(k, c) for k, c in runs]


def target_from_md(read, cigar, md_text):
    """Rebuild the target span from the read (as aligned), its M CIGAR [(run, op)] and the MD text."""
    # MD -> per target position: None (= the read's base) or the reference base
    tgt, i = [], 0
    while i < len(md_text):
        ch = md_text[i]
        if ch.isdigit():
            j = i
            while j < len(md_text) and md_text[j].isdigit():
                j += 1
            tgt += [None] * int(md_text[i:j])
            i = j
        elif ch == "^":
            i += 1
            while i < len(md_text) and not md_text[i].isdigit():
                tgt.append(("D", md_text[i]))
                i += 1
        else:
            tgt.append(("X", ch))
            i += 1
    out, q, t = [], 0, 0
    for run, op in cigar:
        if op == "M":
            for _ in range(run):
                item = tgt[t]
                assert item is None or item[0] == "X", (t, item)
                out.append(read[q] if item is None else ord(item[1]))
                q += 1
                t += 1
        elif op == "D":
            for _ in range(run):
                assert tgt[t][0] == "D", (t, tgt[t])
                out.append(ord(tgt[t][1]))
                t += 1
        elif op in "IS":
            q += run
        else:
            raise AssertionError(op)
    assert t == len(tgt) and q == len(read), (t, len(tgt), q, len(read))
    return bytes(out)


def mutate(rng, text, loc, span):
    """A random alignment of a read made from text[loc:loc + span): -> (read bytes, op bytes).  Every column kind occurs;
    an 'X' column's read base differs from the text's."""
    bases = b"ACGT"
    read, ops, t = bytearray(), bytearray(), loc
    end = loc + span
    for _ in range(int(rng.integers(0, 4))):
        read.append(bases[int(rng.integers(0, 4))])
        ops.append(ord("S"))
    while t < end:
        r = rng.random()
        if r < 0.80:
            read.append(text[t]); ops.append(ord("=")); t += 1
        elif r < 0.88:
            alt = [b for b in bases if b != text[t]]
            read.append(alt[int(rng.integers(0, len(alt)))]); ops.append(ord("X")); t += 1
        elif r < 0.94:
            k = min(int(rng.integers(1, 4)), end - t)
            ops += b"D" * k; t += k
        else:
            k = int(rng.integers(1, 4))
            for _ in range(k):
                read.append(bases[int(rng.integers(0, 4))])
            ops += b"I" * k
    for _ in range(int(rng.integers(0, 4))):
        read.append(bases[int(rng.integers(0, 4))])
        ops.append(ord("S"))
    return bytes(read), bytes(ops)
