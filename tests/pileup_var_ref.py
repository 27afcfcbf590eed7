"""The variant rule of the pileup (docs/GACT_SPEC.md, "Pileup variants and VCF") in plain Python over the references of the
call rule (tests/pileup_call_ref.py) and of the inserted allele (tests/pileup_ins_ref.py): the kinds of every position first,
then the runs of deleted positions as a walk over that list.  Written from the spec section; it shares nothing with the product."""
import pileup_call_ref as R
import pileup_ins_ref as IR
from pileup_ref import COL_FIELDS

SNV, DEL, INS = R.SNV, R.DEL, R.INS
HOM_PCT_DEFAULT = 70
FIELDS = ("pos", "len", "depth", "n_ref", "n_alt", "n_col0", "kind", "ref", "alt", "gt", "bases", "ins_flags")


def options(min_depth=0, min_count=0, min_pct=0, reserved=0, hom_pct=0, reserved3=(0, 0, 0)):
    """-> (the call options, hom_pct) with the defaults in place of zeros; None when the options are refused"""
    call = R.options(min_depth, min_count, min_pct, reserved)
    if call is None or hom_pct > 100 or any(reserved3):
        return None
    return call, hom_pct or HOM_PCT_DEFAULT


def gt(hom_pct, n_alt, depth):
    return 2 if 100 * n_alt >= hom_pct * depth else 1


def variants(cols, words, content, pos0, opt):
    """cols: records with the fields of lrm_pileup_col, one per position of the range; words: (count, K, 4) insertion words or
    None for a plain accumulator; content[k]: the text byte of position k, text position pos0 + k
    -> the list of records as tuples in the order of FIELDS (bases: bytes of length len for INS, b"" otherwise)"""
    call_opt, hom = opt
    n = len(cols)
    col = [tuple(int(cols[g][f]) for f in COL_FIELDS) for g in range(n)]
    called = [R.call(col[g], content[g], call_opt) for g in range(n)]
    deleted = [bool(c[0] & DEL) for c in called]
    out = []
    for g in range(n):
        depth, n_eq, _, _, _, _, n_del, n_ins = col[g]
        kinds, alt, n_alt, _ = called[g]
        if deleted[g] and (g == 0 or not deleted[g - 1]):
            end = g
            while end < n and deleted[end]:
                end += 1
            out.append((pos0 + g, end - g, depth, n_eq, n_del, 0, DEL, content[g], 0, gt(hom, n_del, depth), b"", 0))
        if kinds & SNV:
            out.append((pos0 + g, 1, depth, n_eq, n_alt, 0, SNV, content[g], alt, gt(hom, n_alt, depth), b"", 0))
        if kinds & INS:
            n_col0, ln, flags, bases = (0, 0, 0, b"")
            if words is not None and words.shape[1]:
                n_col0, ln, flags, bases = IR.allele(depth, n_ins, words[g], call_opt)
            out.append((pos0 + g, ln, depth, n_eq, n_ins, n_col0, INS, content[g], 0, gt(hom, n_ins, depth), bases, flags))
    return out


def as_tuples(records):
    """PILEUP_VARIANT_DT records -> the tuples variants() returns, after checking the zero padding"""
    out = []
    for r in records:
        ln = int(r["len"]) if int(r["kind"]) == INS else 0
        assert not r["pad"].any() and not r["bases"][ln:].any(), r
        out.append(tuple(int(r[f]) for f in FIELDS[:10]) + (bytes(r["bases"][:ln]), int(r["ins_flags"])))
    return out


def upper(b):
    return chr(b).upper()


def vcf_line(name, off, seq_len, seq_text, rec):
    """the VCF line of one record tuple of sequence `name`: off its 0-based position in the sequence, seq_text the
    sequence's text bytes"""
    _, ln, depth, n_ref, n_alt, _, kind, ref, alt, g, bases, flags = rec
    info = "DP=%d" % depth
    if kind == SNV:
        pos1, r, a = off + 1, upper(ref), chr(alt)
    elif kind == DEL and off > 0:
        pos1, r, a = off, "".join(upper(b) for b in seq_text[off - 1:off + ln]), upper(seq_text[off - 1])
    elif kind == DEL:
        pos1, r, a = 1, "".join(upper(b) for b in seq_text[0:ln + 1]), upper(seq_text[ln])
    else:
        pos1, r = off + 1, upper(ref)
        a = r + bases.decode() if ln else "<INS>"
        if flags & IR.FULL:
            info += ";INSFULL"
    return "%s\t%d\t.\t%s\t%s\t.\t.\t%s\tGT:AD\t%s:%d,%d\n" % (name, pos1, r, a, info, "1/1" if g == 2 else "0/1", n_ref, n_alt)
