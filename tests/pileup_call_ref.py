"""The call rule of the pileup (docs/GACT_SPEC.md, "Pileup calls") in plain Python, one position at a time, Python integers
throughout.  Written from the spec section; it shares nothing with the product."""
import numpy as np

SNV, DEL, INS = 1, 2, 4
DEFAULTS = dict(min_depth=8, min_count=4, min_pct=25)
BASES = "ACGT"
SITE_FIELDS = ("pos", "depth", "n_ref", "n_alt", "n_del", "n_ins", "ref", "alt", "cons", "kinds")


def options(min_depth=0, min_count=0, min_pct=0, reserved=0):
    """-> the three numbers with the defaults in place of zeros; None when the options are refused"""
    if min_pct > 100 or reserved != 0:
        return None
    return (min_depth or DEFAULTS["min_depth"], min_count or DEFAULTS["min_count"], min_pct or DEFAULTS["min_pct"])


def ref_class(byte):
    """0..3 for A/a, C/c, G/g, T/t, 4 for any other byte"""
    return BASES.find(chr(byte).upper()) if chr(byte).upper() in BASES else 4


def call(col, byte, opt):
    """col: (depth, n_eq, x_a, x_c, x_g, x_t, n_del, n_ins) -> (kinds, alt, n_alt, cons), letters as byte values"""
    depth, n_eq, xa, xc, xg, xt, n_del, n_ins = (int(v) for v in col)
    min_depth, min_count, min_pct = opt
    rc = ref_class(byte)
    allele = [x + (n_eq if k == rc else 0) for k, x in enumerate((xa, xc, xg, xt))]
    allele = [a & 0xFFFFFFFF for a in allele]                          # the counters are 32-bit and wrap

    def passes(n):
        return depth >= min_depth and n >= min_count and 100 * n >= min_pct * depth

    kinds = 0
    if any(passes(allele[k]) for k in range(4) if k != rc):
        kinds |= SNV
    if passes(n_del):
        kinds |= DEL
    if passes(n_ins):
        kinds |= INS
    others = [k for k in range(4) if k != rc]
    top = max(allele[k] for k in others)
    alt_k = next(k for k in others if allele[k] == top)                # a tie: the earlier of A, C, G, T
    alt, n_alt = (ord(BASES[alt_k]), top) if top else (ord("."), 0)
    five = allele + [n_del]
    if depth < min_depth or not any(five):
        cons = ord("N")
    else:
        best = max(five)
        order = ([rc] if rc < 4 else []) + [0, 1, 2, 3, 4]             # the reference class first, then A, C, G, T, the deletion
        cons = ord("ACGT-"[next(k for k in order if five[k] == best)])
    return kinds, alt, n_alt, cons


def sites(cols, content, pos0, opt):
    """cols: records with the fields of lrm_pileup_col; content[k]: the text byte of cols[k], at text position pos0 + k
    -> (list of site tuples in the order of SITE_FIELDS, cons bytes)"""
    out, cons = [], bytearray()
    for k in range(len(cols)):
        c = cols[k]
        col = (c["depth"], c["n_eq"], c["x_a"], c["x_c"], c["x_g"], c["x_t"], c["n_del"], c["n_ins"])
        kinds, alt, n_alt, letter = call(col, content[k], opt)
        cons.append(letter)
        if kinds:
            out.append((pos0 + k, int(c["depth"]), int(c["n_eq"]), n_alt, int(c["n_del"]), int(c["n_ins"]), content[k], alt, letter, kinds))
    return out, bytes(cons)


def sites_sparse(cols, content, pos0, opt):
    """sites() for long windows that are mostly empty.  A record whose eight counters are all 0 is no site and its letter is
    'N' under any accepted options: min_count >= 1 fails every count of 0, and all five counts of the consensus are 0.  Only
    the other positions go through call()."""
    cons = np.full(len(cols), ord("N"), dtype=np.uint8)
    live = np.zeros(len(cols), dtype=bool)
    for f in ("depth", "n_eq", "x_a", "x_c", "x_g", "x_t", "n_del", "n_ins"):
        live |= np.asarray(cols[f]) != 0
    out = []
    for k in np.flatnonzero(live):
        got, letter = sites(cols[k:k + 1], content[k:k + 1], pos0 + int(k), opt)
        cons[k] = letter[0]
        out += got
    return out, cons.tobytes()


def as_tuples(records):
    """site records (any array with SITE_FIELDS) -> the list of tuples sites() returns"""
    return [tuple(int(r[f]) for f in SITE_FIELDS) for r in records]


def line(name, pos1, s):
    """the text line of one site tuple of sequence `name`, pos1 its 1-based position in it"""
    _, depth, n_ref, n_alt, n_del, n_ins, ref, alt, cons, kinds = s
    letters = "".join(ch for bit, ch in ((SNV, "S"), (DEL, "D"), (INS, "I")) if kinds & bit)
    return "%s\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name, pos1, chr(ref), chr(alt), letters, depth, n_ref, n_alt, n_del, n_ins, chr(cons))


def cols_array(rows):
    """[(depth, n_eq, x_a, x_c, x_g, x_t, n_del, n_ins)] -> a record array with those fields"""
    out = np.zeros(len(rows), dtype=[(f, "<u4") for f in ("depth", "n_eq", "x_a", "x_c", "x_g", "x_t", "n_del", "n_ins")])
    for k, r in enumerate(rows):
        out[k] = tuple(int(v) & 0xFFFFFFFF for v in r)
    return out
