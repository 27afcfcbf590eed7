"""The host text stage either side of the hot path (include/lrm_io_host.h): the FASTA / FASTQ batch reader, the SAM and
PAF formatters and the whole-file flows (lrm_accaln*).  Record arrays are numpy arrays of the records.py dtypes."""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import lib


class Reader:
    """lrm_reader: `with Reader(path) as rd: n = rd.next(1000)`; rd.batch is the lrm_read_batch of the last next() that
    returned reads.  It is freed by the following next(), by free() and on the way out."""

    def __init__(self, path):
        self.handle, self.batch = C.c_void_p(), None
        capi.check(lib.lrm_reader_open(C.byref(self.handle), os.fsencode(path)), "lrm_reader_open")

    def next(self, n, into=None, into_bytes=None):
        """Up to n reads -> their number (0: end of file; < 0: the parser's code, text in lrm_last_error).  into: a uint8
        array that takes the sequences when they fit its into_bytes (default: all of it) -- lrm_reader_next_into."""
        self.free()
        b = capi.ReadBatch()
        if into is None:
            got = lib.lrm_reader_next(self.handle, n, C.byref(b))
        else:
            got = lib.lrm_reader_next_into(self.handle, n, C.byref(b), into.ctypes.data, into.nbytes if into_bytes is None else into_bytes)
        if got > 0:
            self.batch = b
        return got

    def free(self):
        if self.batch is not None:
            lib.lrm_read_batch_free(C.byref(self.batch))
            self.batch = None

    def close(self):
        self.free()
        if self.handle:
            lib.lrm_reader_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def mta_table(entries):
    """lrm_mta_entry array of (name, offset, seq_len) tuples; the array keeps the names alive."""
    mta = (capi.MtaEntry * len(entries))()
    for m, (name, offset, seq_len) in zip(mta, entries):
        name = name.encode() if isinstance(name, str) else name
        m.name_len, m.name, m.offset, m.seq_len = len(name), name, offset, seq_len
    return mta


def cigar_table(addr, n_ops, score):
    """lrm_cigar records (CIGAR_DT, at least one) of alignments whose bytes start at the addresses `addr`."""
    cig = np.zeros(max(len(addr), 1), dtype=capi.CIGAR_DT)
    k = len(addr)
    cig["cigar"][:k], cig["n_cigar_op"][:k], cig["score"][:k] = addr, n_ops, score
    return cig


def cigar_array(ops_list, scores, texts=None):
    """lrm_cigar records of alignments given as op byte strings.  texts: the run-length CIGAR text of each, which the
    records then point to (the cigar_text layout: n_cigar_op stays the number of columns).  -> (records, the buffer they
    point into, which the caller keeps for as long as the records are in use)."""
    rows = [bytes(r) + b"\0" for r in (ops_list if texts is None else texts)]
    blob = np.frombuffer(b"".join(rows) + b"\0", dtype=np.uint8)
    starts = np.cumsum([0] + [len(r) for r in rows[:-1]], dtype=np.uint64)[:len(rows)]
    return cigar_table(starts + np.uint64(blob.ctypes.data), [len(o) for o in ops_list], scores), blob


def _text(entry, *args):
    """What a formatter returned as str (None where it refused: lrm_last_error)."""
    length = C.c_uint64()
    p = entry(*args, C.byref(length))
    if not p:
        return None
    try:
        return C.string_at(p, length.value).decode()
    finally:
        lib.lrm_free(p)


def _at(a):
    return None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else C.byref(a)


def sam_header(mta, rg_id):
    return _text(lib.lrm_sam_header, mta, len(mta), rg_id)


def md_text(events, n_eq):
    """lrm_md_format: the MD:Z text of one read from its difference events (uint32 words) and the n_eq of its summary record."""
    ev = np.ascontiguousarray(events, dtype=np.uint32)
    buf = C.create_string_buffer(12 * len(ev) + 24)
    k = lib.lrm_md_format(ev.ctypes.data if len(ev) else None, len(ev), int(n_eq), buf, len(buf))
    assert k >= 0
    return buf.raw[:k].decode()


def sam_format(batch, mta, cig, score, meta, meta_r, n, *, is_text=0, keep=0, split=None, mapq=None, entry=None, md=None,
               secondary=None):
    """secondary: an lrm_secondary_out (or entry == "lrm_sam_format_secondary", then None stands for NULL) --
    lrm_sam_format_secondary: a FLAG 256 line behind the lines of every read with a reported secondary.
    md: (summary records, offsets, counts, events) of the batch, or a map_batch(md=True) result with summary=True --
    lrm_sam_format_md: NM:i and MD:Z behind ED:I (None for events: the lines of lrm_sam_format_mapq).
    The SAM records of a batch: lrm_sam_format_mapq with mapq (MAPQ_DT records), lrm_sam_format_split with split (an
    lrm_split_out), run-length text (is_text) or untouched reads (keep), else lrm_sam_format; entry names one of the three
    instead (the later ones take NULL for what the earlier ones lack)."""
    if secondary is not None or entry == "lrm_sam_format_secondary":
        if isinstance(md, dict):
            md = (md["summary"], md["md_off"], md["md_cnt"], md["md_events"])
        md = (None,) * 4 if md is None else md
        return _text(lib.lrm_sam_format_secondary, C.byref(batch), mta, len(mta), _at(cig), _at(score), _at(meta), _at(meta_r), n,
                     int(is_text), int(keep), _at(split), _at(mapq), *(_at(x) for x in md), _at(secondary))
    if md is not None or entry == "lrm_sam_format_md":
        if isinstance(md, dict):
            md = (md["summary"], md["md_off"], md["md_cnt"], md["md_events"])
        md = (None,) * 4 if md is None else md
        return _text(lib.lrm_sam_format_md, C.byref(batch), mta, len(mta), _at(cig), _at(score), _at(meta), _at(meta_r), n, int(is_text),
                     int(keep), _at(split), _at(mapq), *(_at(x) for x in md))
    entry = entry or ("lrm_sam_format_mapq" if mapq is not None else
                      "lrm_sam_format_split" if split is not None or is_text or keep else "lrm_sam_format")
    args = (C.byref(batch), mta, len(mta), _at(cig), _at(score), _at(meta), _at(meta_r), n)
    assert entry == "lrm_sam_format_mapq" or mapq is None, "%s takes no mapq records" % entry
    assert entry != "lrm_sam_format" or (split is None and not is_text and not keep), "lrm_sam_format takes op bytes and no split"
    if entry != "lrm_sam_format":
        args += (int(is_text), int(keep), _at(split)) + ((_at(mapq),) if entry == "lrm_sam_format_mapq" else ())
    return _text(getattr(lib, entry), *args)


def secondary_out(res):
    """The lrm_secondary_out of DeviceMapper.secondary_results() (op bytes in rows) for sam_format(secondary=...) -> (the
    struct, the arrays it points into, which the caller keeps for as long as the struct is in use)."""
    k = len(res["table"])
    held = {name: np.ascontiguousarray(res[name]) for name in ("table", "rows", "lens", "rival", "ops", "score", "meta", "meta_r")}
    held["score"], held["meta_r"] = held["score"].astype(np.int32), held["meta_r"].astype(np.int32)
    ops = held["ops"]
    stride = ops.strides[0] if k else 0
    held["cig"] = cigar_table(np.uint64(ops.ctypes.data) + np.uint64(stride) * np.arange(k, dtype=np.uint64), res["n_ops"], held["score"])
    for name in ("anchor", "clip"):
        held[name] = np.ascontiguousarray(res[name]) if name in res else None
    at = {name: (a.ctypes.data if a is not None else None) for name, a in held.items()}
    out = capi.SecondaryOut(k, k, at["table"], at["rows"], held["rows"].strides[0] if k else 0, at["lens"], at["rival"], at["cig"],
                            at["ops"], stride, at["score"], at["meta"], at["meta_r"], at["anchor"], at["clip"])
    return out, held


def paf_format(batch, mta, cig, score, meta, meta_r, n, summary, *, is_text=0, mapq=None):
    """lrm_paf_format: the PAF lines of a batch from its SUMMARY_DT records [and MAPQ_DT records]."""
    return _text(lib.lrm_paf_format, C.byref(batch), mta, len(mta), _at(cig), _at(score), _at(meta), _at(meta_r), n, int(is_text),
                 _at(summary), _at(mapq))


def pileup_text(host, s, seq_pos, cols):
    """lrm_pileup_format: the lines of len(cols) positions of sequence s of a HostIndex from its base seq_pos (0-based) on;
    cols: PILEUP_COL_DT records, cols[k] for text position mta[s].offset + seq_pos + k."""
    cols = np.ascontiguousarray(cols, dtype=capi.PILEUP_COL_DT)
    room = (int(host.h.mta[s].name_len) + 128) * len(cols) + 1
    buf = C.create_string_buffer(room)
    k = lib.lrm_pileup_format(host.h.mta, host.mta_len, s, seq_pos, len(cols), host.h.content, cols.ctypes.data if len(cols) else None, buf, room)
    if k < 0:
        raise capi.failure("lrm_pileup_format", rc=k)
    return buf.raw[:k]


def write_pileup(path, host, cols, lo, chunk=1 << 16):
    """The pileup records of a window as text: cols[k] is the record of text position lo + k (DeviceMapper.pileup_columns()
    of a window that starts at lo).  One line per position that lies in a sequence of the HostIndex (index.text_window), in
    text order; no header.  -> the number of lines."""
    lines = 0
    with open(path, "wb") as f:
        for s in range(host.mta_len):
            off, n = int(host.h.mta[s].offset), int(host.h.mta[s].seq_len)
            a, b = max(lo, off), min(lo + len(cols), off + n)
            for p in range(a, b, chunk):
                e = min(p + chunk, b)
                f.write(pileup_text(host, s, p - off, cols[p - lo:e - lo]))
                lines += e - p
    return lines


def sites_text(host, sites):
    """lrm_pileup_sites_format: one line per PILEUP_SITE_DT record (DeviceMapper.pileup_sites()) -- sequence name, 1-based
    position, ref, alt, the kinds as letters of SDI, depth, n_ref, n_alt, n_del, n_ins, cons."""
    sites = np.ascontiguousarray(sites, dtype=capi.PILEUP_SITE_DT)
    longest = max((int(host.h.mta[s].name_len) for s in range(host.mta_len)), default=0)
    room = (longest + 96) * len(sites) + 1
    buf = C.create_string_buffer(room)
    k = lib.lrm_pileup_sites_format(host.h.mta, host.mta_len, sites.ctypes.data if len(sites) else None, len(sites), buf, room)
    if k < 0:
        raise capi.failure("lrm_pileup_sites_format", rc=k)
    return buf.raw[:k]


def write_sites(path, host, sites, chunk=1 << 16, alleles=None):
    """The site table as text, no header -> the number of lines.  alleles: the PILEUP_INS_ALLELE_DT records of the same sites
    (DeviceMapper.pileup_site_alleles()); every line then ends on one more column, the inserted bases ('.' when there are none)."""
    assert alleles is None or len(alleles) == len(sites)
    with open(path, "wb") as f:
        for p in range(0, len(sites), chunk):
            text = sites_text(host, sites[p:p + chunk])
            if alleles is not None:
                lines = text.split(b"\n")[:-1]
                text = b"".join(line + b"\t" + (bytes(a["bases"][:int(a["len"])]) or b".") + b"\n" for line, a in zip(lines, alleles[p:p + chunk]))
            f.write(text)
    return len(sites)


def vcf_header(host, sample="SAMPLE"):
    """lrm_vcf_header: the VCF 4.2 header lines of a HostIndex, one ##contig per sequence."""
    room = 2048 + len(os.fsencode(sample)) + sum(64 + int(host.h.mta[s].name_len) for s in range(host.mta_len))
    buf = C.create_string_buffer(room)
    k = lib.lrm_vcf_header(host.h.mta, host.mta_len, os.fsencode(sample), buf, room)
    if k < 0:
        raise capi.failure("lrm_vcf_header", rc=k)
    return buf.raw[:k]


def vcf_text(host, variants):
    """lrm_pileup_variants_format_vcf: one VCF line per PILEUP_VARIANT_DT record (DeviceMapper.pileup_variants())."""
    variants = np.ascontiguousarray(variants, dtype=capi.PILEUP_VARIANT_DT)
    longest = max((int(host.h.mta[s].name_len) for s in range(host.mta_len)), default=0)
    deleted = int(variants["len"][variants["kind"] == capi.CALL_DEL].sum())        # a deletion's REF holds its deleted bases
    room = (longest + 128) * len(variants) + deleted + 1
    buf = C.create_string_buffer(room)
    k = lib.lrm_pileup_variants_format_vcf(host.h.mta, host.mta_len, host.h.content, variants.ctypes.data if len(variants) else None, len(variants), buf, room)
    if k < 0:
        raise capi.failure("lrm_pileup_variants_format_vcf", rc=k)
    return buf.raw[:k]


def write_vcf(path, host, variants, sample="SAMPLE", chunk=1 << 14):
    """The variant table as a VCF file: the header, then one line per record -> the number of records."""
    with open(path, "wb") as f:
        f.write(vcf_header(host, sample))
        for p in range(0, len(variants), chunk):
            f.write(vcf_text(host, variants[p:p + chunk]))
    return len(variants)


def write_consensus(path, host, s, cons, lo):
    """The consensus of sequence s of a HostIndex as FASTA: cons[k] is the letter of text position lo + k
    (DeviceMapper.pileup_sites(consensus=True) of a window that starts at lo) and has to cover the sequence
    (index.text_window).  Deleted positions ('-') are dropped; 60 columns a line.  -> the number of bases written."""
    off, n = int(host.h.mta[s].offset), int(host.h.mta[s].seq_len)
    assert lo <= off and off + n <= lo + len(cons), "the consensus does not cover the sequence"
    letters = np.ascontiguousarray(cons, dtype=np.uint8)[off - lo:off - lo + n]
    letters = letters[letters != ord("-")].tobytes()
    with open(path, "wb") as f:
        f.write(b">" + host.h.mta[s].name[:int(host.h.mta[s].name_len)] + b"\n")
        for p in range(0, len(letters), 60):
            f.write(letters[p:p + 60] + b"\n")
    return len(letters)


def accaln(genome, reads, out, batch_size, seed_len=20, thres=300, gact=(0, 0, 0), device=0, rg_id=1, options=None, mapq=0, paf=False, md=False,
           secondary=None, pileup=None):
    """pileup: dict(seq=-1, ins_cols=0, min_mapq=0, sites=None, fasta=None, min_depth=0, min_count=0, min_pct=0) -- lrm_accaln_pileup:
    the flow of lrm_accaln_mapq with every batch added to one accumulator over sequence seq (-1: all); behind the last batch the
    sites table goes to `sites` and the polished sequences to `fasta` (either may be None).  out=None is allowed with it: no SAM.
    With vcf= in the dict (and hom_pct=0, sample=None) the variant records go to that VCF file too (lrm_accaln_pileup_vcf).
    secondary: an lrm_secondary_options (capi.SecondaryOptions) -- lrm_accaln_secondary: the flow of lrm_accaln_mapq plus a FLAG
    256 line for every reported secondary alignment.
    md: NM:i and MD:Z on every mapped primary line (lrm_accaln_md).
    A whole reads file to SAM (paf: PAF) -> (total, valid): lrm_accaln_paf, or the first of lrm_accaln_mapq / lrm_accaln_opt
    / lrm_accaln that takes what was given (options: an lrm_map_options).  A failure raises LrmError with the code in .rc."""
    total, valid = C.c_uint64(), C.c_uint64()
    head = (os.fsencode(genome), os.fsencode(reads), None if out is None else os.fsencode(out), capi.Params(batch_size, seed_len, thres), capi.GactParams(*gact), device)
    counts, opt = (C.byref(total), C.byref(valid)), _at(options)
    assert not (md and paf), "PAF lines carry no MD:Z"
    assert secondary is None or not (md or paf), "the secondary flow prints SAM without MD:Z"
    assert out is not None or pileup is not None, "only the pileup flow runs without an output file"
    if pileup is not None:
        assert not (md or paf) and secondary is None, "the pileup flow prints the SAM of lrm_accaln_mapq"
        unknown = set(pileup) - {"seq", "ins_cols", "min_mapq", "sites", "fasta", "min_depth", "min_count", "min_pct", "vcf", "hom_pct", "sample"}
        assert not unknown, "pileup has no field %s" % sorted(unknown)
        path = {k: None if pileup.get(k) is None else os.fsencode(pileup[k]) for k in ("sites", "fasta")}
        po = capi.AccalnPileupOptions(C.sizeof(capi.AccalnPileupOptions), pileup.get("ins_cols", 0), pileup.get("min_mapq", 0), 0,
                                      capi.PileupCallOptions(pileup.get("min_depth", 0), pileup.get("min_count", 0), pileup.get("min_pct", 0), 0),
                                      pileup.get("seq", -1), 0, path["sites"], path["fasta"])
        if pileup.get("vcf") is not None:
            sample = pileup.get("sample")
            vo = capi.AccalnVcfOptions(C.sizeof(capi.AccalnVcfOptions), pileup.get("hom_pct", 0), os.fsencode(pileup["vcf"]),
                                       None if sample is None else os.fsencode(sample), 0)
            rc = lib.lrm_accaln_pileup_vcf(*head, rg_id, *counts, opt, mapq, C.byref(po), C.byref(vo))
        else:
            assert "hom_pct" not in pileup and "sample" not in pileup, "hom_pct and sample belong to vcf="
            rc = lib.lrm_accaln_pileup(*head, rg_id, *counts, opt, mapq, C.byref(po))
        if rc < 0:
            raise capi.failure("lrm_accaln_pileup", rc=rc)
        return int(total.value), int(valid.value)
    entry, tail = (("lrm_accaln_secondary", (rg_id, *counts, opt, C.byref(secondary))) if secondary is not None else ("lrm_accaln_paf", (*counts, opt, mapq)) if paf else ("lrm_accaln_md", (rg_id, *counts, opt, mapq, 1)) if md else ("lrm_accaln_mapq", (rg_id, *counts, opt, mapq)) if mapq else
                   ("lrm_accaln_opt", (rg_id, *counts, opt)) if options is not None else ("lrm_accaln", (rg_id, *counts)))
    rc = getattr(lib, entry)(*head, *tail)
    if rc < 0:
        raise capi.failure(entry, rc=rc)
    return int(total.value), int(valid.value)
