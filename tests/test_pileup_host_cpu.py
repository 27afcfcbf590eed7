"""The host side of the pileup on the host-buffer path (docs/GACT_SPEC.md, "Pileup on the host-buffer path and across
replicas") without a GPU: the new symbols and the layout of the two request structs, lrm_pileup_sites_format_ins against the
bytes of textio.write_sites(alleles=), and the refusals of lrm_accaln_pileup, which come before any output file exists."""
import ctypes as C
import os

import pytest

import pileup_host_cases as HC
from longreadmapper_amd import capi, index, synth, textio
from longreadmapper_amd.capi import lib


def _layout(s):
    return [(f, getattr(s, f).offset, getattr(s, f).size) for f, _ in s._fields_]


def test_symbols_and_struct_layouts():
    for name in ("lrm_map_batch_submit_ex3", "lrm_pileup_merge_dev", "lrm_debug_pileup_merge_staged", "lrm_pileup_create_replica",
                 "lrm_pileup_sites_format_ins", "lrm_accaln_pileup"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    # what stays as it was
    assert lib.lrm_abi_version() == 3 and capi.N_KERNELS == 9
    assert C.sizeof(capi.BatchExtras) == 24 and C.sizeof(capi.BatchDiff) == 48 and C.sizeof(capi.MapOptions) == 76
    # the header's layout (tests/test_aln_diff_cpu.py compiles the header and compares every struct of LATER_STRUCTS with it)
    assert capi.LATER_STRUCTS[capi.BatchPileup] == "lrm_batch_pileup" and capi.LATER_STRUCTS[capi.AccalnPileupOptions] == "lrm_accaln_pileup_options"
    assert C.sizeof(capi.BatchPileup) == 24
    assert _layout(capi.BatchPileup) == [("struct_size", 0, 4), ("min_mapq", 4, 4), ("pileups", 8, 8), ("n_pileups", 16, 4), ("reserved", 20, 4)]
    assert C.sizeof(capi.AccalnPileupOptions) == 56
    assert _layout(capi.AccalnPileupOptions) == [("struct_size", 0, 4), ("ins_cols", 4, 4), ("min_mapq", 8, 4), ("reserved", 12, 4), ("call", 16, 16),
                                                 ("seq", 32, 4), ("reserved2", 36, 4), ("sites_path", 40, 8), ("fasta_path", 48, 8)]


@pytest.fixture(scope="module")
def host():
    hi = index.HostIndex.build([synth.reference(700, seed=3), synth.reference(61, seed=4), synth.reference(300, seed=5)],
                               names=["first sequence", "b", "chrThree"], hlen=3)
    yield hi
    hi.close()


def test_sites_format_ins_equals_the_python_writer(host, tmp_path):
    sites, alleles = HC.site_tables(host.mta())
    assert {int(a["len"]) for a in alleles} >= {0, 1, 8}
    offs = {off for _, off, _ in host.mta()} | {off + n - 1 for _, off, n in host.mta()}
    assert offs <= {int(s["pos"]) for s in sites}                       # a site on every sequence's first and last base
    path = str(tmp_path / "sites.tsv")
    assert textio.write_sites(path, host, sites, alleles=alleles) == len(sites)
    want = open(path, "rb").read()
    k, got = HC.sites_format_ins(host, sites, alleles)
    assert k == len(want) and got == want
    lines = want.split(b"\n")[:-1]
    assert len(lines) == len(sites) and all(len(line.split(b"\t")) == 12 for line in lines)
    assert [line.split(b"\t")[11] for line in lines[:4]] == [b".", b"G", b"GATTACAT", b"GAT"]
    assert lines[0].startswith(b"first sequence\t1\t") and any(line.startswith(b"b\t61\t") for line in lines)
    # one record at a time, and none
    for i in range(len(sites)):
        assert HC.sites_format_ins(host, sites[i:i + 1], alleles[i:i + 1])[1] == lines[i] + b"\n"
    assert HC.sites_format_ins(host, sites[:0], alleles[:0]) == (0, b"")
    # NULL alleles: lrm_pileup_sites_format
    plain = textio.sites_text(host, sites)
    assert HC.sites_format_ins(host, sites, None) == (len(plain), plain)
    assert all(len(line.split(b"\t")) == 11 for line in plain.split(b"\n")[:-1])
    # a buffer with no room for the new column of its last line
    k, _ = HC.sites_format_ins(host, sites, alleles, room=len(want))
    assert k == -2 and b"too small" in lib.lrm_last_error()
    far = sites[:1].copy()
    far["pos"] = 10**9
    assert HC.sites_format_ins(host, far, alleles[:1])[0] == -1 and b"lies in no sequence" in lib.lrm_last_error()


def _accaln_pileup(genome, reads, sam, mapq, **kw):
    path = {k: None if kw.get(k) is None else os.fsencode(kw[k]) for k in ("sites", "fasta")}
    po = capi.AccalnPileupOptions(kw.get("struct_size", C.sizeof(capi.AccalnPileupOptions)), kw.get("ins_cols", 0), kw.get("min_mapq", 0),
                                  kw.get("reserved", 0), capi.PileupCallOptions(0, 0, kw.get("min_pct", 0), kw.get("call_reserved", 0)),
                                  kw.get("seq", -1), kw.get("reserved2", 0), path["sites"], path["fasta"])
    total, valid = C.c_uint64(), C.c_uint64()
    rc = lib.lrm_accaln_pileup(os.fsencode(genome), os.fsencode(reads), None if sam is None else os.fsencode(sam), capi.Params(64, 20, 300),
                               capi.GactParams(0, 0, 0), 0, 1, C.byref(total), C.byref(valid), None, mapq, C.byref(po))
    return rc, lib.lrm_last_error()


def test_accaln_pileup_refusals_come_before_any_output(tmp_path):
    fa, fq = tmp_path / "ref.fa", tmp_path / "reads.fq"
    seqs = [synth.reference(3000, seed=8), synth.reference(2000, seed=9)]
    HC.write_fasta(fa, zip((b"one", b"two"), seqs))
    assert lib.lrm_accidx(str(fa).encode(), 32, 6, 1) == 0
    r = synth.reads(seqs, 4, 300, synth.CLEAN, seed=2)
    HC.write_fastq(fq, r["reads"], r["lens"])
    out = dict(sites=tmp_path / "s.tsv", fasta=tmp_path / "c.fa")
    sam = tmp_path / "out.sam"
    for kw, mapq, text in ((dict(min_mapq=1), 0, b"min_mapq needs mapq"),
                           (dict(reserved=1), 1, b"reserved"), (dict(reserved2=7), 1, b"reserved"), (dict(call_reserved=1), 1, b"reserved"),
                           (dict(seq=2), 1, b"seq 2"), (dict(seq=-2), 1, b"seq -2"), (dict(seq=2**31 - 1), 0, b"seq 2147483647"),
                           (dict(ins_cols=9), 0, b"insertion columns"), (dict(min_pct=101), 0, b"min_pct"), (dict(struct_size=48), 0, b"struct_size")):
        for s in (sam, None):
            rc, err = _accaln_pileup(fa, fq, s, mapq, **out, **kw)
            assert rc == -1 and text in err, (kw, err)
            assert not sam.exists() and not out["sites"].exists() and not out["fasta"].exists(), kw
    assert sorted(p.name for p in tmp_path.iterdir() if p.suffix in (".sam", ".tsv")) == []


def test_textio_accaln_takes_the_request(tmp_path):
    """the Python layer builds the same request: a refusal of the library comes back as LrmError, unknown fields are caught here"""
    with pytest.raises(capi.LrmError, match="min_mapq needs mapq"):
        textio.accaln(str(tmp_path / "none.fa"), str(tmp_path / "none.fq"), None, 64, pileup=dict(seq=0, min_mapq=3, sites=str(tmp_path / "s.tsv")))
    with pytest.raises(AssertionError, match="no field"):
        textio.accaln(str(tmp_path / "none.fa"), str(tmp_path / "none.fq"), None, 64, pileup=dict(sequence=0))
    with pytest.raises(AssertionError):
        textio.accaln(str(tmp_path / "none.fa"), str(tmp_path / "none.fq"), None, 64)
    assert not (tmp_path / "s.tsv").exists()
