"""End to end on the GPU path: `accidx ref.fa` + `accaln ref.fa reads.fq` (lrm_accidx / lrm_accaln, the
single_end() flow of alnmain.c:277-551) against SAM text assembled from the CPU oracle's results.

Past the first three batches: the pipeline owns four buffer sets, so runs of ten batches use every set again (names,
quals, cig pointers and the pageable store that only grows must not carry anything over); reads with bytes other than
upper-case ACGT ask the formatter's own complement table about more than four bytes; FASTA and gzip reads go through the
same flow; lrm_accaln_opt prints the anchored mode's alignments (POS = first aligned base).

Not reachable here: the pinned branch of lrm_accaln_opt (`want_pinned`) is taken for reads files of 16 GiB and more, which
no test of a sensible size can write; the same pinned buffers are covered below the pipeline by test_gpu_boundary*.py."""
import ctypes as C
import gzip

import numpy as np
import pytest

import anchored_ref
import orc
import sam_ref
from longreadmapper_amd import capi, index, synth
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu


def test_accaln_sam_matches_oracle(gpu, tmp_path):
    seqs = [synth.reference(90_000, seed=31), synth.reference(40_000, seed=32)]
    fa = tmp_path / "ref.fa"
    with open(fa, "wb") as f:
        for nm, s in zip((b"chr1 primary", b"chr2"), seqs):
            f.write(b">" + nm + b"\n")
            b = bytes(s)
            for i in range(0, len(b), 60):
                f.write(b[i:i + 60] + b"\n")
    assert lib.lrm_accidx(str(fa).encode(), 32, 10, 1) == 0
    r = synth.reads(seqs, 150, 1200, synth.ONT, seed=5)
    lens = r["lens"].copy()
    lens[::7] = 300
    lens[3] = 15                                   # shorter than a seed
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for i in range(len(lens)):
            s = bytes(r["reads"][i, :lens[i]])
            f.write(b"@read%d extra\n" % i + s + b"\n+\n" + bytes([33 + (i + j) % 40 for j in range(len(s))]) + b"\n")
    sam = tmp_path / "out.sam"
    total, valid = C.c_uint64(), C.c_uint64()
    p = capi.Params(64, 20, 300)                   # batch of 64: three batches with different max_len
    capi.check(lib.lrm_accaln(str(fa).encode(), str(fq).encode(), str(sam).encode(), p, capi.GactParams(0, 0, 0), gpu,
                              424242, C.byref(total), C.byref(valid)), "lrm_accaln")
    got = open(sam).read()

    hi = index.HostIndex.read(str(fa))
    oi = orc.OracleIndex.from_host_index(hi)
    mta = hi.mta()
    assert [m[0] for m in mta] == ["chr1", "chr2"]
    want = sam_ref.header(mta, 424242)
    n_valid = 0
    for lo in range(0, len(lens), 64):             # the oracle per batch, exactly like the host loop
        bl = lens[lo:lo + 64]
        ml = int(bl.max())
        reads = np.zeros((len(bl), ml + 1), dtype=np.uint8)
        for i, l in enumerate(bl):
            reads[i, :l] = r["reads"][lo + i, :l]
        best, _ = oi.seed_batch(reads, bl)
        ext = oi.extend_batch(reads, bl, best)
        for i, l in enumerate(bl):
            k = int(ext["n_ops"][i])
            qual = "".join(chr(33 + (lo + i + j) % 40) for j in range(l))
            want += sam_ref.record("read%d" % (lo + i), bytes(reads[i, :l]).decode(), qual, mta, bytes(ext["ops"][i, :k]),
                                   int(ext["score"][i]), int(ext["meta_r"][i]), int(ext["meta"]["seq_id"][i]),
                                   int(ext["meta"]["off"][i]), int(ext["meta"]["strand"][i]))
            n_valid += int(ext["score"][i] >= 0 and ext["meta_r"][i] != 0)
    assert got == want
    assert total.value == len(lens) and valid.value == n_valid
    lines = got.splitlines()[4:]
    # a read shorter than a seed has no votes: best = {0,0,0}, i.e. locus 0 -- which resolves (quirk kept)
    assert lines[3].split("\t")[1:4] == ["0", "chr1", "1"]
    assert sum(l.split("\t")[1] == "16" for l in lines) > 20


# ---- the flow past its first three batches ---------------------------------------------------------------------------------------

RG = 777
GACT = (320, 120, 128)


def _write_fasta(path, names, seqs, width=60):
    with open(path, "wb") as f:
        for nm, s in zip(names, seqs):
            f.write(b">" + nm + b"\n")
            b = bytes(s)
            for i in range(0, len(b), width):
                f.write(b[i:i + width] + b"\n")


@pytest.fixture(scope="module")
def genome(gpu, tmp_path_factory):
    """One small two-sequence FASTA index for the module: (path, sequences, HostIndex, oracle, mta)."""
    seqs = [synth.reference(110_000, seed=41), synth.reference(50_000, seed=42)]
    fa = tmp_path_factory.mktemp("accaln") / "ref.fa"
    _write_fasta(fa, (b"chrA first", b"chrB"), seqs)
    assert lib.lrm_accidx(str(fa).encode(), 32, 10, 1) == 0
    hi = index.HostIndex.read(str(fa))
    return str(fa), seqs, hi, orc.OracleIndex.from_host_index(hi), hi.mta()


def _qual(i, n):
    return bytes(33 + (i * 7 + j) % 41 for j in range(n))


def _fastq(recs):
    return b"".join(b"@" + nm + b" extra words\n" + s + b"\n+\n" + q + b"\n" for nm, s, q in recs)


def _accaln(genome, reads_path, sam_path, batch, gpu, opt="plain"):
    total, valid = C.c_uint64(), C.c_uint64()
    args = (genome[0].encode(), str(reads_path).encode(), str(sam_path).encode(), capi.Params(batch, 20, 300),
            capi.GactParams(*GACT), gpu, RG, C.byref(total), C.byref(valid))
    if opt == "plain":
        capi.check(lib.lrm_accaln(*args), "lrm_accaln")
    else:
        capi.check(lib.lrm_accaln_opt(*args, C.byref(opt) if opt is not None else None), "lrm_accaln_opt")
    return open(sam_path).read(), total.value, valid.value


_FOLD = np.frombuffer(bytes(b"ACGT"[((c >> 1) ^ (c >> 2)) & 3] for c in range(256)), dtype=np.uint8)


def _expected(genome, recs, batch, anchored=False, min_len=0):
    """SAM text of recs = [(name, seq, qual or None)] from the oracle, batch by batch like the host loop.  Seeds: bytes other
    than ACGT are outside the reference's definition and fold to a 2-bit code as INTEGRATION.md says; the extension and the
    in-place reverse complement see the bytes as they are.  anchored: anchored_ref on the oracle's classic meta."""
    _, _, hi, oi, mta = genome
    pairs = [(o, l) for _, o, l in mta]
    want, n_valid = sam_ref.header(mta, RG), 0
    for lo in range(0, len(recs), batch):
        part = recs[lo:lo + batch]
        bl = np.array([len(s) for _, s, _ in part], dtype=np.uint32)
        reads = np.zeros((len(part), int(bl.max()) + 1), dtype=np.uint8)
        for i, (_, s, _) in enumerate(part):
            reads[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
        folded = np.where(reads != 0, _FOLD[reads], 0).astype(np.uint8)
        best, _ = oi.seed_batch(folded, bl, nthreads=8)
        ext = oi.extend_batch(reads, bl, best, GACT, nthreads=8)
        anc = anchored_ref.extend_batch(hi.content(), pairs, reads, bl, ext["meta"], ext["meta_r"], GACT, min_len) if anchored else None
        for i, (nm, s, q) in enumerate(part):
            ops, score, off = bytes(ext["ops"][i, :max(int(ext["n_ops"][i]), 0)]), int(ext["score"][i]), int(ext["meta"]["off"][i])
            if anc is not None and anc[i] is not None:
                ops, score, off = anc[i]["ops"], int(anc[i]["score"]), int(anc[i]["off"])
            want += sam_ref.record(nm.decode(), bytes(reads[i, :len(s)]).decode(), q.decode() if q is not None else None, mta, ops,
                                   score, int(ext["meta_r"][i]), int(ext["meta"]["seq_id"][i]), off, int(ext["meta"]["strand"][i]))
            n_valid += int(score >= 0 and ext["meta_r"][i] != 0)
    return want, n_valid


def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for k, (a, b) in enumerate(zip(g, w)):
        if a != b:
            fa, fb = a.split("\t"), b.split("\t")
            col = next((c for c, (x, y) in enumerate(zip(fa, fb)) if x != y), min(len(fa), len(fb)))
            return "line %d (%s), SAM column %d: %r != %r" % (k, fb[0], col + 1, fa[col][:80] if col < len(fa) else None, fb[col][:80] if col < len(fb) else None)
    return "%d lines against %d" % (len(g), len(w))


def _same_sam(got, want):
    assert got == want, _first_difference(got, want)


def _recycling_reads(seqs):
    """640 reads in ten batches of 64 whose longest read goes up, down and up again; batch 3 holds random sequences."""
    tops = [1200, 300, 2500, 600, 2500, 150, 1800, 300, 2200, 900]
    r = synth.reads(seqs, 640, 2500, synth.ONT, seed=61)
    rng = np.random.default_rng(3)
    recs = []
    for i in range(640):
        b = i // 64
        n = tops[b] if i % 64 == 5 else int(rng.integers(tops[b] // 2, tops[b] + 1))
        s = bytes(r["reads"][i, :n]) if b != 3 else bytes(synth.reference(n, seed=5000 + i))
        recs.append((b"r%d" % i, s, _qual(i, n)))
    return recs


@pytest.mark.parametrize("n_reads", [577, 640])
def test_buffer_sets_are_used_again(genome, gpu, tmp_path, n_reads):
    """Ten batches through four buffer sets.  577 reads: nine full batches and one of a single read; 640: the loader meets
    the end of the file right behind a full batch."""
    recs = _recycling_reads(genome[1])[:n_reads]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(_fastq(recs))
    got, total, valid = _accaln(genome, fq, tmp_path / "out.sam", 64, gpu)
    want, n_valid = _expected(genome, recs, 64)
    _same_sam(got, want)
    assert total == n_reads and valid == n_valid and valid > n_reads * 3 // 4


def test_bytes_other_than_upper_case_acgt(genome, gpu, tmp_path):
    """Lower-case stretches, N and IUPAC letters on both strands: a forward-strand SEQ prints as it came, a reverse-strand
    SEQ as _rev_comp_in_place (alnmain.c:27-60) leaves it: upper-case complement, N for everything else."""
    r = synth.reads(genome[1], 160, 1000, synth.ONT, seed=67)
    rng = np.random.default_rng(8)
    recs = []
    for i in range(160):
        s = bytearray(bytes(r["reads"][i, :1000]))
        if i % 3 != 2:
            a = int(rng.integers(0, 800))
            s[a:a + 150] = bytes(s[a:a + 150]).lower()
        if i % 2:
            for p in rng.integers(0, 1000, size=4):
                s[p] = ord("N")
        if i % 5 == 0:
            for p, c in zip(rng.integers(0, 1000, size=6), b"RYKMSn"):
                s[p] = c
        recs.append((b"q%d" % i, bytes(s), _qual(i, 1000)))
    fq = tmp_path / "reads.fq"
    fq.write_bytes(_fastq(recs))
    got, total, valid = _accaln(genome, fq, tmp_path / "out.sam", 64, gpu)
    want, n_valid = _expected(genome, recs, 64)
    _same_sam(got, want)
    assert total == 160 and valid == n_valid
    body = [l.split("\t") for l in want.splitlines() if not l.startswith("@")]
    rev = [f for f in body if f[1] == "16"]
    fwd = [f for f in body if f[1] == "0"]
    assert len(rev) > 40 and len(fwd) > 40
    assert sum("N" in f[9] for f in rev) > 20 and all(f[9] == f[9].upper() for f in rev)      # the complement table was asked
    assert sum(f[9] != f[9].upper() for f in fwd) > 20 and sum("R" in f[9] or "Y" in f[9] for f in fwd) > 3


def test_fasta_and_gzip_reads(genome, gpu, tmp_path):
    r = synth.reads(genome[1], 150, 900, synth.ONT, seed=71)
    recs = [(b"f%d" % i, bytes(r["reads"][i, :900 - 3 * (i % 50)]), _qual(i, 900 - 3 * (i % 50))) for i in range(150)]
    want, n_valid = _expected(genome, recs, 64)
    gz = tmp_path / "reads.fq.gz"
    gz.write_bytes(gzip.compress(_fastq(recs), 1))
    got, total, valid = _accaln(genome, gz, tmp_path / "gz.sam", 64, gpu)
    _same_sam(got, want)
    assert total == 150 and valid == n_valid
    fa = tmp_path / "reads.fa"
    _write_fasta(fa, [nm + b" comment" for nm, _, _ in recs], [s for _, s, _ in recs], width=70)
    got, total, valid = _accaln(genome, fa, tmp_path / "fa.sam", 64, gpu)
    want_fa, _ = _expected(genome, [(nm, s, None) for nm, s, _ in recs], 64)
    _same_sam(got, want_fa)
    assert total == 150 and valid == n_valid
    assert all(l.split("\t")[10] == "*" for l in got.splitlines() if not l.startswith("@"))


def test_anchored_sam(genome, gpu, tmp_path):
    """lrm_accaln_opt: anchored = 1 prints the anchored mode's alignments, POS is the first aligned base; without options, or
    with anchored = 0, it is lrm_accaln."""
    r = synth.reads(genome[1], 200, 1500, synth.PACBIO_CLR, seed=73)
    recs = [(b"p%d" % i, bytes(r["reads"][i, :1500 - 11 * (i % 64)]), _qual(i, 1500 - 11 * (i % 64))) for i in range(200)]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(_fastq(recs))
    classic, n_classic = _expected(genome, recs, 64)
    for k, min_len in enumerate((0, 12)):
        got, total, valid = _accaln(genome, fq, tmp_path / ("anchored%d.sam" % k), 64, gpu,
                                    capi.map_options(anchored=1, anchor_min_len=min_len))
        want, n_valid = _expected(genome, recs, 64, anchored=True, min_len=min_len)
        _same_sam(got, want)
        assert total == 200 and valid == n_valid
        moved = sum(a.split("\t")[3] != b.split("\t")[3] for a, b in zip(want.splitlines(), classic.splitlines()) if a[0] != "@")
        assert want != classic and moved > 10                                       # POS is the moved off + 1
    plain, total, valid = _accaln(genome, fq, tmp_path / "plain.sam", 64, gpu)
    _same_sam(plain, classic)
    assert total == 200 and valid == n_classic
    for k, opt in enumerate((None, capi.map_options(anchored=0))):
        got, t2, v2 = _accaln(genome, fq, tmp_path / ("opt%d.sam" % k), 64, gpu, opt)
        assert got == plain and (t2, v2) == (total, valid)
