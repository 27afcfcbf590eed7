"""Product CPU index builder (SA-IS + SA-scan lchash) vs the oracle's restatement of
fmi_build / lc_build (comparison sort + 4^hlen backward searches), the on-disk formats
(Notes.txt:6-29, fmidx.c:221-275, lchash.c:106-127, sa_use.h:31-46, alnmain.c:125-140) and the
reference's own ui40 helpers where oracle/_ref is available."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import orc
from longreadmapper_amd import capi, index, synth


def _cases():
    rng = np.random.default_rng(3)
    yield "random-1k", [synth.reference(1000, seed=2)]
    yield "two-seqs", [synth.reference(700, seed=3), synth.reference(333, seed=4)]
    yield "tandem", [np.frombuffer((b"ACGTTGCA" * 60 + b"GGATC" * 31), dtype=np.uint8)]
    yield "homopolymer", [np.frombuffer(b"A" * 200 + b"C" * 50 + b"A" * 77, dtype=np.uint8)]
    yield "planted", [synth.reference(6000, seed=5, repeat_frac=0.3, rep_len=150, rep_copies=6, rep_div=0.02)]
    yield "tiny", [np.frombuffer(b"ACGTACGATT", dtype=np.uint8)]
    _ = rng


@pytest.mark.parametrize("name,seqs", list(_cases()), ids=[n for n, _ in _cases()])
@pytest.mark.parametrize("hlen", [2, 5, 7])
def test_builder_equals_oracle(name, seqs, hlen):
    if sum(len(s) for s in seqs) * 2 < hlen + 2:
        pytest.skip("too short")
    hi = index.HostIndex.build(seqs, o_ratio=32, hlen=hlen)
    oi = orc.OracleIndex.build(seqs, o_ratio=32, hlen=hlen)
    assert hi.length == oi.length
    assert bytes(hi.content()) == bytes(oi.content())
    assert [(o, l) for _, o, l in hi.mta()] == oi.mta()
    assert np.array_equal(hi.sa(), oi.sa())
    assert np.array_equal(hi.c(), oi.c())
    assert bytes(hi.bwt()) == bytes(oi.bwt())
    assert np.array_equal(hi.o(), oi.o())
    assert np.array_equal(hi.csa(), oi.csa())
    assert np.array_equal(hi.lc(), oi.lc())


def test_sa_is_sorted_and_complete_large():
    # size-independent property at a size the comparison-sort oracle would not like
    ref = synth.reference(300_000, seed=9, repeat_frac=0.1, rep_len=300, rep_copies=20)
    hi = index.HostIndex.build([ref], hlen=6)
    sa = hi.sa().astype(np.int64)
    L = hi.length
    assert np.array_equal(np.sort(sa), np.arange(L))
    text = hi.content()
    # adjacent suffixes in order: compare 64-byte prefixes (ties beyond that are checked on a sample)
    pad = np.concatenate([text, np.zeros(64, dtype=np.uint8)])
    win = np.lib.stride_tricks.sliding_window_view(pad, 64)
    a, b = win[sa[:-1]], win[sa[1:]]
    neq = a != b
    first = neq.argmax(axis=1)
    tie = ~neq.any(axis=1)
    rows = np.arange(L - 1)
    assert np.all((a[rows, first] < b[rows, first]) | tie)
    for r in np.nonzero(tie)[0][:200]:
        x, y = int(sa[r]), int(sa[r + 1])
        assert bytes(text[x:]) < bytes(text[y:])


def test_cat_layout_and_n_replacement():
    hi = index.HostIndex.build([b"acgtn", b"GGN"], names=["chrA", "chrB"], hlen=2)
    cat = bytes(hi.content())
    assert len(cat) == 2 * 5 + 2 * 3 + 1 and cat.endswith(b"$")
    assert cat[:4] == b"ACGT" and cat[4:5] in (b"A", b"C", b"G", b"T")
    fwd = cat[:5]
    assert cat[5:10] == orc.rev_comp(fwd)                       # fwd + revcomp per record (asindex.c:97-102)
    assert hi.mta() == [("chrA", 0, 5), ("chrB", 10, 3)]


def test_file_formats_roundtrip(tmp_path):
    ref = synth.reference(5000, seed=12)
    hi = index.HostIndex.build([ref, ref[:100]], names=["one", "two"], hlen=5)
    g = str(tmp_path / "ref.fa")
    hi.write(g)
    L = hi.length
    # sizes documented in SURVEY section 8: .sa5 = 5L, .lch = 4+8+8*2*4^h, .mfi formula
    assert os.path.getsize(g + ".cat") == L
    assert os.path.getsize(g + ".cat.sa5") == 5 * L                       # test/test-ui40read.cc:39-57
    assert os.path.getsize(g + ".cat.lch") == 4 + 8 + 8 * 2 * 4 ** 5
    o_len, csa_len = 4 * (L // 32 + 1), L // 4 + 1
    assert os.path.getsize(g + ".cat.mfi") == 2048 + 4 + 8 + 8 * o_len + 8 + L + 4 + 8 + 8 * csa_len
    raw = open(g + ".cat.mfi", "rb").read()
    assert struct.unpack_from("<i", raw, 2048)[0] == 32 and struct.unpack_from("<Q", raw, 2052)[0] == o_len
    mta = open(g + ".mta", "rb").read()
    assert mta[:8] == struct.pack("<Q", 3) and mta[8:11] == b"one"       # mstring_write: length, bytes
    assert struct.unpack_from("<QQ", mta, 11) == (0, 5000)
    back = index.HostIndex.read(g)
    assert back.length == L and back.hlen == 5
    for f in ("c", "o", "csa", "bwt", "lc", "sa", "content"):
        assert np.array_equal(getattr(back, f)(), getattr(hi, f)()), f
    assert back.mta() == hi.mta()
    # the reference's own reader (sa_use.h ui40_fread) sees the same values
    rl = orc.ref_ui40_lib()
    if rl is not None:
        assert rl.ref_ui40_sizeof() == 8                                 # 8 bytes in RAM, 5 on disk
        out = np.zeros(L, dtype=np.uint64)
        n = rl.ref_ui40_fread_path((g + ".cat.sa5").encode(), out.ctypes.data, L)
        assert n == L and np.array_equal(out, hi.sa())


def test_ui40_in_memory_layout_matches_reference():
    # test/test-ui40read.cc:12-37: struct {u32 low; u8 high} written raw is 8 bytes
    assert C.sizeof(capi.Ui40) == 8
    rl = orc.ref_ui40_lib()
    if rl is None:
        pytest.skip("oracle/_ref not built here")
    b = (C.c_uint8 * 8)(4, 3, 2, 1, 5, 0, 0, 0)
    assert rl.ref_ui40_from_bytes_convert(b) == (5 << 32) | 0x01020304


def test_accidx_from_fasta(tmp_path):
    ref = synth.reference(3000, seed=21)
    fa = tmp_path / "g.fa"
    with open(fa, "wb") as f:
        f.write(b">chr1 some description\n")
        s = bytes(ref)
        for i in range(0, len(s), 70):
            f.write(s[i:i + 70].lower() + b"\n")
        f.write(b">chr2\n" + bytes(ref[:500]) + b"\n")
    assert capi.lib.lrm_accidx(str(fa).encode(), 32, 6, 1) == 0
    got = index.HostIndex.read(str(fa))
    want = index.HostIndex.build([ref, ref[:500]], names=["chr1", "chr2"], hlen=6)
    assert got.mta() == want.mta()
    for f in ("c", "o", "csa", "bwt", "lc", "sa", "content"):
        assert np.array_equal(getattr(got, f)(), getattr(want, f)()), f


def test_pack_blob_rejects_inconsistent_index():
    hi = index.HostIndex.build([synth.reference(500, seed=1)], hlen=3)
    hi.o()[5] += 1
    with pytest.raises(capi.LrmError, match="O table disagrees"):
        hi.pack_blob()


def _sa_with(algo, text, monkeypatch, scratch=None):
    monkeypatch.setenv("LRM_SA_ALGO", algo)
    if scratch:
        monkeypatch.setenv("LRM_SA_SCRATCH_ROWS", str(scratch))
    buf = np.frombuffer(text, dtype=np.uint8)
    out = np.full(len(text), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)          # ui40 slots: 8 bytes each
    assert capi.lib.lrm_sa_build(buf.ctypes.data, len(text), out.ctypes.data) == 0, capi.lib.lrm_last_error()
    monkeypatch.delenv("LRM_SA_ALGO")
    if scratch:
        monkeypatch.delenv("LRM_SA_SCRATCH_ROWS")
    return out


def _sa_texts():
    yield "random", bytes(synth.reference(300_000, seed=11)) + b"$"
    yield "planted", bytes(synth.reference(400_000, seed=12, repeat_frac=0.3, rep_len=300, rep_copies=50, rep_div=0.02)) + b"$"
    yield "ends-in-A-run", bytes(synth.reference(70_000, seed=13)) + b"A" * 100 + b"$"        # suffixes that run into '$' inside the key window
    yield "poly-A", b"A" * 5000 + b"$"                                                           # every comparison ends at '$'
    yield "tandem", b"ACGTTGCA" * 4000 + b"$"                                                    # long exact repeats: ties through the text
    yield "exact-copies", bytes(synth.reference(3000, seed=14)) * 30 + b"$"
    yield "tiny", b"GATTACA$"
    yield "one", b"C$"
    yield "empty", b"$"


@pytest.mark.parametrize("name,text", list(_sa_texts()), ids=[n for n, _ in _sa_texts()])
def test_parallel_suffix_sorter_equals_sais(monkeypatch, name, text):
    """The bucketed parallel sorter (what GRCh38-sized texts need) against the linear-time SA-IS on the same text,
    with a scratch so small that the buckets go through many groups; padding bytes of the ui40 slots are zeroed."""
    want = _sa_with("sais", text, monkeypatch)
    assert np.array_equal(np.sort(want), np.arange(len(text), dtype=np.uint64))
    for scratch in (None, 1024):
        got = _sa_with("bucket", text, monkeypatch, scratch)
        assert np.array_equal(got, want), (name, scratch)


def test_suffix_sorter_falls_back_on_repetitive_text(monkeypatch):
    """Automatic mode: the tie budget sends a text of long exact repeats to SA-IS; a lower-case / non-ACGT text
    takes the generic path at once.  Same suffix array either way."""
    text = b"ACGTTGCA" * 30000 + b"$"
    want = _sa_with("sais", text, monkeypatch)
    buf = np.frombuffer(text, dtype=np.uint8)
    out = np.zeros(len(text), dtype=np.uint64)
    assert capi.lib.lrm_sa_build(buf.ctypes.data, len(text), out.ctypes.data) == 0
    assert np.array_equal(out, want)
    text = bytes(synth.reference(5000, seed=3)).lower() + b"NNNN" + bytes(synth.reference(100, seed=4)) + b"$"
    buf = np.frombuffer(text, dtype=np.uint8)
    out = np.zeros(len(text), dtype=np.uint64)
    assert capi.lib.lrm_sa_build(buf.ctypes.data, len(text), out.ctypes.data) == 0
    sa = out.astype(np.int64)
    sufs = [text[i:] for i in sa[:200]]
    assert sufs == sorted(sufs) and np.array_equal(np.sort(sa), np.arange(len(text)))


# ---- files that end early, readers called directly, builds side by side, texts that are not upper-case ACGT ----

_FILES = (".mta", ".cat", ".cat.mfi", ".cat.lch", ".cat.sa5")


@pytest.fixture(scope="module")
def small_index_files(tmp_path_factory):
    """A 2000-base, two-sequence index (hlen 4) written once; every case below works on its own copy of the files."""
    ref = synth.reference(2000, seed=17)
    hi = index.HostIndex.build([ref[:1300], ref[1300:]], names=["one", "two"], hlen=4)
    g = str(tmp_path_factory.mktemp("small_index") / "ref.fa")
    hi.write(g)
    return g, hi


def _copy_index(g, tmp_path):
    import shutil
    dst = str(tmp_path / "ref.fa")
    for ext in _FILES:
        shutil.copy(g + ext, dst + ext)
    return dst


def _cut(path, size):
    assert 0 <= size < os.path.getsize(path)
    with open(path, "r+b") as f:
        f.truncate(size)


def _field_cuts(sizes):
    """A byte offset inside every field of a file whose fields have these sizes."""
    at, cuts = 0, []
    for s in sizes:
        cuts.append(at + s // 2)
        at += s
    return cuts


_L_SMALL = 2 * 2000 + 1
_MFI_FIELDS = ("c", "o_ratio", "o_len", "o", "length", "bwt", "csa_ratio", "csa_len", "csa")
_MFI_SIZES = (2048, 4, 8, 8 * 4 * (_L_SMALL // 32 + 1), 8, _L_SMALL, 4, 8, 8 * (_L_SMALL // 4 + 1))
_LCH_FIELDS = ("hlen", "len", "lc")
_LCH_SIZES = (4, 8, 8 * 2 * 4 ** 4)
_TRUNCATIONS = [(".cat.mfi", f, c) for f, c in zip(_MFI_FIELDS, _field_cuts(_MFI_SIZES))] + \
               [(".cat.lch", f, c) for f, c in zip(_LCH_FIELDS, _field_cuts(_LCH_SIZES))]


@pytest.mark.parametrize("ext,field,cut", _TRUNCATIONS, ids=["%s-%s" % (e[5:], f) for e, f, _ in _TRUNCATIONS])
def test_read_of_truncated_table_file_fails_and_names_it(small_index_files, tmp_path, ext, field, cut):
    g, hi = small_index_files
    assert os.path.getsize(g + ".cat.mfi") == sum(_MFI_SIZES) and os.path.getsize(g + ".cat.lch") == sum(_LCH_SIZES)
    d = _copy_index(g, tmp_path)
    _cut(d + ext, cut)
    with pytest.raises(capi.LrmError) as e:
        index.HostIndex.read(d)
    assert os.path.basename(d + ext) in str(e.value)


def test_read_without_cat_fails_and_names_it(small_index_files, tmp_path):
    d = _copy_index(small_index_files[0], tmp_path)
    os.remove(d + ".cat")
    with pytest.raises(capi.LrmError) as e:
        index.HostIndex.read(d)
    assert os.path.basename(d + ".cat") in str(e.value) and ".cat." not in str(e.value)


def test_read_of_truncated_mta_and_sa5_keeps_what_is_whole(small_index_files, tmp_path):
    g, hi = small_index_files
    d = _copy_index(g, tmp_path)
    rec = 8 + 3 + 8 + 8                                       # name length, "one", offset, seq_len
    assert os.path.getsize(d + ".mta") == 2 * rec
    _cut(d + ".mta", rec + rec // 2)                          # the middle of the second record (alnmain.c:125-140 stops there)
    back = index.HostIndex.read(d)
    assert back.mta() == hi.mta()[:1] == [("one", 0, 1300)]
    k = 1234
    _cut(d + ".cat.sa5", 5 * k)                               # ui40_fread semantics: the count it got (sa_use.h:31-46)
    back = index.HostIndex.read(d)
    assert int(back.h.sa.len) == k and np.array_equal(back.sa(), hi.sa()[:k])
    assert back.length == hi.length and np.array_equal(back.bwt(), hi.bwt())


def test_direct_readers_leave_a_zeroed_struct_on_failure(small_index_files, tmp_path):
    d = _copy_index(small_index_files[0], tmp_path)
    _cut(d + ".cat.mfi", _field_cuts(_MFI_SIZES)[5])          # inside bwt: c and o were allocated by then
    _cut(d + ".cat.lch", _field_cuts(_LCH_SIZES)[2])          # inside lc
    fmi = capi.DnaFmi()
    C.memset(C.byref(fmi), 0xFF, C.sizeof(fmi))
    assert capi.lib.lrm_fmi_read(C.byref(fmi), (d + ".cat").encode()) == -1
    assert b".cat.mfi" in capi.lib.lrm_last_error()
    assert not fmi.c and not fmi.o and not fmi.csa and not fmi.bwt
    assert bytes(fmi) == bytes(C.sizeof(fmi))
    lch = capi.LcHash()
    C.memset(C.byref(lch), 0xFF, C.sizeof(lch))
    assert capi.lib.lrm_lc_read((d + ".cat.lch").encode(), C.byref(lch)) == -1
    assert b".cat.lch" in capi.lib.lrm_last_error()
    assert not lch.lc
    assert bytes(lch) == bytes(C.sizeof(lch))


def test_concurrent_builds_equal_serial_builds():
    """Two builds at once in one process (ctypes releases the GIL): no state is shared between them."""
    import threading
    texts = [synth.reference(50_000, seed=41), synth.reference(50_000, seed=42)]
    want = []
    for t in texts:
        hi = index.HostIndex.build([t], hlen=6)
        want.append((hi.sa().copy(), hi.bwt().copy(), hi.lc().copy()))
    bad = []

    def work(i):
        for _ in range(4):
            hi = index.HostIndex.build([texts[i]], hlen=6)
            if not all(np.array_equal(a, b) for a, b in zip((hi.sa(), hi.bwt(), hi.lc()), want[i])):
                bad.append(i)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad


def test_lower_case_text_builds_the_recorded_tables():
    """A text handed straight to lrm_host_index_build is not upper-cased: lower-case bases take the generic paths (SA-IS,
    byte-wise C table, tolerant base codes in the O table and the lchash).  tests/golden/lower_case_index.npz holds the
    text and the tables the library built from it before the builder was split into files."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lower_case_index.npz"))
    text = np.ascontiguousarray(gold["text"])
    assert len(text) == 3000 and bytes(text[-1:]) == b"$" and bytes(text[:-1]).islower()
    h = capi.HostIndex()
    capi.check(capi.lib.lrm_host_index_build(text.ctypes.data, len(text), None, 0, 32, 4, C.byref(h)), "lrm_host_index_build")
    try:
        hi = index.HostIndex()
        hi.h = h
        for f in ("c", "o", "bwt", "lc", "sa"):
            assert np.array_equal(getattr(hi, f)(), gold[f]), f
    finally:
        capi.lib.lrm_host_index_free(C.byref(h))
