"""The byte kernels around the seed and extension stages -- pack2bit_kernel, revcomp_kernel, bs_pack_reads_kernel and
bs_expand_kernel, which handle four bases or four CIGAR columns per instruction (longreadmapper_amd/csrc/base_words.h) --
against the CPU oracle (tests/orc.py), at the sizes where their word, chunk and wavefront boundaries fall.  Batches of at
most 256 reads on a text of 240 kbp; the reads are placed as tests/test_gpu_gact_constructed.py places its reads (best[]
keys written by the test, gact_cases.key_of), so every read extends, on the strand the test chose; seeding is compared
apart, GPU best[] against the oracle's.  Every case runs on the default kernel choice (the byte extension kernels at this
batch size) and with gact_impl = 4 (the bit-sliced kernel, with bs_pack_reads and bs_expand).

  * read lengths around the 16-base dword of pack2bit, the 64-base planar group, the 1-KiB wavefront of the planar pack
    and the reverse complement's RC_SEG, half of the reads on the reverse strand, with row strides max_len + 1 and
    max_len + 2 (between them every row alignment mod 16) and a multiple of 16 (the aligned paths);
  * bs_expand's edges: a read made from n + k text bases by deleting k of them ends k bases after its n-base target
    window does, so its alignment has n + l coded columns (l: bases inserted into the read) and a tail of k - l 'I'
    columns; n and (k, l) are chosen so that the coded columns mod 32 take 0, 1, 15, 16, 17, 31 and the tail is 0, 1, 3,
    4, 5, 15, 16, 17 long (checked on the oracle's own op bytes), with op rows 16 bytes apart and 4 bytes apart only;
  * other bytes: reverse-strand reads that hold a ramp of all 256 byte values at offset 0, 5 and 16 of their row come
    out of extend as comp_base of every byte, reversed (the bit-sliced path hands such a read to the byte kernel, so its
    alignment is the oracle's under gact_impl = 4 too); lower-case reads resolve to the oracle's sequence, strand and
    offset and align as the oracle's (which compares bytes, so a lower-case base matches no text base).

Seeding a read that holds bytes outside ACGT -- lower-case letters among them: the oracle finds no seed in such a read --
is undefined in the oracle; the codes of every byte value are pinned on the CPU (tests/test_base_words_cpu.py)."""
import numpy as np
import pytest

import constructed
import gact_cases
import orc
from longreadmapper_amd import capi, index, mapper

pytestmark = pytest.mark.gpu

GACT = (320, 120, 128)
BITSLICED = 4                                # lrm_map_options.gact_impl
SEQ_LEN = 120_000                            # the text is the sequence and its reverse complement: 240 kbp
LENGTHS = [21, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 8225]
COMP = np.full(256, ord("N"), dtype=np.uint8)                    # comp_base: case folded, anything else -> N
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    COMP[_a] = _b


# ---------------------------------------------------------------------------------------------------------------------
# the text, the reads and the oracle's answers (no device needed)
# ---------------------------------------------------------------------------------------------------------------------
def sequence():
    return gact_cases.rnd(SEQ_LEN, "byte-kernels")


def read_at(seq, pos, n, strand, rng, sub=0.03, ins=0.01, dele=0.01):
    """A read of exactly n bases from the text at pos, with substitutions and indels; reverse strand: its reverse
    complement.  -> (read, key of the window [pos, pos + n))."""
    r = gact_cases._mutate(rng, seq[pos:pos + n + n // 8 + 8], sub, ins, dele)[:n]
    assert len(r) == n
    return (constructed.revcomp(r) if strand else r), gact_cases.key_of(0, len(seq), pos, n, strand)


def length_reads(seq):
    """Four reads of every length in LENGTHS, strands alternating."""
    rng = np.random.default_rng(31)
    reads, keys = [], []
    for n in LENGTHS:
        for rep in range(4):
            pos = int(rng.integers(0, len(seq) - 2 * n - 16))
            r, k = read_at(seq, pos, n, (len(reads) + rep // 2) % 2, rng, *((0.0, 0.0, 0.0) if n < 100 else ()))
            reads.append(r)
            keys.append(k)
    return reads, keys


EDGE_N = [640, 641, 655, 656, 657, 671]                          # n + l mod 32 with l = 0
EDGE_KL = [(0, 0), (1, 0), (3, 0), (4, 0), (5, 0), (15, 0), (16, 0), (17, 0), (5, 2), (18, 1), (2, 2)]


def edge_read(seq, pos, n, k, l, strand):
    """n + k - l text bases from pos, k of them deleted and l bases inserted, all between base 100 and base n - 150 and
    at least 20 apart: n read bases whose window [pos, pos + n) ends k - l bases before the read does."""
    src = bytearray(seq[pos:pos + n + k - l])
    at = [100 + 21 * e for e in range(k + l)]
    assert at[-1] < n - 150 if at else True
    out = bytearray()
    dele, ins = set(at[:k]), set(at[k:])
    for e, c in enumerate(src):
        if e in dele:
            continue
        out.append(c)
        if e in ins:
            out.append(gact_cases.other(gact_cases.other(c), 1))
    assert len(out) == n
    r = bytes(out)
    return (constructed.revcomp(r) if strand else r), gact_cases.key_of(0, len(seq), pos, n, strand)


def edge_reads(seq):
    reads, keys, spec = [], [], []
    for a, n in enumerate(EDGE_N):
        for b, (k, l) in enumerate(EDGE_KL):
            r, key = edge_read(seq, 1000 + 1700 * len(reads), n, k, l, (a + b) % 2)
            reads.append(r)
            keys.append(key)
            spec.append((n, k, l))
    return reads, keys, spec


def tail_of(ops):
    """(coded columns, 'I' columns at the row's end) of an alignment whose coded part ends in a match."""
    t = len(ops) - len(ops.rstrip(b"I"))
    return len(ops) - t, t


def other_byte_reads(seq):
    """-> reads, keys, the indices of the reads that hold the ramp, of the lower-case reads, of the plain ones."""
    rng = np.random.default_rng(37)
    ramp = bytes(range(256))
    reads, keys, ramped, lower, plain = [], [], [], [], []
    for e, off in enumerate((0, 5, 16, 0, 5, 16)):
        n = 1500 + 7 * e
        r, k = read_at(seq, 5000 + 3000 * e, n, 1, rng)
        place = off if e < 3 else n - 256 - off                 # from the row's start, and as far from its end
        reads.append(r[:place] + ramp + r[place + 256:])
        keys.append(k)
        ramped.append(len(reads) - 1)
        r, k = read_at(seq, 40000 + 3000 * e, n + 1, e % 2, rng)
        reads.append(r.lower() if e % 3 else bytes(c | 0x20 if i % 3 == 0 else c for i, c in enumerate(r)))
        keys.append(k)
        lower.append(len(reads) - 1)
        r, k = read_at(seq, 80000 + 3000 * e, n + 2, (e + 1) % 2, rng)
        reads.append(r)
        keys.append(k)
        plain.append(len(reads) - 1)
    return reads, keys, ramped, lower, plain


def oracle_extend(oi, reads, keys):
    """-> the oracle's extend_batch result, with `rows`: the reads as it leaves them."""
    arr, lens = gact_cases.read_matrix(reads)
    best = np.zeros(len(lens), dtype=mapper.ENTRY_DT)
    best["key"] = np.array(keys, dtype=np.uint64)
    want = oi.extend_batch(arr, lens, best, GACT)
    want["rows"] = [bytes(arr[k, :lens[k]]) for k in range(len(lens))]
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(gpu):
    seq = sequence()
    hi = index.HostIndex.build([seq], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu)
    oi = orc.OracleIndex.from_host_index(hi)
    yield seq, di, oi
    di.close()


@pytest.fixture(scope="module")
def lengths(world):
    seq, di, oi = world
    reads, keys = length_reads(seq)
    return reads, keys, oracle_extend(oi, reads, keys)


@pytest.fixture(scope="module")
def edges(world):
    seq, di, oi = world
    reads, keys, spec = edge_reads(seq)
    return reads, keys, spec, oracle_extend(oi, reads, keys)


@pytest.fixture(scope="module")
def others(world):
    seq, di, oi = world
    reads, keys, ramped, lower, plain = other_byte_reads(seq)
    return reads, keys, ramped, lower, plain, oracle_extend(oi, reads, keys)


def gpu_extend(di, reads, keys, stride, store_stride=None):
    """lrm_extend_batch on rows `stride` bytes apart and op rows `store_stride` bytes apart (None: 2 * max_len)."""
    arr, lens = gact_cases.read_matrix(reads, stride)
    lens, n, max_len, batch = mapper._batch(arr, lens)
    best = np.zeros(n, dtype=mapper.ENTRY_DT)
    best["key"] = np.array(keys, dtype=np.uint64)
    buf = mapper.ResultBuffers(n, store_stride or 2 * max_len)
    capi.check(capi.lib.lrm_extend_batch(di.handle, *batch, best.ctypes.data, capi.GactParams(*GACT), *buf.out_args),
               "lrm_extend_batch")
    return buf.result(), arr, lens


def check_extend(got, arr, lens, want, what):
    n = len(lens)
    assert np.array_equal(got["meta_r"], want["meta_r"]) and (got["meta_r"] == 1).all(), what
    for f in ("loc", "off", "seq_id", "strand"):                   # (the records' padding bytes are nobody's result)
        assert np.array_equal(got["meta"][f], want["meta"][f]), (what, f)
    assert np.array_equal(got["score"], want["score"]), (what, np.nonzero(got["score"] != want["score"])[0][:8])
    assert np.array_equal(got["n_ops"], want["n_ops"]), (what, np.nonzero(got["n_ops"] != want["n_ops"])[0][:8])
    for k in range(n):
        m = int(want["n_ops"][k])
        assert bytes(got["ops"][k, :m]) == bytes(want["ops"][k, :m]), (what, k, int(lens[k]))
        assert bytes(arr[k, :lens[k]]) == want["rows"][k], (what, k, int(lens[k]))
        assert not arr[k, lens[k]:].any(), (what, k)               # nothing written past the read's end


def check_seeds(di, oi, reads, stride):
    arr, lens = gact_cases.read_matrix(reads, stride)
    want, _ = oi.seed_batch(arr, lens)
    got = mapper.seed_batch(di, arr, lens)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    return want


def strides(max_len):
    """Read row strides: max_len + 1 and max_len + 2 (one of them is odd: every row alignment mod 16), and a multiple of 16."""
    return {"plus1": max_len + 1, "plus2": max_len + 2, "x16": (max_len + 16) & ~15}


@pytest.mark.parametrize("stride", ["plus1", "plus2", "x16"])
@pytest.mark.parametrize("impl", [0, BITSLICED])
def test_read_lengths(world, lengths, map_options, impl, stride):
    seq, di, oi = world
    reads, keys, want = lengths
    st = strides(max(LENGTHS))[stride]
    assert sorted(set(len(r) for r in reads)) == LENGTHS and len(reads) <= 256
    assert sorted(set(int(s) for s in want["meta"]["strand"])) == [0, 1]
    map_options(di, gact_impl=impl)
    got, arr, lens = gpu_extend(di, reads, keys, st)
    check_extend(got, arr, lens, want, (impl, stride))
    odd = [v for v in strides(max(LENGTHS)).values() if v % 2]
    assert len(odd) == 1 and len({(k * odd[0]) % 16 for k in range(len(reads))}) == 16      # rows at every alignment


@pytest.mark.parametrize("stride", ["plus1", "plus2", "x16"])
def test_read_lengths_seed(world, lengths, stride):
    """pack2bit's full dwords, its tail dword and the read's end at every offset inside a dword; best[] as the oracle's."""
    seq, di, oi = world
    reads, keys, _ = lengths
    want = check_seeds(di, oi, reads, strides(max(LENGTHS))[stride])
    long_ = [k for k, r in enumerate(reads) if len(r) >= 1000]
    near = [k for k in long_ if abs(int(want["key"][k]) - keys[k]) <= 64]        # the voted locus drifts with the indels
    assert len(long_) == 40 and len(near) >= 36, len(near)    # the long reads map where the test put them


def test_expand_edges_are_the_intended_ones(world, edges):
    """By the oracle's own op bytes: read (n, k, l) has n + l coded columns and then k - l 'I' columns."""
    reads, keys, spec, want = edges
    seen = set()
    for i, (n, k, l) in enumerate(spec):
        ops = bytes(want["ops"][i, :int(want["n_ops"][i])])
        assert tail_of(ops) == (n + l, k - l), (n, k, l, tail_of(ops))
        seen.add(((n + l) % 32, k - l))
    assert {c for c, _ in seen} >= {0, 1, 15, 16, 17, 31} and {t for _, t in seen} >= {0, 1, 3, 4, 5, 15, 16, 17}
    assert all((c, t) in seen for c in (0, 1, 15, 16, 17, 31) for t in (0, 1, 3, 4, 5, 15, 16, 17))


@pytest.mark.parametrize("store", ["x16", "x4"])
@pytest.mark.parametrize("impl", [0, BITSLICED])
def test_expand_edges(world, edges, map_options, impl, store):
    seq, di, oi = world
    reads, keys, spec, want = edges
    need = 2 * max(len(r) for r in reads)
    store_stride = (need + 15) & ~15 if store == "x16" else ((need + 15) & ~15) + 4
    assert store_stride % 16 == (0 if store == "x16" else 4) and len(reads) <= 256
    map_options(di, gact_impl=impl)
    got, arr, lens = gpu_extend(di, reads, keys, max(len(r) for r in reads) + 1, store_stride)
    check_extend(got, arr, lens, want, (impl, store))


@pytest.mark.parametrize("impl", [0, BITSLICED])
def test_other_bytes(world, others, map_options, impl):
    seq, di, oi = world
    reads, keys, ramped, lower, plain, want = others
    map_options(di, gact_impl=impl)
    for st in strides(max(len(r) for r in reads)).values():
        got, arr, lens = gpu_extend(di, reads, keys, st)
        check_extend(got, arr, lens, want, (impl, st))
        for k in ramped:                                        # comp_base of every byte, reversed
            src = np.frombuffer(reads[k], dtype=np.uint8)
            assert int(got["meta"]["strand"][k]) == 1 and set(src.tolist()) == set(range(256))
            assert bytes(arr[k, :lens[k]]) == bytes(COMP[src][::-1]), (impl, st, k)
        for k in lower:
            assert int(got["score"][k]) >= 0 and int(got["n_ops"][k]) >= len(reads[k])
