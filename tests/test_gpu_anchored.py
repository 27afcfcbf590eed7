"""The anchored extension mode on the GPU against tests/anchored_ref.py (brute-force anchor, orc_gact jobs, stitch)."""
import numpy as np
import pytest

import anchored_cases
import anchored_ref
import orc
from longreadmapper_amd import capi, index, mapper, synth

pytestmark = pytest.mark.gpu
GACT = (320, 120, 128)
ANCHOR_KEYS = ("text_pos", "read_pos", "len", "delta", "left_ops", "flags")


@pytest.fixture(scope="module")
def small(gpu):
    """The constructed three-sequence text, uploaded."""
    ss = anchored_cases.seqs()
    hi = index.HostIndex.build(ss, hlen=8)
    text, mta, cases = anchored_cases.cases()
    assert bytes(hi.content()[:len(text) - 1]) == bytes(text[:-1])
    di = index.DeviceIndex.upload(hi, gpu)
    yield ss, hi, di, text, mta, cases
    di.close()


@pytest.fixture(scope="module")
def ref3(gpu):
    seqs = [synth.reference(1_500_000, seed=41, repeat_frac=0.05, rep_len=300, rep_copies=200, rep_div=0.05),
            synth.reference(700_000, seed=42), synth.reference(300_000, seed=43)]
    hi = index.HostIndex.build(seqs, names=["chrA", "chrB", "chrC"], hlen=12)
    di = index.DeviceIndex.upload(hi, gpu)
    yield seqs, hi, di
    di.close()


def _same_meta(a, b):
    """lrm_seq_meta field by field (the struct's padding bytes are not part of the result)."""
    return all(np.array_equal(a[f], b[f]) for f in ("loc", "off", "seq_id", "strand"))


def _anchor_tuple(a):
    return (a["len"], a["delta"], a["read_pos"]) if a["flags"] & capi.ANCHOR_ANCHORED else None


def test_debug_anchor_on_the_constructed_cases(small):
    ss, hi, di, text, mta, cases = small
    for c in cases:
        S, len_s = mta[c["seq"]]
        L = c["L"]
        if not S <= L < S + len_s:                         # the tap takes loci on the forward half only
            continue
        got = mapper.debug_anchor(di, c["read"], L, c["min_len"])
        assert _anchor_tuple(got) == c["want"], c["name"]
        if c["want"]:
            assert got["text_pos"] == L + got["delta"] + got["read_pos"]
        else:
            assert got["flags"] == capi.ANCHOR_FALLBACK


def test_debug_anchor_on_sampled_reads(ref3):
    seqs, hi, di = ref3
    text = hi.content()
    mta = [(o, l) for _, o, l in hi.mta()]
    rng = np.random.default_rng(9)
    checked = anchored = 0
    for profile, length, count, seed in ((synth.ONT, 1, 4, 1), (synth.ONT, 37, 6, 2), (synth.PACBIO_CLR, 700, 12, 3),
                                         (synth.ONT, 2048, 8, 4), (synth.PACBIO_CLR, 5000, 10, 5), (synth.ONT, 20_000, 8, 6),
                                         (synth.PACBIO_CLR, 100_000, 3, 7)):
        r = synth.reads(seqs, count, length, profile, seed=seed)
        for i in range(count):
            read = r["reads"][i, :int(r["lens"][i])]
            if r["strand"][i]:
                read = anchored_ref.revcomp(read)
            S, len_s = mta[int(r["seq"][i])]
            L = int(min(max(S + int(r["pos"][i]) + int(rng.integers(-40, 41)), S), S + len_s - 1))
            want = anchored_ref.find_anchor(read, text, L, S, len_s)
            got = mapper.debug_anchor(di, read, L)
            assert _anchor_tuple(got) == want, (length, i)
            checked += 1
            anchored += want is not None
    assert checked > 40 and anchored > 20


def _ragged_batch(seqs, mta, n_total, seed=21):
    """Reads of many lengths with loci built from the truth (jittered), random reads (no anchor), reads at the sequence
    edges, and loci that resolve to no sequence.  -> reads (n, stride), lens, best"""
    rng = np.random.default_rng(seed)
    parts = []
    shapes = [(60, 0.30), (150, 0.30), (400, 0.25), (900, 0.10), (2100, 0.04), (4200, 0.01)]
    for k, (length, frac) in enumerate(shapes):
        cnt = int(n_total * frac)
        r = synth.reads(seqs, cnt, length, synth.PACBIO_CLR if k % 2 else synth.ONT, seed=seed + k)
        parts.append(r)
    stride = max(p["reads"].shape[1] for p in parts)
    n = sum(len(p["lens"]) for p in parts)
    reads = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    best = np.zeros(n, dtype=mapper.ENTRY_DT)
    at = 0
    for p in parts:
        m = len(p["lens"])
        reads[at:at + m, :p["reads"].shape[1]] = p["reads"]
        lens[at:at + m] = p["lens"]
        S = np.array([mta[s][0] for s in p["seq"]], dtype=np.int64)
        ls = np.array([mta[s][1] for s in p["seq"]], dtype=np.int64)
        pos = p["pos"].astype(np.int64) + rng.integers(-20, 21, m)
        fwd = S + pos
        rev = S + 2 * ls - (p["pos"].astype(np.int64) + p["span"].astype(np.int64)) + rng.integers(-20, 21, m)
        best["key"][at:at + m] = np.where(p["strand"] == 0, fwd, rev).clip(0).astype(np.uint64)
        at += m
    # every 16th read: random bases at its locus (mapped, never anchored)
    for i in range(0, n, 16):
        reads[i, :lens[i]] = anchored_cases._BASES[rng.integers(0, 4, int(lens[i]))]
    # sequence edges: windows that start at the first base / end at the last base of a sequence, both strands
    for k, i in enumerate(range(5, n, 97)):
        s = k % len(mta)
        S, ls = mta[s]
        ln = int(lens[i])
        start = 0 if k % 2 == 0 else ls - ln
        fwd = seqs[s][start:start + ln].copy()
        fwd[5::37] = anchored_cases._BASES[(np.searchsorted(anchored_cases._BASES, fwd[5::37]) + 1) % 4]
        if k % 4 < 2:
            reads[i, :ln], best["key"][i] = fwd, S + start
        else:
            reads[i, :ln], best["key"][i] = anchored_ref.revcomp(fwd), S + 2 * ls - (start + ln)
    # windows that straddle the two halves of a sequence resolve to nothing: no extension at all
    for i in range(7, n, 101):
        best["key"][i] = mta[0][0] + mta[0][1] - 5
    return reads, lens, best


def _check_against_ref(got, want, anchors=None):
    bad = []
    for i, w in enumerate(want):
        if w is None:
            ok = got["meta_r"][i] == 0 and got["score"][i] == -1 and got["n_ops"][i] == 0
        else:
            k = w["n_ops"]
            ok = (got["meta_r"][i] == 1 and got["n_ops"][i] == k and got["score"][i] == w["score"] and
                  bytes(got["ops"][i, :k]) == w["ops"] and int(got["meta"]["loc"][i]) == w["loc"] and
                  int(got["meta"]["off"][i]) == w["off"])
            if ok and anchors is not None:
                ok = all(int(anchors[key][i]) == w[key] for key in ANCHOR_KEYS)
        if not ok:
            bad.append(i)
    assert not bad, (len(bad), bad[:5])


@pytest.fixture(scope="module")
def ragged(ref3):
    seqs, hi, di = ref3
    mta = [(o, l) for _, o, l in hi.mta()]
    reads, lens, best = _ragged_batch(seqs, mta, 21_000)
    assert len(lens) >= 20_000
    di.set_map_options()
    oriented = reads.copy()
    classic = mapper.extend_batch(di, oriented, lens, best, GACT)
    return reads, lens, best, oriented, classic, mta


def test_batch_equals_reference_on_the_bitsliced_kernel(ref3, ragged, gpu):
    """>= 20 000 reads, automatic dispatch: the launch record shows the bit-sliced kernel; ops, n_ops, score, meta,
    meta_r and the lrm_anchor records equal the reference."""
    import torch
    seqs, hi, di = ref3
    reads, lens, best, oriented, classic, mta = ragged
    want = anchored_ref.extend_batch(hi.content(), mta, oriented, lens, classic["meta"], classic["meta_r"], GACT)
    kinds = [w["flags"] if w else 0 for w in want]
    assert sum(k == anchored_ref.FALLBACK for k in kinds) > 500 and sum(k == 0 for k in kinds) > 0
    assert sum(bool(k & anchored_ref.LEFT_CLIPPED) for k in kinds) > 0 and sum(bool(k & anchored_ref.RIGHT_CLIPPED) for k in kinds) > 0
    n, max_len = len(lens), int(lens.max())
    dm = mapper.DeviceMapper(di, n, max_len, gact=GACT, device=gpu, anchored=True)
    before = dm.workspace_bytes()
    dm.set_timing(True)
    dm.best[:, 0] = torch.from_numpy(best["key"].astype(np.int64)).cuda()
    d_reads = torch.from_numpy(reads).cuda()
    dm.extend(d_reads, torch.from_numpy(lens.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    t = dm.timing()
    assert t["gact_bs_kernel"][1] == 2 and t["gact_kernel"][1] == 0          # extension + stitch, both in the bit-sliced slot
    assert dm.workspace_bytes() > before                                       # the mode's scratch came with its first call
    got = dm.results(n)
    assert np.array_equal(d_reads.cpu().numpy(), oriented)
    _check_against_ref(got, want, got["anchor"])
    # unanchored reads: byte for byte what the classic path gives
    for i in np.flatnonzero(np.array(kinds) == anchored_ref.FALLBACK)[:2000]:
        k = int(classic["n_ops"][i])
        assert got["n_ops"][i] == k and got["score"][i] == classic["score"][i] and _same_meta(classic["meta"][i], got["meta"][i]), i
        assert bytes(got["ops"][i, :k]) == bytes(classic["ops"][i, :k])
    dm.close()
    # a default-mode workspace of the same shape holds exactly what it held before the mode existed to it
    plain = mapper.DeviceMapper(di, n, max_len, gact=GACT, device=gpu)
    assert plain.workspace_bytes() == before
    plain.close()


@pytest.mark.parametrize("impl,gact", [(1, GACT), (3, GACT), (4, GACT), (0, (320, 120, 256)), (0, (128, 32, 32))])
def test_batch_equals_reference_under_every_kernel(ref3, ragged, map_options, impl, gact):
    seqs, hi, di = ref3
    reads, lens, best, oriented, classic, mta = ragged
    pick = np.arange(0, len(lens), 9)
    map_options(di, gact_impl=impl)
    rd = reads[pick].copy()
    got = mapper.extend_batch(di, rd, lens[pick], best[pick], gact, anchored=True)
    assert np.array_equal(rd, oriented[pick])
    want = anchored_ref.extend_batch(hi.content(), mta, oriented[pick], lens[pick], classic["meta"][pick],
                                     classic["meta_r"][pick], gact)
    _check_against_ref(got, want)
    # the option off again: the classic result, byte for byte
    rd = reads[pick].copy()
    off = mapper.extend_batch(di, rd, lens[pick], best[pick], GACT)
    for key in ("n_ops", "score", "meta_r"):
        assert np.array_equal(off[key], classic[key][pick])
    assert _same_meta(off["meta"], classic["meta"][pick])
    for a, i in enumerate(pick):
        assert bytes(off["ops"][a, :off["n_ops"][a]]) == bytes(classic["ops"][i, :classic["n_ops"][i]])


def test_host_paths_and_layouts(ref3):
    seqs, hi, di = ref3
    di.set_map_options()
    r = synth.reads(seqs, 300, 3000, synth.PACBIO_CLR, seed=31)
    lens = r["lens"]
    base = r["reads"].copy()
    rows = mapper.map_batch(di, base, lens, anchored=True)
    assert (rows["meta_r"] == 1).mean() > 0.9
    ra, rb = r["reads"].copy(), r["reads"].copy()
    pa = mapper.map_batch_submit(di, ra, lens, options={"dense_results": 1}, anchored=True)
    pb = mapper.map_batch_submit(di, rb, lens, options={"cigar_text": 1}, anchored=True)
    dense, text = pa.wait(), pb.wait()
    for res, rd in ((dense, ra), (text, rb)):
        assert np.array_equal(rd, base)
        for key in ("best", "n_ops", "score", "meta", "meta_r"):
            assert np.array_equal(res[key], rows[key]), key
    for i in range(len(lens)):
        ops = mapper.ops_of(rows, i)
        assert mapper.ops_of(dense, i) == ops
        assert mapper.text_of(text, i).decode() == (orc.parse_cigar(ops) if rows["meta_r"][i] and rows["score"][i] >= 0 else "*")
    # device path on the same batch
    rd = r["reads"].copy()
    dev = mapper.extend_batch(di, rd, lens, rows["best"], anchored=True)
    for key in ("n_ops", "score", "meta_r"):
        assert np.array_equal(dev[key], rows[key]), key
    assert _same_meta(dev["meta"], rows["meta"])
    # a store too small for the mode is refused, not truncated
    small = np.zeros((len(lens), 2 * int(lens.max()) // 16 * 16), dtype=np.uint8)
    with pytest.raises(capi.LrmError, match="anchored extension: store_stride"):
        mapper.map_batch(di, r["reads"].copy(), lens, store=small, anchored=True)
    with pytest.raises(capi.LrmError, match="anchor_min_len"):
        mapper.map_batch(di, r["reads"].copy(), lens, anchored=True, anchor_min_len=7)


def _rates(seqs, di, r, anchored):
    reads = r["reads"].copy()
    res = mapper.map_batch(di, reads, r["lens"], anchored=anchored)
    ok = (res["meta_r"] == 1) & (res["meta"]["seq_id"] == r["seq"]) & (res["meta"]["strand"] == r["strand"])
    return res, ok


def test_the_point_of_the_feature_pacbio_15k(ref3):
    """2 000 PacBio-CLR reads of 15 kbp: the classic window drifts out of the band, the anchored mode follows the read."""
    seqs, hi, di = ref3
    di.set_map_options()
    r = synth.reads(seqs, 2000, 15_000, synth.PACBIO_CLR, seed=13)
    classic, ok_c = _rates(seqs, di, r, False)
    anch, ok_a = _rates(seqs, di, r, True)
    assert np.array_equal(ok_c, ok_a) and ok_a.mean() > 0.9
    rate_c = classic["score"][ok_c] / r["lens"][ok_c]
    rate_a = anch["score"][ok_a] / r["lens"][ok_a]
    print("PacBio CLR 15 kbp: classic median ED/len %.4f, anchored median %.4f, 95th percentile %.4f" %
          (np.median(rate_c), np.median(rate_a), np.quantile(rate_a, 0.95)))
    assert np.median(rate_a) < np.median(rate_c)
    assert np.median(rate_a) <= 0.19 and np.quantile(rate_a, 0.95) <= 0.22
    pos = anch["meta"]["off"][ok_a].astype(np.int64)                 # SAM POS - 1
    assert (np.abs(pos - r["pos"][ok_a].astype(np.int64)) <= 16).mean() >= 0.99
    worst = max(anchored_ref.edge_indel_runs(mapper.ops_of(anch, i)) for i in np.flatnonzero(ok_a)[:400])
    assert worst <= 50


def test_ont_10k_anchored_is_no_worse(ref3):
    seqs, hi, di = ref3
    di.set_map_options()
    r = synth.reads(seqs, 500, 10_000, synth.ONT, seed=11)
    classic, ok_c = _rates(seqs, di, r, False)
    anch, ok_a = _rates(seqs, di, r, True)
    assert np.median(anch["score"][ok_a]) <= np.median(classic["score"][ok_c])


def test_two_replicas_on_one_device_give_the_same_bytes(ref3, gpu):
    seqs, hi, di = ref3
    di.set_map_options()
    r = synth.reads(seqs, 400, 2500, synth.PACBIO_CLR, seed=17)
    one = mapper.map_batch(di, r["reads"].copy(), r["lens"], anchored=True)
    d2 = index.DeviceIndex.upload_multi(hi, [gpu, gpu])
    try:
        assert d2.replicas == 2
        two = mapper.map_batch(d2, r["reads"].copy(), r["lens"], anchored=True)
        d2.set_map_options(anchored=1)
        two_handle = mapper.map_batch(d2, r["reads"].copy(), r["lens"], store=np.zeros_like(one["ops"]))
    finally:
        d2.close()
    for res in (two, two_handle):
        for key in ("best", "ops", "n_ops", "score", "meta", "meta_r"):
            assert np.array_equal(res[key], one[key]), key
