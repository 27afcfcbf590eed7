"""End clipping of the anchored mode (lrm_map_options.clip) on the GPU against tests/clip_ref.py -- the rule of
docs/GACT_SPEC.md, "End clipping", applied to what tests/anchored_ref.py computes -- and what the step is for: read ends
that do not align come out as 'S' columns instead of as a stretch of noise columns."""
import ctypes as C

import numpy as np
import pytest

import anchored_cases
import anchored_ref
import clip_ref
import orc
import sam_ref
from longreadmapper_amd import capi, index, mapper, synth
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu
GACT = (320, 120, 128)
ANCHOR_KEYS = ("text_pos", "read_pos", "len", "delta", "left_ops", "flags")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ref3(gpu):
    seqs = [synth.reference(1_500_000, seed=41, repeat_frac=0.05, rep_len=300, rep_copies=200, rep_div=0.05),
            synth.reference(700_000, seed=42), synth.reference(300_000, seed=43)]
    hi = index.HostIndex.build(seqs, names=["chrA", "chrB", "chrC"], hlen=12)
    di = index.DeviceIndex.upload(hi, gpu)
    yield seqs, hi, di
    di.close()


def _mta(hi):
    return [(o, l) for _, o, l in hi.mta()]


def _random(rng, n):
    return BASES[rng.integers(0, 4, n)]


def _truth_keys(r, mta, rng, jitter=20):
    """best[].key from the truth of synth.reads: the window start on the strand the read came from, jittered."""
    m = len(r["lens"])
    S = np.array([mta[s][0] for s in r["seq"]], dtype=np.int64)
    ls = np.array([mta[s][1] for s in r["seq"]], dtype=np.int64)
    fwd = S + r["pos"].astype(np.int64) + rng.integers(-jitter, jitter + 1, m)
    rev = S + 2 * ls - (r["pos"].astype(np.int64) + r["span"].astype(np.int64)) + rng.integers(-jitter, jitter + 1, m)
    return np.where(r["strand"] == 0, fwd, rev).clip(0).astype(np.uint64)


def _ragged(seqs, mta, seed=5):
    """Lengths 1 .. 6000, both strands; a third of the reads with 50 .. 1500 bases overwritten with random bases at one or
    both ends; random reads (mapped, never anchored) and loci that resolve to nothing among them."""
    rng = np.random.default_rng(seed)
    parts = []
    for k, (length, cnt) in enumerate(((1, 4), (11, 6), (19, 6), (37, 40), (150, 300), (400, 300), (900, 200), (2100, 120),
                                       (4200, 60), (6000, 40))):
        r = synth.reads(seqs, cnt, length, synth.PACBIO_CLR if k % 2 else synth.ONT, seed=seed + k)
        parts.append((r, _truth_keys(r, mta, rng)))
    stride = max(r["reads"].shape[1] for r, _ in parts)
    n = sum(len(r["lens"]) for r, _ in parts)
    reads, lens, best = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=mapper.ENTRY_DT)
    at = 0
    for r, keys in parts:
        m = len(r["lens"])
        reads[at:at + m, :r["reads"].shape[1]], lens[at:at + m], best["key"][at:at + m] = r["reads"], r["lens"], keys
        at += m
    junk = np.zeros((n, 2), dtype=np.int64)
    for i in range(0, n, 3):
        ln = int(lens[i])
        head = int(rng.integers(50, 1501)) if i % 2 == 0 or i % 9 == 0 else 0
        tail = int(rng.integers(50, 1501)) if i % 2 == 1 or i % 9 == 0 else 0
        head, tail = min(head, ln // 3), min(tail, ln // 3)
        reads[i, :head] = _random(rng, head)
        reads[i, ln - tail:ln] = _random(rng, tail)
        junk[i] = head, tail
    for i in range(1, n, 16):
        reads[i, :lens[i]] = _random(rng, int(lens[i]))
    for i in range(7, n, 101):
        best["key"][i] = mta[0][0] + mta[0][1] - 5
    return reads, lens, best, junk


@pytest.fixture(scope="module")
def ragged(ref3):
    seqs, hi, di = ref3
    mta = _mta(hi)
    reads, lens, best, junk = _ragged(seqs, mta)
    di.set_map_options()
    oriented = reads.copy()
    classic = mapper.extend_batch(di, oriented, lens, best, GACT)
    return reads, lens, best, oriented, classic, mta


def _same_meta(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("loc", "off", "seq_id", "strand"))


def _check(got, want, anchors=None, clip=None):
    bad = []
    for i, w in enumerate(want):
        if w is None:
            ok = got["meta_r"][i] == 0 and got["score"][i] == -1 and got["n_ops"][i] == 0
            if ok and clip is not None:
                ok = clip["left"][i] == 0 and clip["right"][i] == 0 and anchors["flags"][i] == 0
        else:
            k = w["n_ops"]
            ok = (got["meta_r"][i] == 1 and got["n_ops"][i] == k and got["score"][i] == w["score"] and
                  bytes(got["ops"][i, :k]) == w["ops"] and int(got["meta"]["loc"][i]) == w["loc"] and
                  int(got["meta"]["off"][i]) == w["off"])
            if ok and anchors is not None:
                ok = all(int(anchors[key][i]) == w[key] for key in ANCHOR_KEYS)
            if ok and clip is not None:
                ok = int(clip["left"][i]) == w.get("clip_left", 0) and int(clip["right"][i]) == w.get("clip_right", 0)
        if not ok:
            bad.append(i)
    assert not bad, (len(bad), bad[:5])


def _device_run(di, gpu, reads, lens, best, gact=GACT, **kw):
    import torch
    n, max_len = len(lens), int(lens.max())
    dm = mapper.DeviceMapper(di, n, max_len, gact=gact, device=gpu, **kw)
    dm.best[:, 0] = torch.from_numpy(best["key"].astype(np.int64)).cuda()
    d_reads = torch.from_numpy(reads).cuda()
    dm.extend(d_reads, torch.from_numpy(lens.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    res = dm.results(n)
    res["workspace_bytes"] = dm.workspace_bytes()
    dm.close()
    return res, d_reads.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl,gact", [(1, GACT), (3, GACT), (4, GACT), (0, (320, 120, 256))])
def test_clipped_batch_equals_reference(ref3, ragged, map_options, gpu, impl, gact):
    seqs, hi, di = ref3
    reads, lens, best, oriented, classic, mta = ragged
    map_options(di, gact_impl=impl)
    base = anchored_ref.extend_batch(hi.content(), mta, oriented, lens, classic["meta"], classic["meta_r"], gact)
    kinds = [b["flags"] if b else 0 for b in base]
    assert sum(k == anchored_ref.FALLBACK for k in kinds) > 50 and sum(k == 0 for k in kinds) > 5
    for P, B in ((0, 0), (1, 1), (5, 40)):
        want = [None if b is None else clip_ref.apply_clip(b, int(lens[i]), P, B) for i, b in enumerate(base)]
        rd = reads.copy()
        got = mapper.extend_batch(di, rd, lens, best, gact, clip=True, clip_penalty=P, clip_end_bonus=B)
        assert np.array_equal(rd, oriented)
        _check(got, want)
        dev, rd = _device_run(di, gpu, reads, lens, best, gact, clip=True, clip_penalty=P, clip_end_bonus=B)
        assert np.array_equal(rd, oriented)
        _check(dev, want, dev["anchor"], dev["clip"])
    cl = np.array([w["clip_left"] if w else 0 for w in want])
    cr = np.array([w["clip_right"] if w else 0 for w in want])
    assert (cl > 0).sum() > 100 and (cr > 0).sum() > 100 and ((cl > 0) & (cr > 0)).sum() > 20
    # unanchored reads are left exactly as the mode leaves them
    for i in np.flatnonzero(np.array(kinds) == anchored_ref.FALLBACK):
        assert want[i]["ops"] == base[i]["ops"] and b"S" not in want[i]["ops"]


def test_off_means_off(ref3, ragged, gpu):
    seqs, hi, di = ref3
    reads, lens, best, oriented, classic, mta = ragged
    di.set_map_options()
    want = anchored_ref.extend_batch(hi.content(), mta, oriented, lens, classic["meta"], classic["meta_r"], GACT)
    rd = reads.copy()
    _check(mapper.extend_batch(di, rd, lens, best, GACT, anchored=True, clip=False), want)
    # the anchored entry point never clips, whatever the handle's options say; its workspace holds no clip records
    plain, _ = _device_run(di, gpu, reads, lens, best, anchored=True)
    with di.map_options_plus(anchored=1, clip=1):
        dev, _ = _device_run(di, gpu, reads, lens, best, anchored=True)
    _check(dev, want, dev["anchor"])
    assert "clip" not in dev and dev["workspace_bytes"] == plain["workspace_bytes"]
    clipped, _ = _device_run(di, gpu, reads, lens, best, clip=True)
    assert clipped["workspace_bytes"] == plain["workspace_bytes"] + 2 * len(lens) * 16
    # the classic mode with the handle's options back: what it was
    rd = reads.copy()
    off = mapper.extend_batch(di, rd, lens, best, GACT)
    for key in ("n_ops", "score", "meta_r", "ops"):
        assert np.array_equal(off[key], classic[key]), key
    # clip without anchored, and parameters out of range, are refused
    small = reads[:64].copy()
    with pytest.raises(capi.LrmError, match="clip needs lrm_map_options.anchored"):
        mapper.map_batch(di, small, lens[:64], options={"clip": 1})
    with pytest.raises(capi.LrmError, match="clip needs lrm_map_options.anchored"):
        with di.map_options_plus(clip=1):
            mapper._extend_batch(di, small, lens[:64], best[:64], GACT, True)
    with pytest.raises(capi.LrmError, match="clip_penalty"):
        mapper.map_batch(di, small, lens[:64], clip=True, clip_penalty=16)
    with pytest.raises(capi.LrmError, match="clip_end_bonus"):
        mapper.map_batch(di, small, lens[:64], clip=True, clip_end_bonus=256)


# ---------------------------------------------------------------------------------------------------------
# layouts and paths
# ---------------------------------------------------------------------------------------------------------
def _with_junk(rng, r, head, tail):
    """synth.reads result with `head` / `tail` random bases around every ORIENTED read -> reads (n, stride), lens."""
    n = len(r["lens"])
    stride = r["reads"].shape[1] + head + tail
    out = np.zeros((n, stride), dtype=np.uint8)
    lens = r["lens"].astype(np.uint32) + head + tail
    for i in range(n):
        a, b = (head, tail) if r["strand"][i] == 0 else (tail, head)
        ln = int(r["lens"][i])
        out[i, :a], out[i, a:a + ln], out[i, a + ln:a + ln + b] = _random(rng, a), r["reads"][i, :ln], _random(rng, b)
    return out, lens


def test_layouts_paths_and_replicas(ref3, gpu):
    seqs, hi, di = ref3
    di.set_map_options()
    rng = np.random.default_rng(23)
    r = synth.reads(seqs, 300, 2500, synth.PACBIO_CLR, seed=31)
    reads, lens = _with_junk(rng, r, 120, 333)
    base = reads.copy()
    rows = mapper.map_batch(di, base, lens, clip=True)
    assert (rows["meta_r"] == 1).mean() > 0.9
    ra, rb = reads.copy(), reads.copy()
    dense = mapper.map_batch_submit(di, ra, lens, options={"dense_results": 1}, clip=True).wait()
    text = mapper.map_batch_submit(di, rb, lens, options={"cigar_text": 1}, clip=True).wait()
    for res, rd in ((dense, ra), (text, rb)):
        assert np.array_equal(rd, base)
        for key in ("best", "n_ops", "score", "meta", "meta_r"):
            assert np.array_equal(res[key], rows[key]), key
    soft = 0
    for i in range(len(lens)):
        ops = mapper.ops_of(rows, i)
        assert mapper.ops_of(dense, i) == ops
        t = mapper.text_of(text, i).decode()
        assert t == (orc.parse_cigar(ops) if rows["meta_r"][i] and rows["score"][i] >= 0 else "*")
        cl, cr = len(ops) - len(ops.lstrip(b"S")), len(ops) - len(ops.rstrip(b"S"))
        assert t.startswith("%dS" % cl) == (cl > 0) and t.endswith("%dS" % cr) == (cr > 0)
        soft += cl > 0 and cr > 0
    assert soft > 200
    dev, _ = _device_run(di, gpu, reads, lens, rows["best"], clip=True)
    for key in ("n_ops", "score", "meta_r"):
        assert np.array_equal(dev[key], rows[key]), key
    assert _same_meta(dev["meta"], rows["meta"])
    for i in range(len(lens)):
        k = int(rows["n_ops"][i])
        assert bytes(dev["ops"][i, :k]) == mapper.ops_of(rows, i)
        assert dev["ops"][i, :dev["clip"]["left"][i]].tobytes() == b"S" * int(dev["clip"]["left"][i])
    d2 = index.DeviceIndex.upload_multi(hi, [gpu, gpu])
    try:
        two = mapper.map_batch(d2, reads.copy(), lens, clip=True)
        d2.set_map_options(anchored=1, clip=1)
        two_handle = mapper.map_batch(d2, reads.copy(), lens, store=np.zeros_like(rows["ops"]))
    finally:
        d2.close()
    for res in (two, two_handle):
        for key in ("best", "ops", "n_ops", "score", "meta", "meta_r"):
            assert np.array_equal(res[key], rows[key]), key


def test_accaln_prints_soft_clips(gpu, tmp_path):
    seqs = [synth.reference(110_000, seed=41), synth.reference(50_000, seed=42)]
    fa = tmp_path / "ref.fa"
    with open(fa, "wb") as f:
        for nm, s in zip((b"chrA", b"chrB"), seqs):
            f.write(b">" + nm + b"\n" + bytes(s) + b"\n")
    assert lib.lrm_accidx(str(fa).encode(), 32, 10, 1) == 0
    hi = index.HostIndex.read(str(fa))
    mta = hi.mta()
    rng = np.random.default_rng(3)
    r = synth.reads(seqs, 120, 1500, synth.ONT, seed=9)
    reads, lens = _with_junk(rng, r, 90, 210)
    recs = [(b"q%d" % i, bytes(reads[i, :lens[i]]), bytes(33 + (i + j) % 40 for j in range(int(lens[i])))) for i in range(len(lens))]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@" + nm + b"\n" + s + b"\n+\n" + q + b"\n" for nm, s, q in recs))
    sam = tmp_path / "out.sam"
    total, valid = C.c_uint64(), C.c_uint64()
    opt = capi.map_options(anchored=1, clip=1)
    capi.check(lib.lrm_accaln_opt(str(fa).encode(), str(fq).encode(), str(sam).encode(), capi.Params(512, 20, 300),
                                  capi.GactParams(*GACT), gpu, 77, C.byref(total), C.byref(valid), C.byref(opt)), "lrm_accaln_opt")
    di = index.DeviceIndex.upload(hi, gpu)
    try:
        res = mapper.map_batch(di, reads, lens, clip=True)                     # (reverse-strand reads come back oriented: SEQ)
    finally:
        di.close()
    want = sam_ref.header(mta, 77)
    for i, (nm, s, q) in enumerate(recs):
        want += sam_ref.record(nm.decode(), bytes(reads[i, :lens[i]]).decode(), q.decode(), mta, mapper.ops_of(res, i), int(res["score"][i]),
                               int(res["meta_r"][i]), int(res["meta"]["seq_id"][i]), int(res["meta"]["off"][i]),
                               int(res["meta"]["strand"][i]))
    got = open(sam).read()
    assert got == want
    cig = [ln.split("\t")[5] for ln in got.splitlines() if ln[0] != "@"]
    assert sum(c.endswith("S") and c.split("S")[0].isdigit() for c in cig) > 80          # <cl>S ... <cr>S
    assert total.value == len(lens)
    # SEQ stays the whole read: a soft clip
    assert all(len(ln.split("\t")[9]) == int(lens[i]) for i, ln in enumerate(l for l in got.splitlines() if l[0] != "@"))


# ---------------------------------------------------------------------------------------------------------
# the seam: 'S' | reversed left | right | 'S' at every alignment of the 16-byte groups
# ---------------------------------------------------------------------------------------------------------
def test_every_residue_of_the_three_seams(ref3, gpu):
    seqs, hi, di = ref3
    di.set_map_options()
    mta, text = _mta(hi), hi.content()
    rng = np.random.default_rng(8)
    S, ls = mta[1]
    combos = [(x, 0, 0) for x in range(16)] + [(0, y, 0) for y in range(16)] + [(0, 0, z) for z in range(16)]
    combos += [tuple(int(v) for v in rng.integers(0, 16, 3)) for _ in range(150)]
    rows = []
    for k, (x, y, z) in enumerate(combos):
        cl, g1, g2, cr = 40 + x, 30 + y, 60 + z, 50 + (k % 7)
        n, start = cl + g1 + 1 + g2 + cr, 5000 + 997 * k
        face = seqs[1][start:start + n]
        read = face.copy()
        read[:cl] = anchored_cases.noise(rng, cl, face[:cl])
        read[cl + g1] = anchored_cases.noise(rng, 1, face[cl + g1:cl + g1 + 1])[0]
        read[n - cr:] = anchored_cases.noise(rng, cr, face[n - cr:])
        rows.append((read, S + start + int(rng.integers(-5, 6))))
    n = len(rows)
    lens = np.array([len(r) for r, _ in rows], dtype=np.uint32)
    reads = np.zeros((n, int(lens.max()) + 1), dtype=np.uint8)
    best = np.zeros(n, dtype=mapper.ENTRY_DT)
    for i, (r, L) in enumerate(rows):
        reads[i, :len(r)], best["key"][i] = r, L
    want = [clip_ref.extend_clipped(reads[i, :lens[i]], text, int(best["key"][i]), S, ls, GACT) for i in range(n)]
    seen = [set(), set(), set()]
    for w in want:
        b0, b1 = w["clip_left"], w["left_ops"]
        b2 = w["n_ops"] - w["clip_right"]
        assert 0 < b0 < b1 < b2 < w["n_ops"]
        for s, v in zip(seen, (b0, b1, b2)):
            s.add(v % 16)
    assert all(len(s) == 16 for s in seen), [sorted(s) for s in seen]
    for impl in (3, 4):
        di.set_map_options(gact_impl=impl)
        dev, _ = _device_run(di, gpu, reads, lens, best, clip=True)
        _check(dev, want, dev["anchor"], dev["clip"])
    di.set_map_options()


# ---------------------------------------------------------------------------------------------------------
# the point of the feature
# ---------------------------------------------------------------------------------------------------------
def _placed(res, r):
    return (res["meta_r"] == 1) & (res["meta"]["seq_id"] == r["seq"]) & (res["meta"]["strand"] == r["strand"])


def _soft_ends(res, i):
    ops = mapper.ops_of(res, i)
    return len(ops) - len(ops.lstrip(b"S")), len(ops) - len(ops.rstrip(b"S")), ops


def test_junk_ends_are_clipped_ont_10k(ref3):
    seqs, hi, di = ref3
    di.set_map_options()
    rng = np.random.default_rng(12)
    r = synth.reads(seqs, 1000, 10_000, synth.ONT, seed=11)
    reads, lens = _with_junk(rng, r, 300, 600)
    plain = mapper.map_batch(di, reads.copy(), lens, anchored=True)
    clip = mapper.map_batch(di, reads.copy(), lens, clip=True)
    ok = _placed(clip, r)
    assert np.array_equal(ok, _placed(plain, r)) and ok.mean() > 0.9
    idx = np.flatnonzero(ok)
    ends = np.array([_soft_ends(clip, i)[:2] for i in idx])
    aligned = lens[idx] - ends.sum(axis=1)
    good = (np.abs(ends[:, 0] - 300) <= 40) & (np.abs(ends[:, 1] - 600) <= 40)
    rate_c, rate_p = clip["score"][idx] / aligned, plain["score"][idx] / lens[idx]
    pos_err = np.abs(clip["meta"]["off"][idx].astype(np.int64) - r["pos"][idx].astype(np.int64))
    # the noise rate the defaults rest on: columns other than '=' inside the junk, without clipping
    noise = []
    for i in idx[:300]:
        ops = mapper.ops_of(plain, i)
        q = np.cumsum(np.frombuffer(ops, dtype=np.uint8) != ord("D"))          # query bases consumed through each column
        tail = ops[int(np.searchsorted(q, int(lens[i]) - 500)):]                # the columns of the last 500 read bases
        noise.append(1 - tail.count(b"=") / max(len(tail), 1))
    print("junk 300 + 600 around ONT 10 kbp: %d placed; both ends within 40: %.3f; median ED/aligned %.4f clipped, %.4f "
          "unclipped; POS within 40: %.3f; non-'=' columns inside the junk (unclipped): median %.3f, min %.3f" %
          (len(idx), good.mean(), np.median(rate_c), np.median(rate_p), (pos_err <= 40).mean(), np.median(noise), np.min(noise)))
    assert good.mean() >= 0.95
    assert np.median(rate_c) <= 0.10 and np.median(rate_p) > 0.125            # measured: 0.095 against 0.132
    assert (pos_err <= 40).mean() >= 0.95
    # '=' +1 against -2: junk loses as long as more than a third of its columns is not '=' (measured: median 0.45, min 0.43)
    assert np.median(noise) > 0.40 and np.min(noise) > 1 / 3


@pytest.mark.parametrize("profile,length,seed", [(synth.ONT, 10_000, 11), (synth.PACBIO_CLR, 15_000, 13)], ids=["ont", "pacbio"])
def test_untouched_reads_keep_their_ends(ref3, profile, length, seed):
    seqs, hi, di = ref3
    di.set_map_options()
    r = synth.reads(seqs, 500, length, profile, seed=seed)
    plain = mapper.map_batch(di, r["reads"].copy(), r["lens"], anchored=True)
    clip = mapper.map_batch(di, r["reads"].copy(), r["lens"], clip=True)
    idx = np.flatnonzero(_placed(clip, r))
    total = np.array([sum(_soft_ends(clip, i)[:2]) for i in idx])
    med_c, med_p = np.median(clip["score"][idx]), np.median(plain["score"][idx])
    print("untouched reads: %d placed, clipped >= 30 bases in total: %.4f, largest %d, median score %.0f against %.0f" %
          (len(idx), (total >= 30).mean(), total.max(), med_c, med_p))
    assert len(idx) > 400 and (total < 30).mean() >= 0.99
    assert abs(med_c - med_p) <= 0.01 * med_p


def test_chimeras_keep_one_part(ref3):
    seqs, hi, di = ref3
    di.set_map_options()
    a = synth.reads(seqs, 300, 6000, synth.ONT, seed=51)
    b = synth.reads(seqs, 300, 4000, synth.ONT, seed=52)
    n = 300
    lens = (a["lens"] + b["lens"]).astype(np.uint32)
    reads = np.zeros((n, int(lens.max()) + 1), dtype=np.uint8)
    for i in range(n):
        la, lb = int(a["lens"][i]), int(b["lens"][i])
        reads[i, :la], reads[i, la:la + lb] = a["reads"][i, :la], b["reads"][i, :lb]
    res = mapper.map_batch(di, reads.copy(), lens, clip=True)
    on_a, on_b = _placed(res, a), _placed(res, b)
    good = 0
    for i in range(n):
        cl, cr, _ = _soft_ends(res, i)
        if on_a[i]:                      # the other part follows the kept one in the read as sequenced
            other, got = int(b["lens"][i]), (cr if a["strand"][i] == 0 else cl)
        elif on_b[i]:
            other, got = int(a["lens"][i]), (cl if b["strand"][i] == 0 else cr)
        else:
            continue
        good += abs(got - other) <= 60
    print("chimeras 6 kbp + 4 kbp: placed on the first part %d, on the second %d, other part clipped to within 60: %d of %d" %
          (on_a.sum(), on_b.sum(), good, n))
    assert (on_a | on_b).mean() >= 0.95 and good >= 0.9 * n


def test_overhang_at_the_sequence_end_is_soft_clipped(ref3, gpu):
    """A window may not cross the end of its sequence (locus_resolve), and the anchor lies within 32 diagonals of the
    window: the largest overhang that still anchors is 31 bases.  It comes out as 'S', not as a run of 'I'."""
    seqs, hi, di = ref3
    di.set_map_options()
    mta = _mta(hi)
    S, ls = mta[2]
    rng = np.random.default_rng(6)
    n, ln = 64, 700
    reads = np.zeros((n, ln + 1), dtype=np.uint8)
    best = np.zeros(n, dtype=mapper.ENTRY_DT)
    over = np.array([8 + k % 24 for k in range(n)])
    for k in range(n):
        h = int(over[k])
        fwd = np.concatenate([seqs[2][ls - (ln - h):], _random(rng, h)])
        fwd[11:ln - h - 40:41] = BASES[(np.searchsorted(BASES, fwd[11:ln - h - 40:41]) + 1) % 4]
        reads[k, :ln], best["key"][k] = fwd, S + ls - ln                       # the last window of the sequence
    lens = np.full(n, ln, dtype=np.uint32)
    plain, _ = _device_run(di, gpu, reads, lens, best, anchored=True)
    clip, _ = _device_run(di, gpu, reads, lens, best, clip=True)
    assert (clip["meta_r"] == 1).all()
    flags = clip["anchor"]["flags"]
    assert ((flags & capi.ANCHOR_ANCHORED) != 0).all() and ((flags & capi.ANCHOR_RIGHT_CLIPPED) != 0).all()
    assert ((flags & capi.ANCHOR_SOFT_RIGHT) != 0).all()
    err = np.abs(clip["clip"]["right"].astype(np.int64) - over)
    runs = [len(o) - len(o.rstrip(b"I")) for o in (bytes(plain["ops"][i, :plain["n_ops"][i]]) for i in range(n))]
    print("overhang 8 .. 31 at the end of chrC: trailing 'S' off by at most %d; unclipped trailing 'I' runs %d .. %d" %
          (err.max(), min(runs), max(runs)))
    assert err.max() <= 4 and min(runs) >= 4
    for i in range(n):
        aligned = bytes(clip["ops"][i, :clip["n_ops"][i]]).rstrip(b"S")
        assert aligned.endswith(b"=") and int(clip["meta"]["off"][i]) + len(aligned) - aligned.count(b"I") <= ls
