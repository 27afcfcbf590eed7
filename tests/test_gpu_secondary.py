"""Secondary alignments on the GPU (docs/GACT_SPEC.md, "Secondary alignments"): the rival entries of rival_locus_kernel against
tests/rival_ref.py (the rule in Python on top of the oracle's seed trace); what they must not depend on; the candidate table,
the gathered rows and every per-candidate output against the unchanged extension calls over a batch made of those rows; what
the stage must leave alone; what its results mean on a text with a planted two-copy repeat."""
import numpy as np
import pytest

import mapq_ref
import orc
import rival_ref
import workloads
from longreadmapper_amd import capi, index, mapper, synth
from test_gpu_mapq import SMALL, VARIANTS

pytestmark = pytest.mark.gpu
A0, B0, LN = 20_000, 80_000, 12_000            # the planted repeat of the "meaning" scenario: [A0, A0 + LN) copied to [B0, B0 + LN)


def _entries(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 3)


def _same_entries(got, want, what=""):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())


def _device_entries(di, gpu, reads, lens, seed_len=20, thres=300, min_hits=0, ratio_pct=0):
    """DeviceMapper(..., mapq=True): seed, then lrm_rival_dev -> (entries (n, 3) uint64, mapq records, best)"""
    import torch
    n, stride = reads.shape
    dm = mapper.DeviceMapper(di, n, stride - 1, seed_len, thres, device=gpu, mapq=True)
    try:
        d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
        dm.seed(torch.from_numpy(reads).cuda(), d_lens)
        got = dm.rival(d_lens, n, min_hits, ratio_pct)
        torch.cuda.synchronize()
        res = dm.results(n)
        dm.stats()                                      # raises if the sticky kernel-error word of the workspace is set
        return _entries(got).copy(), res["mapq"].copy(), res["best"].copy()
    finally:
        dm.close()


@pytest.fixture(scope="module")
def scen(gpu):
    cache = {}

    def get(name):
        if name not in cache:
            sc = workloads.scenario(name)
            oi = orc.OracleIndex.from_host_index(sc["hi"])
            want = rival_ref.batch(oi, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])
            cache[name] = (sc, index.DeviceIndex.upload(sc["hi"], gpu, **SMALL), oi, want)
        return cache[name]
    yield get
    for _, di, _, _ in cache.values():
        di.close()


@pytest.mark.parametrize("name", workloads.SEED_SCENARIOS)
def test_entries_equal_the_rule_on_every_seed_scenario(scen, gpu, name):
    sc, di, oi, want = scen(name)
    got, rec, best = _device_entries(di, gpu, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])
    _same_entries(got, want, name)
    cand = want[:, 1] > 0
    assert np.array_equal(np.flatnonzero(cand), rival_ref.plan(rec))
    floor = {"repeats-ties": 30, "repeats-overflow": 20}
    if name in floor:
        assert cand.sum() >= floor[name]
        assert (got[cand, 2] == got[cand, 0] >> np.uint64(4)).all() and (got[cand, 1] >= 1).all() and (got[cand, 1] <= rec["n2"][cand]).all()
        assert (got[cand, 0] != best["key"][cand]).all()
    else:
        assert not cand.any() and not got.any()


@pytest.mark.parametrize("name", ["ont-2k", "repeats-ties"])
def test_entries_do_not_depend_on_the_configuration(scen, gpu, name):
    sc, di, oi, want = scen(name)
    for what, iopt, mopt in VARIANTS:
        dv = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL, **iopt)
        try:
            dv.set_map_options(**mopt)
            got = _device_entries(dv, gpu, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])[0]
            _same_entries(got, want, (name, what))
        finally:
            dv.close()
    # other thresholds: every read with a rival is a candidate, or only the exact ties
    for H, pct in ((1, 1), (8, 100)):
        got = _device_entries(di, gpu, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"], H, pct)[0]
        _same_entries(got, rival_ref.batch(oi, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"], H, pct), (name, H, pct))


@pytest.fixture(scope="module")
def planted(gpu):
    """120 kbp with an exact 12 kbp two-copy repeat, 240 ONT reads of 3 kbp: 35 lie wholly inside a copy."""
    base = synth.reference(120_000, seed=61).copy()
    base[B0:B0 + LN] = base[A0:A0 + LN]
    hi = index.HostIndex.build([base], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    r = synth.reads([base], 240, 3000, synth.ONT, seed=63)
    oi = orc.OracleIndex.from_host_index(hi)
    want = rival_ref.batch(oi, r["reads"], r["lens"])
    yield dict(base=base, hi=hi, di=di, r=r, oi=oi, want=want)
    di.close()


def _where(r):
    pos, end = r["pos"].astype(np.int64), r["pos"].astype(np.int64) + r["span"].astype(np.int64)
    inside = ((pos >= A0) & (end <= A0 + LN)) | ((pos >= B0) & (end <= B0 + LN))
    unique = ((end <= A0) | (pos >= A0 + LN)) & ((end <= B0) | (pos >= B0 + LN))
    other = np.where(pos < B0, pos + (B0 - A0), pos - (B0 - A0))               # the same place of the other copy
    return pos, inside, unique, other


def _resolve(oi, keys, lens):
    """seq_lookup of every key -> (found, off, strand)"""
    out = [orc.seq_lookup(oi.mta(), int(k), int(n)) for k, n in zip(keys, lens)]
    return (np.array([o[0] for o in out]), np.array([o[1][1] for o in out], dtype=np.int64), np.array([o[1][3] for o in out]))


def _two_places_are_the_true_ones(oi, r, best_keys, rival_keys, sel):
    pos, _, _, other = _where(r)
    f1, o1, s1 = _resolve(oi, best_keys[sel], r["lens"][sel])
    f2, o2, s2 = _resolve(oi, rival_keys[sel], r["lens"][sel])
    near = lambda a, b: np.abs(a - b) <= 300
    ok = f1.astype(bool) & f2.astype(bool) & (s1 == r["strand"][sel]) & (s2 == r["strand"][sel])
    ok &= (near(o1, pos[sel]) & near(o2, other[sel])) | (near(o1, other[sel]) & near(o2, pos[sel]))
    return ok


def test_small_pair_table_takes_the_candidates_away_where_the_rule_says(scen, planted, gpu):
    cases = [(scen(nm)[0]["reads"], scen(nm)[0]["lens"], scen(nm)[0]["seed_len"], scen(nm)[0]["thres"], scen(nm)[1], scen(nm)[2])
             for nm in ("repeats-ties", "seed12")]
    cases.append((planted["r"]["reads"], planted["r"]["lens"], 20, 300, planted["di"], planted["oi"]))
    kept = lost = 0
    for reads, lens, seed_len, thres, di, oi in cases:
        full = rival_ref.batch(oi, reads, lens, seed_len, thres)
        want = rival_ref.batch(oi, reads, lens, seed_len, thres, slots=16)
        di.debug_set_mapq_slots(16)
        try:
            got, rec, _ = _device_entries(di, gpu, reads, lens, seed_len, thres)
        finally:
            di.debug_set_mapq_slots(0)
        _same_entries(got, want, "16 slots")
        over = (rec["flags"] & capi.MAPQ_OVERFLOW) != 0
        assert not got[over].any()
        assert np.array_equal(got[~over], full[~over])                   # a read whose pairs fit has the entry of the full table
        kept += int((got[:, 1] > 0).sum())
        lost += int(((full[:, 1] > 0) & over).sum())
    assert kept >= 5 and lost >= 30


def test_long_reads_take_the_wider_sub_buckets(gpu):
    """Reads of 140 kbp (r = 15: sub-buckets of 32 diagonals) inside an exact 150 kbp two-copy repeat, next to reads of up to
    4096 bases (r = 9) on the same text; seed, mapping quality and rival only."""
    base = synth.reference(500_000, seed=81).copy()
    a0, b0, ln = 60_000, 300_000, 150_000
    base[b0:b0 + ln] = base[a0:a0 + ln]
    hi = index.HostIndex.build([base], hlen=10)
    long_r = synth.reads([base[a0:a0 + ln]], 6, 140_000, synth.ONT, seed=83)
    short_r = synth.reads([base[a0:a0 + ln]], 3, 4096, synth.ONT, seed=85)
    lens = np.concatenate([long_r["lens"], np.minimum(short_r["lens"], 4096)]).astype(np.uint32)
    reads = np.zeros((9, int(lens.max()) + 1), dtype=np.uint8)
    for i in range(9):
        src = long_r["reads"][i] if i < 6 else short_r["reads"][i - 6]
        reads[i, :lens[i]] = src[:lens[i]]
    assert sorted({mapq_ref.radius_log2(int(n)) for n in lens}) == [9, 15] and rival_ref.sub_shift(15) == 5
    oi = orc.OracleIndex.from_host_index(hi)
    want = rival_ref.batch(oi, reads, lens)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    try:
        got, rec, best = _device_entries(di, gpu, reads, lens)
    finally:
        di.close()
    _same_entries(got, want, "long reads")
    assert (got[:, 1] > 0).all() and (rec["radius"][:6] == 1 << 15).all() and (rec["radius"][6:] == 512).all()
    # the two places are the two copies
    d = np.abs(got[:, 0].astype(np.int64) - best["key"].astype(np.int64))
    assert (np.abs(d - (b0 - a0)) <= 2000).all()


def test_meaning_of_the_entries_on_a_planted_two_copy_repeat(planted, gpu):
    r, oi = planted["r"], planted["oi"]
    got, rec, best = _device_entries(planted["di"], gpu, r["reads"], r["lens"])
    _same_entries(got, planted["want"], "planted")
    pos, inside, unique, other = _where(r)
    cand = got[:, 1] > 0
    assert inside.sum() == 35 and unique.sum() == 183
    assert cand[inside].all() and not cand[unique].any()
    assert _two_places_are_the_true_ones(oi, r, best["key"], got[:, 0], inside).all()


def test_meaning_of_the_entries_on_a_diverged_copy(gpu):
    """The second copy carries 3 % substitutions: most reads inside a copy still have a rival above half the winner's hits,
    and every candidate's two places are the true ones."""
    base = synth.reference(120_000, seed=61).copy()
    base[B0:B0 + LN] = base[A0:A0 + LN]
    rng = np.random.default_rng(71)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for p in np.flatnonzero(rng.random(LN) < 0.03) + B0:
        base[p] = acgt[(int(np.flatnonzero(acgt == base[p])[0]) + int(rng.integers(1, 4))) % 4]
    hi = index.HostIndex.build([base], hlen=10)
    r = synth.reads([base], 240, 3000, synth.ONT, seed=73)
    oi = orc.OracleIndex.from_host_index(hi)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    try:
        got, rec, best = _device_entries(di, gpu, r["reads"], r["lens"])
    finally:
        di.close()
    _same_entries(got, rival_ref.batch(oi, r["reads"], r["lens"]), "diverged")
    pos, inside, unique, other = _where(r)
    cand = got[:, 1] > 0
    print("diverged copy: %d of %d inside reads are candidates, %d candidates in all" % ((cand & inside).sum(), inside.sum(), cand.sum()))
    assert (cand & inside).sum() >= 30 and not cand[unique].any()
    assert _two_places_are_the_true_ones(oi, r, best["key"], got[:, 0], cand & inside).all()


# ---------------------------------------------------------------------------------------------------------
# the stage: table, rows, extension, flags
# ---------------------------------------------------------------------------------------------------------
MODES = {"classic": {}, "anchored": dict(anchored=True), "clipped": dict(clip=True)}
PER_CANDIDATE = ("n_ops", "score", "meta_r")


def _stage(di, gpu, reads, lens, mode, sec=True, **kw):
    """seed -> extend -> secondary through DeviceMapper -> (primary results before the stage, after it, the reads before, after,
    secondary results, workspace bytes before the stage, after it)"""
    import torch
    n, stride = reads.shape
    dm = mapper.DeviceMapper(di, n, stride - 1, device=gpu, mapq=True, secondary=sec, **MODES[mode], **kw)
    try:
        d_reads, d_lens = torch.from_numpy(reads).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        torch.cuda.synchronize()
        before, reads_before, b0 = dm.results(n), d_reads.cpu().numpy(), dm.workspace_bytes()
        if not sec:
            assert dm.sec is None
            return before, None, reads_before, None, None, b0, b0
        k = dm.secondary(d_reads, d_lens)
        torch.cuda.synchronize()
        out = dm.secondary_results()
        assert len(out["table"]) == k
        dm.stats()
        return before, dm.results(n), reads_before, d_reads.cpu().numpy(), out, b0, dm.workspace_bytes()
    finally:
        dm.close()


def _same_meta(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("loc", "off", "seq_id", "strand"))


def _same_as_the_extension_call(di, gpu, mode, reads, lens, cand, entries, out):
    """Every per-candidate output of a stage result `out` against the unchanged extension call of the mode over a batch made of
    the reads[cand] as sequenced, with best = entries[cand] ((n, 3) uint64 rival entries)."""
    import torch
    k = len(cand)
    rows = np.zeros((k, out["rows"].shape[1]), dtype=np.uint8)
    rows[:, :reads.shape[1]] = reads[cand]
    d2 = mapper.DeviceMapper(di, k, reads.shape[1] - 1, device=gpu, **MODES[mode])
    try:
        d_rows, d_lens = torch.from_numpy(rows).cuda(), torch.from_numpy(lens[cand].astype(np.int32)).cuda()
        d2.best[:k] = torch.from_numpy(entries[cand].view(np.int64)).cuda()
        d2.extend(d_rows, d_lens)
        torch.cuda.synchronize()
        want, rows_after = d2.results(k), d_rows.cpu().numpy()
    finally:
        d2.close()
    for key in PER_CANDIDATE:
        assert np.array_equal(out[key], want[key]), key
    assert _same_meta(out["meta"], want["meta"])
    for s in range(k):
        n_ops = int(want["n_ops"][s])
        assert bytes(out["ops"][s, :n_ops]) == bytes(want["ops"][s, :n_ops]), s
    for name in ("anchor", "clip"):
        if name in want:
            assert out[name].tobytes() == want[name].tobytes(), name
    assert np.array_equal(out["rows"], rows_after)


@pytest.mark.parametrize("mode", list(MODES))
def test_the_stage_launches_the_stages_unchanged(planted, gpu, mode):
    r, di = planted["r"], planted["di"]
    reads, lens = r["reads"], r["lens"].astype(np.uint32)
    prim, _, oriented, _, out, _, _ = _stage(di, gpu, reads, lens, mode)
    cand = np.flatnonzero(planted["want"][:, 1] > 0)
    k = len(cand)
    assert k >= 40 and np.array_equal(out["table"]["read"], cand) and not out["table"]["_pad"].any()
    assert np.array_equal(out["table"]["hits"], planted["want"][cand, 1]) and np.array_equal(out["lens"], lens[cand])
    for f, col in (("key", 0), ("val", 1), ("bucket", 2)):
        assert np.array_equal(out["rival"][f], planted["want"][cand, col]), f
    # the candidate batch as sequenced, through the unchanged extension call of the mode
    mirrored = (prim["meta_r"][cand] != 0) & (prim["meta"]["strand"][cand] == 1)
    assert mirrored.sum() >= 5 and (~mirrored).sum() >= 5 and not np.array_equal(oriented[cand[mirrored]], reads[cand[mirrored]])
    _same_as_the_extension_call(di, gpu, mode, reads, lens, cand, planted["want"], out)
    # the rows are the reads as sequenced -- turned round by THIS extension where the rival resolved to the reverse strand --
    # and every byte behind a row's end is 0
    turned = (out["meta_r"] != 0) & (out["meta"]["strand"] == 1)
    assert turned.any() and (~turned).any()
    for s in range(k):
        n = int(lens[cand[s]])
        orig = bytes(reads[cand[s], :n])
        assert bytes(out["rows"][s, :n]) == (orc.rev_comp(orig) if turned[s] else orig), s
        assert not out["rows"][s, n:].any()
    # flags
    same_place = (prim["meta_r"][cand] != 0) & (out["meta_r"] != 0) & (out["meta"]["seq_id"] == prim["meta"]["seq_id"][cand]) & \
        (out["meta"]["strand"] == prim["meta"]["strand"][cand]) & \
        (np.abs(out["meta"]["off"].astype(np.int64) - prim["meta"]["off"][cand].astype(np.int64)) < lens[cand] // 2)
    reported = (out["meta_r"] != 0) & (out["score"] != -1) & ~same_place
    if mode != "classic":
        reported &= (out["anchor"]["flags"] & capi.ANCHOR_ANCHORED) != 0
    flags = out["table"]["flags"]
    assert np.array_equal((flags & capi.SEC_DUPLICATE) != 0, same_place) and np.array_equal((flags & capi.SEC_ALIGNED) != 0, reported)
    assert not (flags & ~np.uint32(3)).any() and reported.sum() >= 30


def test_meaning_of_the_reported_secondaries(planted, gpu):
    """Anchored with end clipping: the reads inside a copy come out with a reported secondary at the other copy."""
    r = planted["r"]
    prim, _, _, _, out, _, _ = _stage(planted["di"], gpu, r["reads"], r["lens"].astype(np.uint32), "clipped")
    pos, inside, unique, other = _where(r)
    at = {int(read): s for s, read in enumerate(out["table"]["read"])}
    good = 0
    for i in np.flatnonzero(inside):
        s = at[int(i)]
        p_off, s_off = int(prim["meta"]["off"][i]), int(out["meta"]["off"][s])
        there = min(abs(s_off - int(pos[i])), abs(s_off - int(other[i]))) <= 300 and abs(s_off - p_off) > LN       # a true place, not the primary's
        good += bool(out["table"]["flags"][s] & capi.SEC_ALIGNED) and there and out["meta"]["strand"][s] == r["strand"][i]
    print("reported secondaries at the other copy: %d of %d reads inside a copy" % (good, inside.sum()))
    assert good >= 0.9 * inside.sum()
    assert not any(int(i) in at for i in np.flatnonzero(unique))


def test_sam_lines_of_the_reported_secondaries(planted, gpu, tmp_path):
    """The stage's results through lrm_sam_format_secondary: one FLAG 256 line per reported secondary, right behind its read's
    primary line, its fields the records'; the text without those lines is lrm_sam_format_md's byte for byte."""
    import sam_ref
    from longreadmapper_amd import textio
    r = planted["r"]
    reads, lens = r["reads"], r["lens"].astype(np.uint32)
    n = len(lens)
    prim, _, _, _, out, _, _ = _stage(planted["di"], gpu, reads, lens, "clipped")
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for i in range(n):
            f.write(b"@r%d\n" % i + bytes(reads[i, :lens[i]]) + b"\n+\n" + b"I" * int(lens[i]) + b"\n")
    rd = textio.Reader(fq)
    assert rd.next(n) == n
    mta = textio.mta_table([(b"chrP", 0, 120_000)])
    ops = np.ascontiguousarray(prim["ops"])
    score, meta_r = prim["score"].astype(np.int32), prim["meta_r"].astype(np.int32)
    cig = textio.cigar_table(np.uint64(ops.ctypes.data) + np.uint64(ops.strides[0]) * np.arange(n, dtype=np.uint64), prim["n_ops"], score)
    args = (rd.batch, mta, cig, score, prim["meta"], meta_r, n)
    base = textio.sam_format(*args, keep=1, mapq=prim["mapq"], entry="lrm_sam_format_md")
    sec, held = textio.secondary_out(out)
    lines = textio.sam_format(*args, keep=1, mapq=prim["mapq"], secondary=sec).splitlines()
    is_sec = [bool(int(x.split("\t")[1]) & 256) for x in lines]
    assert [x for x, s in zip(lines, is_sec) if not s] == base.splitlines()
    reported = np.flatnonzero(out["table"]["flags"] & capi.SEC_ALIGNED)
    assert sum(is_sec) == len(reported) >= 30
    at = [k for k, s in enumerate(is_sec) if s]
    for k, s in zip(at, reported):
        read = int(out["table"]["read"][s])
        want = ["r%d" % read, str(256 + 16 * int(out["meta"]["strand"][s])), "chrP", str(int(out["meta"]["off"][s]) + 1), "0",
                sam_ref.rle(bytes(out["ops"][s, :int(out["n_ops"][s])])), "*", "0", "0", "*", "*", "ED:I:%d" % out["score"][s], "tp:A:S"]
        assert lines[k].split("\t") == want
        assert lines[k - 1].split("\t")[0] == "r%d" % read and not is_sec[k - 1]
    rd.close()


@pytest.mark.parametrize("opts", [dict(), dict(keep_reads=1), dict(cigar_text=1), dict(cigar_text=1, keep_reads=1), dict(dense_results=1)],
                         ids=["rows", "keep-reads", "cigar-text", "cigar-text-keep-reads", "dense"])
def test_host_buffers_equal_the_device_path(planted, gpu, opts):
    """mapper.secondary_batch over what map_batch(mapq=True) returned, against the device stage, byte for byte."""
    import sam_ref
    r, di = planted["r"], planted["di"]
    reads, lens = r["reads"], r["lens"].astype(np.uint32)
    prim, _, oriented, _, out, _, _ = _stage(di, gpu, reads, lens, "clipped")
    rm = reads.copy()
    res = mapper.map_batch(di, rm, lens, options=dict(opts), clip=True, mapq=True)
    assert np.array_equal(rm, reads if opts.get("keep_reads") else oriented) and not np.array_equal(reads, oriented)
    before = rm.copy()
    sec = mapper.secondary_batch(di, rm, lens, res, options=dict(opts), clip=True)
    assert np.array_equal(rm, before)
    k = len(out["table"])
    assert k >= 40 and len(sec["table"]) == k
    for name in ("table", "rival", "anchor", "clip"):
        assert sec[name].tobytes() == out[name].tobytes(), name
    for name in ("lens", "n_ops", "score", "meta_r"):
        assert np.array_equal(sec[name], out[name]), name
    assert _same_meta(sec["meta"], out["meta"])
    assert np.array_equal(sec["rows"][:k], out["rows"])
    assert ("ops_off" in sec) == bool(opts.get("cigar_text") or opts.get("dense_results")) and bool(sec.get("is_text")) == bool(opts.get("cigar_text"))
    for s in range(k):
        ops = bytes(out["ops"][s, :int(out["n_ops"][s])])
        if opts.get("cigar_text"):
            assert mapper.text_of(sec, s).decode() == (sam_ref.rle(ops) if out["meta_r"][s] and out["score"][s] != -1 else "*"), s
        else:
            assert mapper.ops_of(sec, s) == ops, s
    # room for one candidate fewer: -3 with the count
    with pytest.raises(capi.LrmError, match="room for %d" % (k - 1)) as e:
        mapper.secondary_batch(di, rm, lens, res, options=dict(opts), clip=True, cap=k - 1)
    assert e.value.rc == -3 and e.value.n_sec == k
    if not opts:                                    # a group handle: its first device does the pass
        dg = index.DeviceIndex.upload_multi(planted["hi"], [gpu, gpu], **SMALL)
        try:
            again = mapper.secondary_batch(dg, rm, lens, res, options={}, clip=True)
            assert again["table"].tobytes() == out["table"].tobytes() and np.array_equal(again["score"], out["score"])
        finally:
            dg.close()


def test_accaln_prints_the_secondaries(gpu, tmp_path):
    """FASTQ in, SAM out: the file of lrm_accaln_secondary minus its FLAG 256 lines is lrm_accaln_mapq's byte for byte, and the
    FLAG 256 lines are the reported secondaries of the batches, field for field."""
    import ctypes as C
    from longreadmapper_amd import textio
    from longreadmapper_amd.capi import lib
    base = synth.reference(120_000, seed=61).copy()
    base[B0:B0 + LN] = base[A0:A0 + LN]
    fa = tmp_path / "ref.fa"
    with open(fa, "wb") as f:
        f.write(b">chrP\n")
        b = bytes(base)
        for i in range(0, len(b), 60):
            f.write(b[i:i + 60] + b"\n")
    assert lib.lrm_accidx(str(fa).encode(), 32, 10, 1) == 0
    n = 150
    r = synth.reads([base], n, 1500, synth.ONT, seed=75)
    lens = r["lens"].astype(np.uint32)
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for i in range(n):
            s = bytes(r["reads"][i, :lens[i]])
            f.write(b"@r%d\n" % i + s + b"\n+\n" + bytes(33 + (i + j) % 40 for j in range(len(s))) + b"\n")
    opt = capi.map_options(anchored=1, clip=1)
    so = capi.SecondaryOptions(C.sizeof(capi.SecondaryOptions), 0, 0, 1, 0, 1, 0, 0)
    counts0 = textio.accaln(fa, fq, tmp_path / "mapq.sam", 64, device=gpu, rg_id=7, options=opt, mapq=1)
    counts1 = textio.accaln(fa, fq, tmp_path / "sec.sam", 64, device=gpu, rg_id=7, options=opt, secondary=so)
    plain, got = open(tmp_path / "mapq.sam").read(), open(tmp_path / "sec.sam").read()
    assert counts0 == counts1 and counts0[0] == n
    is_sec = [not x.startswith("@") and bool(int(x.split("\t")[1]) & 256) for x in got.splitlines()]
    assert "\n".join(x for x, s in zip(got.splitlines(), is_sec) if not s) + "\n" == plain
    # the records the batches of 64 give
    hi = index.HostIndex.read(str(fa))
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    want = []
    try:
        for lo in range(0, n, 64):
            bl = lens[lo:lo + 64]
            rows = np.zeros((len(bl), int(bl.max()) + 1), dtype=np.uint8)
            for i, k in enumerate(bl):
                rows[i, :k] = r["reads"][lo + i, :k]
            o = dict(keep_reads=1, cigar_text=1)
            res = mapper.map_batch(di, rows, bl, options=dict(o), clip=True, mapq=True)
            sec = mapper.secondary_batch(di, rows, bl, res, options=dict(o), clip=True)
            for s in np.flatnonzero(sec["table"]["flags"] & capi.SEC_ALIGNED):
                want.append(["r%d" % (lo + int(sec["table"]["read"][s])), str(256 + 16 * int(sec["meta"]["strand"][s])), "chrP",
                             str(int(sec["meta"]["off"][s]) + 1), "0", mapper.text_of(sec, s).decode(), "*", "0", "0", "*", "*",
                             "ED:I:%d" % sec["score"][s], "tp:A:S"])
    finally:
        di.close()
    lines = [x.split("\t") for x, s in zip(got.splitlines(), is_sec) if s]
    assert len(lines) == len(want) > 0 and lines == want
    # so == NULL: lrm_accaln_mapq with its mode on
    total, valid = C.c_uint64(), C.c_uint64()
    capi.check(lib.lrm_accaln_secondary(str(fa).encode(), str(fq).encode(), str(tmp_path / "null.sam").encode(), capi.Params(64, 20, 300),
                                        capi.GactParams(0, 0, 0), gpu, 7, C.byref(total), C.byref(valid), C.byref(opt), None), "lrm_accaln_secondary")
    assert open(tmp_path / "null.sam").read() == plain and (total.value, valid.value) == counts0


def test_nothing_else_moves_and_nothing_is_allocated_without_it(planted, gpu):
    r = planted["r"]
    reads, lens = r["reads"], r["lens"].astype(np.uint32)
    n = len(lens)
    before, after, reads_before, reads_after, out, b0, b1 = _stage(planted["di"], gpu, reads, lens, "clipped")
    assert np.array_equal(reads_before, reads_after)
    for key in before:
        a, b = before[key], after[key]
        assert a.tobytes() == b.tobytes(), key
    assert b1 - b0 == 24 * n + 8 * ((n + 255) // 256) + 8                 # the stage's scratch, allocated by its first call
    off = _stage(planted["di"], gpu, reads, lens, "clipped", sec=False)
    assert off[5] == b0 and np.array_equal(off[2], reads_before)
    for key in before:
        assert off[0][key].tobytes() == before[key].tobytes(), key
    with pytest.raises(capi.LrmError, match="needs mapq"):
        mapper.DeviceMapper(planted["di"], 4, 100, device=gpu, secondary=True)


def test_capacity(planted, gpu):
    import torch
    r = planted["r"]
    reads, lens = r["reads"], r["lens"].astype(np.uint32)
    k = int((planted["want"][:, 1] > 0).sum())
    for cap, ok in ((k - 1, False), (k, True)):
        dm = mapper.DeviceMapper(planted["di"], len(lens), reads.shape[1] - 1, device=gpu, mapq=True, secondary=True, sec_cap=cap)
        try:
            d_reads, d_lens = torch.from_numpy(reads).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
            dm.seed(d_reads, d_lens)
            dm.extend(d_reads, d_lens)
            if ok:
                assert dm.secondary(d_reads, d_lens) == k
                continue
            with pytest.raises(capi.LrmError, match="room for %d" % cap) as e:
                dm.secondary(d_reads, d_lens)
            torch.cuda.synchronize()
            assert e.value.rc == -3 and e.value.n_sec == k and dm.n_sec == 0
            assert not any(bool(t.any()) for t in dm.sec.values())        # no result array was written
        finally:
            dm.close()
