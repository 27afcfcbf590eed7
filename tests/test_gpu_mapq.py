"""Mapping quality on the GPU (docs/GACT_SPEC.md, "Mapping quality"): the lrm_mapq records of mapq_vote_kernel, every field,
against tests/mapq_ref.py (the rule in Python on top of the oracle's seed trace); what the records must not depend on;
what the other outputs must not notice; what the numbers mean on a text with a planted two-copy repeat; the SAM flow."""
import ctypes as C

import numpy as np
import pytest

import mapq_ref
import orc
import workloads
from longreadmapper_amd import capi, index, mapper, synth
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu
FIELDS = ("n1", "n2", "radius", "mapq", "phase", "flags")


def _same_records(got, want, what=""):
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, bad[:8].tolist(), [tuple(int(got[i][g]) for g in FIELDS) for i in bad[:3]],
                               [tuple(int(want[i][g]) for g in FIELDS) for i in bad[:3]])
    assert not got["_pad"].any()


def _device_records(di, gpu, reads, lens, seed_len=20, thres=300):
    """DeviceMapper(..., mapq=True).seed -> (records, best, workspace bytes before the call, after it, stats)"""
    import torch
    n, stride = reads.shape
    dm = mapper.DeviceMapper(di, n, stride - 1, seed_len, thres, device=gpu, mapq=True)
    before = dm.workspace_bytes()
    dm.seed(torch.from_numpy(reads).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    res = dm.results(n)
    st = dm.stats()                                     # raises if the sticky kernel-error word of the workspace is set
    after = dm.workspace_bytes()
    dm.close()
    return res["mapq"].copy(), res["best"].copy(), before, after, st


SMALL = dict(lc_long_max=13)       # every handle of this module stays small: the automatic long seed table takes what HBM is free


@pytest.fixture(scope="module")
def scen(gpu):
    cache = {}

    def get(name):
        if name not in cache:
            sc = workloads.scenario(name)
            cache[name] = (sc, index.DeviceIndex.upload(sc["hi"], gpu, **SMALL), orc.OracleIndex.from_host_index(sc["hi"]))
        return cache[name]
    yield get
    for _, di, _ in cache.values():
        di.close()


@pytest.mark.parametrize("name", workloads.SEED_SCENARIOS)
def test_records_equal_the_rule_on_every_seed_scenario(scen, gpu, name):
    sc, di, oi = scen(name)
    want, pairs = mapq_ref.batch(oi, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])
    got, best, before, after, _ = _device_records(di, gpu, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])
    want_best, phases = oi.seed_batch(sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])
    for f in ("key", "val", "bucket"):
        assert np.array_equal(best[f], want_best[f])
    _same_records(got, want, name)
    assert np.array_equal(got["phase"][best["val"] > 0], (phases - 1)[best["val"] > 0])
    assert after - before == len(sc["lens"])            # one byte per read: the deciding phase
    assert not (got["flags"] & capi.MAPQ_OVERFLOW).any() and pairs.max() <= capi.MAPQ_SLOTS
    zero = best["val"] == 0
    assert not any(got[f][zero].any() for f in FIELDS) and (got["n1"][~zero] >= 1).all()
    if name == "clean-1k":
        assert (got["phase"] == 0).mean() > 0.5 and (got["mapq"] >= 50).mean() > 0.9
    if name == "ont-2k":
        assert (got["phase"] == 20).all()
    if name in ("repeats-ties", "repeats-overflow"):
        assert (got["mapq"] == 0).sum() >= 4 and got["n2"].max() > 20
    if name == "ragged":
        assert zero.sum() >= 3


@pytest.fixture(scope="module")
def planted(gpu):
    """2 Mbp with planted repeat families, ONT-like reads of ragged lengths up to 20 kbp."""
    seqs = [synth.reference(1_400_000, seed=51, repeat_frac=0.06, rep_len=400, rep_copies=150, rep_div=0.03),
            synth.reference(600_000, seed=52)]
    hi = index.HostIndex.build(seqs, hlen=12)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    n = 2400
    r = synth.reads(seqs, n, 20_000, synth.ONT, seed=53)
    rng = np.random.default_rng(54)
    new_lens = np.minimum(r["lens"], rng.integers(200, 20_001, n)).astype(np.uint32)
    new_lens[::97] = rng.integers(0, 60, len(new_lens[::97]))
    reads, lens = workloads.ragged(r["reads"], r["lens"], new_lens)
    yield hi, di, reads, lens
    di.close()


def test_large_ont_batch_over_planted_repeats(planted, gpu):
    hi, di, reads, lens = planted
    oi = orc.OracleIndex.from_host_index(hi)
    want, pairs = mapq_ref.batch(oi, reads, lens)
    got, best, _, _, _ = _device_records(di, gpu, reads, lens)
    _same_records(got, want, "planted")
    assert len({int(x) for x in got["radius"]}) >= 4 and got["radius"].max() == 4096      # 512 .. 4096: reads up to 20 kbp
    assert (got["mapq"] >= 50).sum() > 1500 and (got["n2"] > 5).sum() > 500 and pairs.max() > 300
    # the same records from the host boundary, several seed sub-batches and slices
    rm = reads.copy()
    res = mapper.map_batch(di, rm, lens, options=dict(slice_reads=1000, sub_batches=3), mapq=True)
    _same_records(res["mapq"], want, "planted, host buffers")


VARIANTS = [("rounds-1", {}, dict(seed_rounds=1)), ("rounds-2", {}, dict(seed_rounds=2)), ("exact-vote", {}, dict(vote_exact_only=1)),
            ("seed-table", dict(seed_table=1), {}), ("no-seed-table", dict(seed_table=0), {}), ("sa-sampled-4", dict(sa_sampled=4), {}),
            ("sa-sampled-4-table", dict(sa_sampled=4, seed_table=1), dict(seed_rounds=1))]


@pytest.mark.parametrize("name", ["clean-1k", "ont-2k", "repeats-ties"])
def test_records_do_not_depend_on_the_configuration(scen, gpu, name):
    sc, di, oi = scen(name)
    want, _ = mapq_ref.batch(oi, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])
    for what, iopt, mopt in VARIANTS:
        dv = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL, **iopt)
        try:
            if "seed_table" in iopt:                    # the seed table really is there / really is not
                assert dv.tables()["seed_table_len"] == (20 if iopt["seed_table"] else 0)
            dv.set_map_options(**mopt)
            got = _device_records(dv, gpu, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])[0]
            _same_records(got, want, (name, what, "device"))
            rm = sc["reads"].copy()
            res = mapper.map_batch(dv, rm, sc["lens"], sc["seed_len"], sc["thres"], options=dict(sub_batches=3, **mopt), mapq=True)
            _same_records(res["mapq"], want, (name, what, "host"))
        finally:
            dv.close()
    # a group handle of two replicas: every share written in place
    dg = index.DeviceIndex.upload_multi(sc["hi"], [gpu, gpu], **SMALL)
    try:
        rm = sc["reads"].copy()
        res = mapper.map_batch(dg, rm, sc["lens"], sc["seed_len"], sc["thres"], mapq=True)
        _same_records(res["mapq"], want, (name, "group of two"))
    finally:
        dg.close()


@pytest.mark.parametrize("name", ["ont-2k", "clean-1k"])
def test_every_other_output_is_the_same_and_nothing_is_allocated_without_it(scen, gpu, name):
    import torch
    sc, di, oi = scen(name)
    ra, rb = sc["reads"].copy(), sc["reads"].copy()
    off = mapper.map_batch(di, ra, sc["lens"], sc["seed_len"], sc["thres"], options=dict(sub_batches=2))
    on = mapper.map_batch(di, rb, sc["lens"], sc["seed_len"], sc["thres"], options=dict(sub_batches=2), mapq=True)
    assert "mapq" not in off and on["mapq"].dtype == mapper.MAPQ_DT
    for k in ("best", "ops", "n_ops", "score", "meta_r"):
        assert np.array_equal(on[k], off[k]), k
    assert all(np.array_equal(on["meta"][f], off["meta"][f]) for f in ("loc", "off", "seq_id", "strand")) and np.array_equal(ra, rb)
    # lrm_map_batch_submit_mapq(NULL) is lrm_map_batch_submit; lrm_seed_batch_mapq_dev(NULL) is lrm_seed_batch_dev
    n, stride = sc["reads"].shape
    d_reads, d_lens = torch.from_numpy(sc["reads"]).cuda(), torch.from_numpy(sc["lens"].astype(np.int32)).cuda()
    dm = mapper.DeviceMapper(di, n, stride - 1, sc["seed_len"], sc["thres"], device=gpu)
    b0 = dm.workspace_bytes()
    dm.seed(d_reads, d_lens)
    p = capi.Params(n, sc["seed_len"], sc["thres"])
    best2 = torch.zeros((n, 3), dtype=torch.int64, device=dm.dev)
    capi.check(lib.lrm_seed_batch_mapq_dev(di.handle, dm.ws, d_reads.data_ptr(), d_reads.stride(0), d_lens.data_ptr(), n, stride - 1, p,
                                           best2.data_ptr(), None, dm._stream()), "lrm_seed_batch_mapq_dev")
    torch.cuda.synchronize()
    assert dm.workspace_bytes() == b0 and torch.equal(best2, dm.best[:n])
    assert np.array_equal(dm.results(n)["best"], on["best"])
    dm.close()
    flag, mq, valid = mapper.result_flags(on["score"], on["meta_r"], on["meta"], mapq=on["mapq"])
    mapped = (on["meta_r"] != 0) & (on["score"] != -1)
    assert np.array_equal(mq[mapped], on["mapq"]["mapq"][mapped]) and not mq[~mapped].any()


def test_small_table_forces_overflow_exactly_where_the_rule_says(scen, gpu):
    for name in ("repeats-ties", "ont-2k", "seed12"):
        sc, di, oi = scen(name)
        want, pairs = mapq_ref.batch(oi, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"], slots=16)
        di.debug_set_mapq_slots(16)
        try:
            got, _, _, _, st = _device_records(di, gpu, sc["reads"], sc["lens"], sc["seed_len"], sc["thres"])
        finally:
            di.debug_set_mapq_slots(0)
        _same_records(got, want, (name, "16 slots"))
        over = (got["flags"] & capi.MAPQ_OVERFLOW) != 0
        assert np.array_equal(over, pairs > 16) and (got["n2"][over] == got["n1"][over]).all() and not got["mapq"][over].any()
        if name == "seed12":                            # reads on either side of 16 distinct pairs in one batch
            assert over.any() and (~over).any()
        if name == "repeats-ties":
            assert over.all()
    with pytest.raises(capi.LrmError, match="power of two"):
        scen("ont-2k")[1].debug_set_mapq_slots(24)
    with pytest.raises(capi.LrmError, match="power of two"):
        scen("ont-2k")[1].debug_set_mapq_slots(8192)


def test_meaning_on_a_planted_two_copy_repeat(gpu):
    """An exact 30 kbp two-copy repeat in 400 kbp: 10 kbp reads wholly inside a copy cannot be placed, reads from unique
    sequence can, and a MAPQ of 30 and more is nearly always right."""
    base = synth.reference(400_000, seed=61).copy()
    a0, b0, ln = 50_000, 250_000, 30_000
    base[b0:b0 + ln] = base[a0:a0 + ln]
    hi = index.HostIndex.build([base], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    try:
        n = 900
        r = synth.reads([base], n, 10_000, synth.ONT, seed=62)
        rm = r["reads"].copy()
        res = mapper.map_batch(di, rm, r["lens"], mapq=True)
    finally:
        di.close()
    mq = res["mapq"]["mapq"].astype(np.int64)
    pos, end = r["pos"].astype(np.int64), r["pos"].astype(np.int64) + r["span"].astype(np.int64)
    inside = ((pos >= a0) & (end <= a0 + ln)) | ((pos >= b0) & (end <= b0 + ln))
    unique = ((end <= a0) | (pos >= a0 + ln)) & ((end <= b0) | (pos >= b0 + ln))
    assert inside.sum() >= 30 and unique.sum() >= 400
    far = ~((np.abs(res["meta"]["off"].astype(np.int64) - pos) <= 300) & (res["meta"]["strand"] == r["strand"]) & (res["meta_r"] != 0))
    confident = mq >= 30
    print("mapq: inside a copy max %d (n %d); unique >= 50: %.4f (n %d); mapq >= 30: %d reads, %d misplaced" %
          (mq[inside].max(), inside.sum(), (mq[unique] >= 50).mean(), unique.sum(), confident.sum(), (far & confident).sum()))
    assert mq[inside].max() <= 3
    assert (mq[unique] >= 50).mean() >= 0.95
    assert (far & confident).sum() <= 0.01 * confident.sum()


def test_accaln_prints_the_records(gpu, tmp_path):
    """FASTQ in, SAM out: column 5 and v1:i / v2:i are the records of lrm_map_batch_submit_mapq; without the flag the file is
    lrm_accaln_opt's byte for byte."""
    seqs = [synth.reference(120_000, seed=71, repeat_frac=0.1, rep_len=500, rep_copies=20, rep_div=0.0), synth.reference(40_000, seed=72)]
    fa = tmp_path / "ref.fa"
    with open(fa, "wb") as f:
        for nm, s in zip((b"chrA", b"chrB"), seqs):
            f.write(b">" + nm + b"\n")
            b = bytes(s)
            for i in range(0, len(b), 60):
                f.write(b[i:i + 60] + b"\n")
    assert lib.lrm_accidx(str(fa).encode(), 32, 10, 1) == 0
    n = 150
    r = synth.reads(seqs, n, 1500, synth.ONT, seed=73)
    lens = r["lens"].copy()
    lens[::9] = 400
    lens[5] = 12
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for i in range(n):
            s = bytes(r["reads"][i, :lens[i]])
            f.write(b"@r%d\n" % i + s + b"\n+\n" + bytes(33 + (i + j) % 40 for j in range(len(s))) + b"\n")

    def run(path, mode):
        total, valid = C.c_uint64(), C.c_uint64()
        args = (str(fa).encode(), str(fq).encode(), str(path).encode(), capi.Params(64, 20, 300), capi.GactParams(0, 0, 0), gpu, 7,
                C.byref(total), C.byref(valid))
        if mode is None:
            capi.check(lib.lrm_accaln_opt(*args, None), "lrm_accaln_opt")
        else:
            capi.check(lib.lrm_accaln_mapq(*args, None, mode), "lrm_accaln_mapq")
        return open(path).read(), total.value, valid.value

    plain, total, valid = run(tmp_path / "plain.sam", None)
    off, t0, v0 = run(tmp_path / "off.sam", 0)
    on, t1, v1 = run(tmp_path / "on.sam", 1)
    assert off == plain and (t0, v0) == (t1, v1) == (total, valid) and total == n
    # the records the batches of 64 give (the flow maps batch by batch: max_len, and with it nothing the rule looks at, differs)
    hi = index.HostIndex.read(str(fa))
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    try:
        recs = []
        for lo in range(0, n, 64):
            bl = lens[lo:lo + 64].astype(np.uint32)
            rows = np.zeros((len(bl), int(bl.max()) + 1), dtype=np.uint8)
            for i, k in enumerate(bl):
                rows[i, :k] = r["reads"][lo + i, :k]
            recs.append(mapper.map_batch(di, rows, bl, mapq=True)["mapq"])
        recs = np.concatenate(recs)
        want, _ = mapq_ref.batch(orc.OracleIndex.from_host_index(hi), r["reads"], lens)
        _same_records(recs, want, "accaln batches")
    finally:
        di.close()
    a = [x.split("\t") for x in plain.splitlines() if not x.startswith("@")]
    b = [x.split("\t") for x in on.splitlines() if not x.startswith("@")]
    assert len(a) == len(b) == n and [x for x in plain.splitlines() if x.startswith("@")] == [x for x in on.splitlines() if x.startswith("@")]
    n_mapped = 0
    for i, (fa_, fb) in enumerate(zip(a, b)):
        mapped = not int(fa_[1]) & 4
        n_mapped += mapped
        assert fa_[4] == ("255" if mapped else "0") and fb[4] == (str(int(recs["mapq"][i])) if mapped else "0")
        assert fb[-2:] == ["v1:i:%d" % recs["n1"][i], "v2:i:%d" % recs["n2"][i]] and fb[-3].startswith("ED:I:")
        assert fb[:4] + fb[5:-2] == fa_[:4] + fa_[5:]
    assert n_mapped > 100 and len({x[4] for x in b}) > 3
