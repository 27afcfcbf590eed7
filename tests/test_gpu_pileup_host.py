"""The pileup on the host-buffer path and across replicas on the GPU (docs/GACT_SPEC.md, section of that name): batches through
map_batch(..., pileup=) against the device path and against the host rule over what the batches returned; two batches in
flight; the anchored + clip mode; the MAPQ filter; a group handle with one accumulator per replica and the merge;
pileup_merge_kernel alone on both routes; the accaln flow.  Everything is compared for equality, and every test reads the
raw planes with their guard words."""
import ctypes as C

import numpy as np
import pytest

import pileup_call_cases as KC
import pileup_host_cases as HC
import test_gpu_pileup as P
import test_pileup_ins_cpu as H
import workloads
from longreadmapper_amd import capi, index, mapper, synth, textio
from longreadmapper_amd.capi import lib
from longreadmapper_amd.pileup import Pileup

pytestmark = pytest.mark.gpu
SMALL = dict(lc_long_max=13)
K8 = HC.INS_COLS


def _device_path(di, gpu, reads, lens, window, seed_len=20, thres=300, **kw):
    """DeviceMapper over one batch -> (the mapper: the caller closes it, the raw planes, the raw insertion planes, results)"""
    import torch
    n, stride = reads.shape
    dm = mapper.DeviceMapper(di, n, stride - 1, seed_len, thres, device=gpu, pileup=window, pileup_ins_cols=K8, **kw)
    d_reads = torch.from_numpy(reads.copy()).cuda()
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    dm.seed(d_reads, d_lens)
    dm.extend(d_reads, d_lens)
    torch.cuda.synchronize()
    raw, ins = HC.dm_raw(dm)
    return dm, HC.guarded(raw), HC.guarded(ins), dm.results(n)


def _planes(acc):
    """the counter words of both allocations of a Pileup, their guard words checked"""
    return HC.guarded(acc.raw()), HC.guarded(acc.ins_raw())


def _run(handle, runs_in, acc, options, **kw):
    """every (reads, lens) through map_batch one after the other -> [(reads as the call left them, lens, res)]"""
    return [(reads, lens, mapper.map_batch(handle, reads, lens, 20, 300, options=options, pileup=acc, **kw)) for reads, lens in runs_in]


def _same_array(a, b):
    """every byte of a plain array, every field of a record array (the padding of a record is whatever the device buffer held)"""
    if a.dtype.names:
        return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[f], b[f]) for f in a.dtype.names if f != "_pad")
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_outputs(runs, plain):
    assert len(runs) == len(plain)
    for (reads, lens, res), (p_reads, p_lens, p_res) in zip(runs, plain):
        assert set(res) == set(p_res) and np.array_equal(reads, p_reads) and np.array_equal(lens, p_lens)
        for key in res:
            if isinstance(res[key], np.ndarray):
                assert _same_array(res[key], p_res[key]), key
            else:
                assert res[key] == p_res[key], key


@pytest.fixture(scope="module")
def planted(gpu):
    """The planted workload once: the device path's planes and calls, and the batches of the host path without an accumulator."""
    w = KC.planted()
    hi = index.HostIndex.build([w["text"]], names=["planted"], hlen=10)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    window = index.text_window(hi, 0)
    dm, raw, ins, _ = _device_path(di, gpu, w["reads"], w["lens"], window)
    sites, n_sites, _ = dm.pileup_sites()
    calls = dict(sites=sites, n_sites=n_sites, alleles=dm.pileup_site_alleles(sites), polish=dm.pileup_polish(), part=dm.pileup_polish(6000, 188_000))
    dm.close()
    assert raw.any() and ins.any()
    plain = {name: _run(di, HC.batches(w), None, opt) for name, opt in (("pipe", HC.PIPE), ("sliced", dict(HC.PIPE, slice_reads=HC.SLICE_READS)))}
    yield dict(w=w, hi=hi, di=di, window=window, raw=raw, ins=ins, calls=calls, plain=plain)
    di.close()
    hi.close()


# ---------------------------------------------------------------------------------------------------------
# 1. the same counts as the device path
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pipe", "sliced"])
def test_same_counts_as_the_device_path(planted, gpu, name):
    s = planted
    options = HC.PIPE if name == "pipe" else dict(HC.PIPE, slice_reads=HC.SLICE_READS)
    acc = Pileup(s["di"], *s["window"], K8, device=gpu)
    try:
        created = acc.bytes()
        runs = _run(s["di"], HC.batches(s["w"]), acc, options)
        raw, ins = _planes(acc)
        assert np.array_equal(raw, s["raw"]) and np.array_equal(ins, s["ins"]), name
        want, want_ins = HC.host_planes(runs, *s["window"], K8)
        assert np.array_equal(raw, want) and np.array_equal(ins, want_ins), name
        _same_outputs(runs, s["plain"][name])
        assert acc.bytes() == created                                   # nothing allocated on the accumulator
        # the read side on the Python object
        assert acc.columns(1000, 300).tobytes() == acc.columns()[1000:1300].tobytes()
        assert acc.ins_columns(1000, 300).tobytes() == acc.ins_columns()[1000:1300].tobytes()
        acc.reset()
        raw, ins = _planes(acc)
        assert not raw.any() and not ins.any()
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# 2. two batches in flight on one accumulator
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["text-keep-pinned", "pageable"])
def test_two_batches_in_flight(planted, gpu, how):
    s = planted
    pinned = how == "text-keep-pinned"
    options = dict(HC.PIPE, cigar_text=1, keep_reads=1) if pinned else HC.PIPE
    held = []

    def buffers():
        """fresh batches; pinned: reads and store in pinned memory"""
        out = []
        for reads, lens in HC.batches(s["w"]):
            store = None
            if pinned:
                pr = mapper.pinned_empty(reads.shape)
                pr[:] = reads
                store = mapper.pinned_empty((len(lens), max(mapper.units16(mapper.store_need(int(lens.max()), False)), 16)))
                store[:] = 0
                held.extend([pr, store])
                reads = pr
            out.append((reads, lens, store))
        return out

    submit = lambda acc, b: mapper.map_batch_submit(s["di"], b[0], b[1], 20, 300, store=b[2], options=options, pileup=acc)
    one, two = Pileup(s["di"], *s["window"], K8, device=gpu), Pileup(s["di"], *s["window"], K8, device=gpu)
    try:
        seq = [submit(one, b).wait() for b in buffers()]
        bufs = buffers()
        first, second = submit(two, bufs[0]), submit(two, bufs[1])       # submit, submit, wait, wait
        flight = [first.wait(), second.wait(), submit(two, bufs[2]).wait()]
        raw1, ins1 = _planes(one)
        raw2, ins2 = _planes(two)
        assert np.array_equal(raw1, raw2) and np.array_equal(ins1, ins2), how
        assert np.array_equal(raw1, s["raw"]) and np.array_equal(ins1, s["ins"]), how      # whatever the layout of the results
        for a, b in zip(seq, flight):
            for key in ("best", "n_ops", "score", "meta", "meta_r"):
                assert _same_array(a[key], b[key]), (how, key)
        if pinned:                                                        # keep_reads: the caller's reads stayed as sequenced
            assert np.array_equal(np.concatenate([b[0] for b in bufs]), s["w"]["reads"])
    finally:
        one.close()
        two.close()
        for a in held:
            mapper.pinned_free(a)


# ---------------------------------------------------------------------------------------------------------
# 3. anchored + clip
# ---------------------------------------------------------------------------------------------------------
def test_anchored_clip_mode(planted, gpu):
    s = planted
    reads, lens = s["w"]["reads"][:600].copy(), s["w"]["lens"][:600].copy()
    dm, raw, ins, _ = _device_path(s["di"], gpu, reads, lens, s["window"], clip=True)
    dm.close()
    acc = Pileup(s["di"], *s["window"], K8, device=gpu)
    try:
        res = mapper.map_batch(s["di"], reads, lens, 20, 300, options=HC.PIPE, clip=True, pileup=acc)
        got, got_ins = _planes(acc)
        assert np.array_equal(got, raw) and np.array_equal(got_ins, ins) and raw.any() and ins.any()
        want, want_ins = HC.host_planes([(reads, lens, res)], *s["window"], K8)
        assert np.array_equal(got, want) and np.array_equal(got_ins, want_ins)
    finally:
        acc.close()


# ---------------------------------------------------------------------------------------------------------
# 4. the MAPQ filter
# ---------------------------------------------------------------------------------------------------------
def _filter_scene(name):
    if name == "ont":
        sc = workloads.scenario("ont-2k")
        return sc["hi"], sc["reads"], sc["lens"], None
    # the planted two-copy repeat of tests/test_gpu_pileup.py: the vote cannot place the reads inside the copies
    base = synth.reference(400_000, seed=61).copy()
    base[250_000:280_000] = base[50_000:80_000]
    hi = index.HostIndex.build([base], hlen=10)
    r = synth.reads([base], 160, 10_000, synth.ONT, seed=62)
    return hi, r["reads"], r["lens"], hi


@pytest.mark.parametrize("scene", ["ont", "two-copy-repeat"])
def test_min_mapq_filter(gpu, scene):
    hi, reads, lens, owned = _filter_scene(scene)
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    window = (0, int(hi.h.con_len))
    acc = Pileup(di, *window, K8, device=gpu)
    try:
        dm, raw, ins, _ = _device_path(di, gpu, reads, lens, window, mapq=True, pileup_min_mapq=1)
        dm.close()
        mine = reads.copy()
        res = mapper.map_batch(di, mine, lens, 20, 300, options=HC.PIPE, mapq=True, pileup=acc, pileup_min_mapq=1)
        got, got_ins = _planes(acc)
        assert np.array_equal(got, raw) and np.array_equal(got_ins, ins) and raw.any()
        want, want_ins = HC.host_planes([(mine, lens, res)], *window, K8, min_mapq=1)
        assert np.array_equal(got, want) and np.array_equal(got_ins, want_ins)
        live = (res["meta_r"] != 0) & (res["score"] != -1) & (res["n_ops"] > 0)
        dropped = int((live & (res["mapq"]["mapq"] == 0)).sum())
        print("%s: %d mapped reads, %d of them with MAPQ 0 kept out of the pileup" % (scene, int(live.sum()), dropped))
        if scene == "two-copy-repeat":                                   # (the 64 reads of the ont scene are all placed)
            assert dropped >= 3 and int((live & (res["mapq"]["mapq"] >= 1)).sum()) >= 50
            unfiltered, _ = HC.host_planes([(mine, lens, res)], *window, 0)
            assert not np.array_equal(unfiltered, want)
        # the filter needs the records of the batch
        before = acc.raw()
        with pytest.raises(capi.LrmError, match="min_mapq needs lrm_batch_extras.mapq_out"):
            mapper.map_batch(di, reads.copy(), lens, 20, 300, options=HC.PIPE, pileup=acc, pileup_min_mapq=1)
        assert np.array_equal(acc.raw(), before)
    finally:
        acc.close()
        di.close()
        if owned is not None:
            owned.close()


# ---------------------------------------------------------------------------------------------------------
# 5. a group handle: one accumulator per replica, merged
# ---------------------------------------------------------------------------------------------------------
def test_group_handle_and_merge(planted, gpu):
    import torch
    s = planted
    dg = index.DeviceIndex.upload_multi(s["hi"], [gpu, gpu], **SMALL)
    a = b = None
    try:
        assert dg.replicas == 2
        h = C.c_void_p()
        assert lib.lrm_pileup_create(C.byref(h), dg.handle, 0, 100) < 0 and b"group handle" in lib.lrm_last_error() and not h     # as before
        assert lib.lrm_pileup_create_replica(C.byref(h), dg.handle, 2, 0, 100, 0) < 0 and b"replica 2" in lib.lrm_last_error() and not h
        a = Pileup(dg, *s["window"], K8, replica=0, device=gpu)
        b = Pileup(lib.lrm_index_replica(dg.handle, 1), *s["window"], K8, device=gpu)
        runs = _run(dg, HC.batches(s["w"]), [a, b], HC.PIPE)
        _same_outputs(runs, s["plain"]["pipe"])
        raw_a, ins_a = _planes(a)
        raw_b, ins_b = _planes(b)
        assert raw_a.any() and raw_b.any() and ins_a.any() and ins_b.any()              # both replicas took a share
        assert np.array_equal(raw_a + raw_b, s["raw"]) and np.array_equal(ins_a + ins_b, s["ins"])
        a.merge(b)
        torch.cuda.synchronize()
        got, got_ins = _planes(a)
        assert np.array_equal(got, s["raw"]) and np.array_equal(got_ins, s["ins"])
        after_b = _planes(b)
        assert np.array_equal(after_b[0], raw_b) and np.array_equal(after_b[1], ins_b)    # src is not modified
        calls = s["calls"]
        sites, n_sites, _ = a.sites()
        assert n_sites == calls["n_sites"] and sites.tobytes() == calls["sites"].tobytes()
        assert a.site_alleles(sites).tobytes() == calls["alleles"].tobytes()
        assert a.polish().tobytes() == calls["polish"].tobytes()
        part = bytes(a.polish(6000, 188_000, cap=1000))
        assert part == bytes(calls["part"]) == H.copy_slice(s["w"], 6000, 194_000) and len(part) == 187_995
        # the refusals: nothing is queued, nothing is added
        reads, lens = HC.batches(s["w"])[0]
        for piles, text in (([a], "1 accumulators for a handle of 2"), ([a, b, b], "3 accumulators"), ([b, a], "not created on replica 0"),
                            ([a, None], r"pileups\[1\] is NULL"), ([None, b], r"pileups\[0\] is NULL")):
            with pytest.raises(capi.LrmError, match=text):
                mapper.map_batch(dg, reads, lens, 20, 300, options=HC.PIPE, pileup=piles)
        arr = (C.c_void_p * 2)(a.handle, b.handle)
        bp = capi.BatchPileup(C.sizeof(capi.BatchPileup), 0, arr, 2, 1)
        buf = mapper.ResultBuffers(len(lens), 2 * s["w"]["reads"].shape[1])
        t = C.c_void_p()
        rc = lib.lrm_map_batch_submit_ex3(dg.handle, reads.ctypes.data, reads.shape[1], lens.ctypes.data, len(lens), capi.Params(len(lens), 20, 300),
                                          capi.GactParams(*mapper.DEFAULT_GACT), buf.best.ctypes.data, *buf.out_args, None, None, None, C.byref(bp), C.byref(t))
        assert rc < 0 and b"reserved" in lib.lrm_last_error() and not t
        assert np.array_equal(_planes(a)[0], s["raw"]) and np.array_equal(_planes(b)[0], raw_b)
    finally:
        for acc in (a, b):
            if acc is not None:
                acc.close()
        dg.close()


# ---------------------------------------------------------------------------------------------------------
# 6. the merge alone
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ont_index(gpu):
    sc = workloads.scenario("ont-2k")
    di = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL)
    yield di
    di.close()


def _add(acc, rows):
    b = P._batch(rows, stride=224, read_stride=208)
    capi.check(lib.lrm_pileup_add_dev(acc.handle, b["reads"].data_ptr(), b["read_stride"], b["lens"].data_ptr(), b["store"].data_ptr(), b["stride"],
                                      b["n_ops"].data_ptr(), b["score"].data_ptr(), b["meta_r"].data_ptr(), b["meta"].data_ptr(), b["n"], None, 0,
                                      acc._stream()), "lrm_pileup_add_dev")


@pytest.mark.parametrize("K", HC.MERGE_KS)
@pytest.mark.parametrize("W", HC.MERGE_WIDTHS)
def test_merge_alone(ont_index, gpu, W, K):
    lo = 5000
    dst, src = Pileup(ont_index, lo, lo + W, K, device=gpu), Pileup(ont_index, lo, lo + W, K, device=gpu)
    try:
        _add(src, HC.edge_rows(lo, W, seed=W + K))
        _add(dst, HC.edge_rows(lo, W, seed=1000 + W) + HC.edge_rows(lo, W, seed=2000 + W)[:2])
        d0, s0 = dst.raw(), src.raw()
        di0, si0 = (dst.ins_raw(), src.ins_raw()) if K else (None, None)
        first, second = HC.edge_words(W, K)
        assert all(s0[i] for i in first) and all(d0[i] for i in first) and not np.array_equal(d0, s0)
        if K:
            assert all(si0[i] for i in second) and all(di0[i] for i in second)
        created = dst.bytes()
        staged = created + HC.MERGE_CHUNK_BYTES

        def check(times, bytes_now):
            got = dst.raw()
            assert np.array_equal(HC.guarded(got), HC.guarded(d0) + np.uint32(times) * HC.guarded(s0)), (W, K, times)
            assert np.array_equal(src.raw(), s0)                        # src and its guard words as they were
            if K:
                assert np.array_equal(HC.guarded(dst.ins_raw()), HC.guarded(di0) + np.uint32(times) * HC.guarded(si0)), (W, K, times)
                assert np.array_equal(src.ins_raw(), si0)
            assert dst.bytes() == bytes_now and src.bytes() == created, (W, K, times)

        dst.merge(src)
        check(1, created)
        dst.merge(src)                                                  # merging twice adds twice
        check(2, created)
        dst.merge(src, staged_chunk=4)
        check(3, staged)                                                # the staging buffer is booked by the first staged merge ...
        dst.merge(src, staged_chunk=1024)
        check(4, staged)                                                # ... once
        dst.merge(src)
        check(5, staged)
    finally:
        dst.close()
        src.close()


def test_merge_refusals(ont_index, gpu):
    lo, W = 5000, 300
    dst = Pileup(ont_index, lo, lo + W, 4, device=gpu)
    others = dict(window_lo=Pileup(ont_index, lo + 1, lo + W, 4, device=gpu), window_hi=Pileup(ont_index, lo, lo + W + 1, 4, device=gpu),
                  cols=Pileup(ont_index, lo, lo + W, 8, device=gpu), plain=Pileup(ont_index, lo, lo + W, 0, device=gpu),
                  same=Pileup(ont_index, lo, lo + W, 4, device=gpu))
    try:
        _add(dst, HC.edge_rows(lo, W, seed=1))
        before, before_ins, created = dst.raw(), dst.ins_raw(), dst.bytes()
        for name, text in (("window_lo", "windows"), ("window_hi", "windows"), ("cols", "insertion columns"), ("plain", "insertion columns")):
            for chunk in (None, 8):
                with pytest.raises(capi.LrmError, match=text):
                    dst.merge(others[name], staged_chunk=chunk)
        with pytest.raises(capi.LrmError, match="same accumulator"):
            dst.merge(dst)
        for chunk in (0, 2, 3, 6, 1022):
            with pytest.raises(capi.LrmError, match="not a multiple of 4"):
                dst.merge(others["same"], staged_chunk=chunk)
        with pytest.raises(capi.LrmError, match="staging buffer holds"):
            dst.merge(others["same"], staged_chunk=HC.MERGE_CHUNK_BYTES // 4 + 4)
        assert lib.lrm_pileup_merge_dev(dst.handle, None, None) < 0 and lib.lrm_pileup_merge_dev(None, dst.handle, None) < 0
        assert np.array_equal(dst.raw(), before) and np.array_equal(dst.ins_raw(), before_ins) and dst.bytes() == created
    finally:
        dst.close()
        for acc in others.values():
            acc.close()


# ---------------------------------------------------------------------------------------------------------
# 7. the accaln flow
# ---------------------------------------------------------------------------------------------------------
def _fasta(name, seq):
    """>name and the sequence 60 columns a line, as textio.write_consensus lays one out"""
    seq = bytes(seq)
    return b">" + name + b"\n" + b"".join(seq[p:p + 60] + b"\n" for p in range(0, len(seq), 60))


def test_accaln_flow(planted, gpu, tmp_path):
    s = planted
    w, calls = s["w"], s["calls"]
    fa, fq = tmp_path / "planted.fa", tmp_path / "reads.fq"
    HC.write_fasta(fa, [(b"planted", w["text"])])
    assert lib.lrm_accidx(str(fa).encode(), 32, 10, 1) == 0
    HC.write_fastq(fq, w["reads"], w["lens"])
    n = len(w["lens"])
    run = lambda out, **kw: textio.accaln(str(fa), str(fq), None if out is None else str(tmp_path / out), 600, device=gpu, rg_id=7, mapq=1, **kw)
    counts = run("plain.sam")
    assert counts[0] == n and counts[1] > n * 9 // 10
    req = lambda tag: dict(seq=0, ins_cols=K8, sites=str(tmp_path / (tag + ".tsv")), fasta=str(tmp_path / (tag + ".fa")))
    assert run("pile.sam", pileup=req("with")) == counts
    assert open(tmp_path / "pile.sam", "rb").read() == open(tmp_path / "plain.sam", "rb").read()
    # the device path's table and polished bytes through the Python writers
    hi = index.HostIndex.read(str(fa))
    try:
        assert index.text_window(hi, 0) == s["window"]
        assert textio.write_sites(str(tmp_path / "want.tsv"), hi, calls["sites"], alleles=calls["alleles"]) == calls["n_sites"]
    finally:
        hi.close()
    want_sites, want_fasta = open(tmp_path / "want.tsv", "rb").read(), _fasta(b"planted", calls["polish"])
    assert calls["n_sites"] >= 60 and len(want_sites.split(b"\n")) == calls["n_sites"] + 1
    assert open(tmp_path / "with.tsv", "rb").read() == want_sites
    assert open(tmp_path / "with.fa", "rb").read() == want_fasta
    # without a SAM file: the same two files, the same counters
    assert run(None, pileup=req("alone")) == counts
    assert open(tmp_path / "alone.tsv", "rb").read() == want_sites and open(tmp_path / "alone.fa", "rb").read() == want_fasta
    assert sorted(p.name for p in tmp_path.glob("*.sam")) == ["pile.sam", "plain.sam"]
    # either path may be missing
    only = dict(req("only"), sites=None)
    assert run(None, pileup=only) == counts
    assert open(tmp_path / "only.fa", "rb").read() == want_fasta and not (tmp_path / "only.tsv").exists()
