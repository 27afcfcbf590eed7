"""Split reads (lrm_map_options.split; docs/GACT_SPEC.md, "Split reads") on the GPU: the soft-clipped ends of a clipped batch
mapped as reads of their own -- the segment table against tests/split_ref.py, every per-segment output against the existing
calls over a batch made of the segment rows, host entry point against device entry point, SAM text against the Python
formatter -- and what the stage is for: the other half of a chimeric read gets a supplementary alignment."""
import ctypes as C

import numpy as np
import pytest

import sam_ref
import split_ref
from longreadmapper_amd import capi, index, mapper, synth
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu
GACT = (320, 120, 128)
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
SEG_KEYS = ("n_ops", "score", "meta_r")


@pytest.fixture(scope="module")
def ref3(gpu):
    seqs = [synth.reference(1_500_000, seed=41, repeat_frac=0.05, rep_len=300, rep_copies=200, rep_div=0.05),
            synth.reference(700_000, seed=42), synth.reference(300_000, seed=43)]
    hi = index.HostIndex.build(seqs, names=["chrA", "chrB", "chrC"], hlen=12)
    di = index.DeviceIndex.upload(hi, gpu)
    yield seqs, hi, di
    di.close()


def _random(rng, n):
    return BASES[rng.integers(0, 4, n)]


def _concat(parts):
    """Reads made of the given pieces (uint8 arrays) back to back -> reads (n, stride), lens."""
    lens = np.array([sum(len(p) for p in ps) for ps in parts], dtype=np.uint32)
    reads = np.zeros((len(parts), int(lens.max()) + 1), dtype=np.uint8)
    for i, ps in enumerate(parts):
        at = 0
        for p in ps:
            reads[i, at:at + len(p)] = p
            at += len(p)
    return reads, lens


def _piece(r, i):
    return r["reads"][i, :int(r["lens"][i])]


def _ragged_chimeras(seqs, seed=3):
    """Chimeras of two and three parts (synth.reads draws both strands: every combination occurs), junk heads and tails,
    random reads (no anchor), plain reads, lengths 1 .. 6000."""
    rng = np.random.default_rng(seed)
    sets = {ln: synth.reads(seqs, 260, ln, synth.ONT if k % 2 == 0 else synth.PACBIO_CLR, seed=seed + k)
            for k, ln in enumerate((150, 260, 420, 900, 2100, 3000))}
    nxt = {ln: 0 for ln in sets}

    def take(ln):
        i = nxt[ln]
        nxt[ln] += 1
        return _piece(sets[ln], i)

    parts = []
    for k in range(60):
        parts.append([take(3000), take(2100)])
        parts.append([take(2100), take(900)])
        parts.append([take(900), take(420), take(2100)])
        parts.append([take(420), take(3000), take(260)])
        parts.append([take(260), take(900)])
    for k in range(60):
        parts.append([_random(rng, int(rng.integers(50, 700))), take(2100), _random(rng, int(rng.integers(50, 700)))])
        parts.append([take(900)])
        parts.append([take(150)])
    for k in range(20):
        parts.append([_random(rng, int(rng.integers(1, 3000)))])
    for ln in (1, 7, 19, 37):
        parts.append([_random(rng, ln)])
    order = rng.permutation(len(parts))
    return _concat([parts[i] for i in order])


def _device_split(di, gpu, reads, lens, gact=GACT, **kw):
    """seed -> clipped extension -> split through DeviceMapper; -> results (with res["split"]), the reads as they were left."""
    import torch
    n, max_len = len(lens), int(lens.max()) if len(lens) else 1
    dm = mapper.DeviceMapper(di, max(n, 1), max_len, gact=gact, device=gpu, clip=True, split=True, **kw)
    try:
        d_reads = torch.from_numpy(reads).cuda()
        d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens, n)
        dm.extend(d_reads, d_lens, n)
        k = dm.split(d_reads, d_lens, n)
        torch.cuda.synchronize()
        res = dm.results(n)
        assert len(res["split"]["seg"]) == k
        res["workspace_bytes"] = dm.workspace_bytes()
        return res, d_reads.cpu().numpy()
    finally:
        dm.close()


def _table(seg, mask=~np.uint32(split_ref.SEG_ALIGNED)):
    return [(int(s["read"]), int(s["start"]), int(s["len"]), int(s["flags"] & mask)) for s in seg]


def _rows_of(oriented, lens, table):
    """The segment batch before its own extension: slices of the reads as the primary's extension left them."""
    seg_lens = np.array([t[2] for t in table], dtype=np.uint32)
    rows = np.zeros((len(table), (int(seg_lens.max()) if len(table) else 0) + 16), dtype=np.uint8)
    for s, (read, start, ln, _) in enumerate(table):
        rows[s, :ln] = oriented[read, start:start + ln]
    return rows, seg_lens


def _same_meta(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("loc", "off", "seq_id", "strand"))


def _check_segments(sp, want, rows_after, table):
    """sp: a split result; want: map_batch over the segment rows (rows layout); rows_after: those rows as map_batch left them."""
    k = len(table)
    assert _table(sp["seg"]) == table
    assert np.array_equal(sp["lens"], [t[2] for t in table])
    assert np.array_equal(sp["best"], want["best"])
    for key in SEG_KEYS:
        assert np.array_equal(sp[key], want[key]), key
    assert _same_meta(sp["meta"], want["meta"])
    for s in range(k):
        ops = mapper.ops_of(want, s)
        if sp.get("is_text"):
            assert mapper.text_of(sp, s).decode() == (sam_ref.rle(ops) if want["meta_r"][s] and want["score"][s] >= 0 else "*")
        else:
            assert mapper.ops_of(sp, s) == ops, s
        ln = table[s][2]
        assert np.array_equal(sp["rows"][s, :ln], rows_after[s, :ln]), s
        assert (int(sp["clip"]["left"][s]), int(sp["clip"]["right"][s])) == split_ref.clip_of_ops(ops if want["meta_r"][s] else b"")
        reported = bool(sp["meta_r"][s] != 0 and sp["anchor"]["flags"][s] & capi.ANCHOR_ANCHORED)
        assert bool(sp["seg"]["flags"][s] & split_ref.SEG_ALIGNED) == reported


@pytest.fixture(scope="module")
def chimeras(ref3):
    seqs, hi, di = ref3
    return _ragged_chimeras(seqs)


@pytest.mark.parametrize("impl,gact", [(1, GACT), (3, GACT), (4, GACT), (0, (320, 120, 256))])
def test_segments_equal_the_existing_calls_over_their_rows(ref3, chimeras, map_options, gpu, impl, gact):
    seqs, hi, di = ref3
    reads, lens = chimeras
    map_options(di, gact_impl=impl)
    res, oriented = _device_split(di, gpu, reads, lens, gact)
    sp = res["split"]
    table = split_ref.plan(lens, res["clip"]["left"], res["clip"]["right"])
    assert len(table) > 250 and sum(t[3] for t in table) > 60 and len({t[0] for t in table}) < len(table)      # both sides, two per read
    rows, seg_lens = _rows_of(oriented, lens, table)
    after = rows.copy()
    want = mapper.map_batch(di, after, seg_lens, gact=gact, clip=True)
    _check_segments(sp, want, after, table)
    for s, t in enumerate(table):                                   # zeros from the segment's end to the next multiple of 16
        assert not sp["rows"][s, t[2]:(t[2] + 15) // 16 * 16].any()
    flags = sp["seg"]["flags"]
    print("impl %d: %d reads, %d segments, %d reported, %d without a locus" %
          (impl, len(lens), len(table), int(((flags & 2) != 0).sum()), int((sp["meta_r"] == 0).sum())))
    assert ((flags & 2) != 0).sum() > 150 and ((flags & 2) == 0).sum() > 50
    # the primary pass is what it is without the stage
    plain = mapper.map_batch(di, reads.copy(), lens, gact=gact, clip=True)
    for key in ("best",) + SEG_KEYS:
        assert np.array_equal(res[key], plain[key]), key
    for i in range(len(lens)):
        assert bytes(res["ops"][i, :res["n_ops"][i]]) == mapper.ops_of(plain, i)


def test_host_entry_point_equals_device(ref3, chimeras, gpu):
    seqs, hi, di = ref3
    di.set_map_options()
    reads, lens = chimeras
    dev, oriented = _device_split(di, gpu, reads, lens)
    table = _table(dev["split"]["seg"])
    rows, seg_lens = _rows_of(oriented, lens, table)
    after = rows.copy()
    want = mapper.map_batch(di, after, seg_lens, clip=True)
    full = _table(dev["split"]["seg"], mask=~np.uint32(0))
    d2 = index.DeviceIndex.upload_multi(hi, [gpu, gpu])
    try:
        for handle, options in ((di, None), (di, {"dense_results": 1}), (di, {"cigar_text": 1}), (di, {"keep_reads": 1}),
                                (di, {"cigar_text": 1, "keep_reads": 1}), (d2, None), (d2, {"dense_results": 1, "keep_reads": 1})):
            buf = reads.copy()
            res = mapper.map_batch(handle, buf, lens, options=options, clip=True)
            if options and options.get("keep_reads"):
                assert np.array_equal(buf, reads)
            sp = mapper.split_batch(handle, buf, lens, res, options=options)
            _check_segments(sp, want, after, table)
            assert _table(sp["seg"], mask=~np.uint32(0)) == full, options
            for key in ("text_pos", "read_pos", "len", "delta", "left_ops", "flags"):
                assert np.array_equal(sp["anchor"][key], dev["split"]["anchor"][key]), key
    finally:
        d2.close()


def test_chunks_capacity_and_empty_batches(ref3, gpu):
    import torch
    seqs, hi, di = ref3
    di.set_map_options()
    rng = np.random.default_rng(11)
    a = synth.reads(seqs, 2500, 700, synth.ONT, seed=61)
    b = synth.reads(seqs, 2500, 500, synth.ONT, seed=62)
    c = synth.reads(seqs, 2500, 400, synth.ONT, seed=63)
    reads, lens = _concat([[_piece(a, i), _piece(b, i), _piece(c, i)] for i in range(2500)])
    whole, _ = _device_split(di, gpu, reads, lens)
    k = len(whole["split"]["seg"])
    assert k > 2000
    small, _ = _device_split(di, gpu, reads, lens, seg_rows=64)               # dozens of chunks through 64 rows
    own, _ = _device_split(di, gpu, reads, lens, seg_rows=0)                  # the primary's workspace a second time
    for other in (small, own):
        for key in ("seg", "lens", "best", "n_ops", "score", "meta_r", "clip", "rows"):
            assert np.array_equal(other["split"][key], whole["split"][key]), key
        for key in ("text_pos", "read_pos", "len", "delta", "left_ops", "flags"):
            assert np.array_equal(other["split"]["anchor"][key], whole["split"]["anchor"][key]), key
        assert _same_meta(other["split"]["meta"], whole["split"]["meta"])
        for s in range(k):
            assert mapper.ops_of(other["split"], s) == mapper.ops_of(whole["split"], s)
    with pytest.raises(capi.LrmError, match="segments, room for") as e:
        _device_split(di, gpu, reads, lens, seg_cap=k - 1)
    assert (e.value.rc, e.value.n_seg) == (-3, k)
    res = mapper.map_batch(di, reads.copy(), lens, clip=True)
    with pytest.raises(capi.LrmError, match="segments, room for") as e:
        mapper.split_batch(di, reads, lens, res, cap=k - 1)
    assert (e.value.rc, e.value.n_seg) == (-3, k)
    # no segment: untouched reads; nothing is written
    r = synth.reads(seqs, 200, 3000, synth.ONT, seed=64)
    dm = mapper.DeviceMapper(di, 200, 3000, device=gpu, clip=True, split=True)
    try:
        for t in dm.seg.values():
            t.fill_(77)
        d_reads, d_lens = torch.from_numpy(r["reads"]).cuda(), torch.from_numpy(r["lens"].astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        assert dm.split(d_reads, d_lens) == 0 and dm.split(d_reads, d_lens, 0) == 0
        torch.cuda.synchronize()
        assert all(bool((t == 77).all()) for t in dm.seg.values())
    finally:
        dm.close()
    res = mapper.map_batch(di, r["reads"].copy(), r["lens"], clip=True)
    assert len(mapper.split_batch(di, r["reads"], r["lens"], res)["seg"]) == 0
    assert len(mapper.split_batch(di, r["reads"][:0], r["lens"][:0], {k2: v[:0] for k2, v in res.items() if k2 != "is_text"})["seg"]) == 0


def test_scratch_grows_with_a_larger_second_batch(ref3, gpu):
    """Two calls on one segment workspace: 200 reads (one workgroup of the count / mark kernels), then 600 (three; the
    per-workgroup scratch of the first call is too small) with a two-segment read in lane 255 of the first workgroup."""
    import torch
    seqs, hi, di = ref3
    di.set_map_options()
    rng = np.random.default_rng(23)
    n, M = 600, 50
    lens = rng.integers(200, 301, n).astype(np.uint32)
    reads = np.zeros((n, 304), dtype=np.uint8)
    for i in range(n):
        reads[i, :lens[i]] = _random(rng, int(lens[i]))
    cl, cr = (rng.integers(0, 100, n) * (rng.random(n) < 0.6)).astype(np.uint32), (rng.integers(0, 100, n) * (rng.random(n) < 0.6)).astype(np.uint32)
    cl[255], cr[255] = 70, 90
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    dm = mapper.DeviceMapper(di, n, 300, device=gpu, clip=True, split=True, split_min_len=M)
    try:
        clip = np.zeros(n, dtype=mapper.CLIP_DT)
        clip["left"], clip["right"] = cl, cr
        dm.clip.copy_(torch.from_numpy(clip.view(np.int32).reshape(n, 2)).cuda())
        d_reads, d_lens = torch.from_numpy(reads).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
        grown = []
        for m in (200, 600):
            k = dm.split(d_reads, d_lens, m)
            torch.cuda.synchronize()
            grown.append(int(lib.lrm_workspace_bytes(dm.ws_seg)))
            sp = dm.split_results()
            table = split_ref.plan(lens[:m], cl[:m], cr[:m], M)
            assert k == len(table) > m // 2 and _table(sp["seg"]) == table
            assert np.array_equal(sp["lens"], [t[2] for t in table])
            rows, seg_lens = _rows_of(reads, lens, table)
            for s, t in enumerate(table):                           # (a segment with a reverse-strand locus was turned round)
                row = bytes(rows[s, :t[2]])
                if sp["meta_r"][s] != 0 and sp["meta"]["strand"][s] == 1:
                    row = row.translate(comp)[::-1]
                assert bytes(sp["rows"][s, :t[2]]) == row, (m, s)
        assert [t for t in table if t[0] == 255] == [(255, 0, 70, 0), (255, int(lens[255]) - 90, 90, 1)]
        assert grown[1] - grown[0] == 8 * (3 - 1)                   # 8 bytes per workgroup of 256 reads
    finally:
        dm.close()
    assert np.array_equal(d_reads.cpu().numpy(), reads)


def test_off_means_off(ref3, chimeras, gpu):
    seqs, hi, di = ref3
    di.set_map_options()
    reads, lens = chimeras
    base = mapper.map_batch(di, reads.copy(), lens, clip=True)
    with_opt = mapper.map_batch(di, reads.copy(), lens, options={"split": 1, "split_min_len": 100}, clip=True)
    for key in ("best", "ops", "n_ops", "score", "meta", "meta_r"):
        assert np.array_equal(base[key], with_opt[key]), key
    a = mapper.DeviceMapper(di, 64, 2000, device=gpu, clip=True)
    b = mapper.DeviceMapper(di, 64, 2000, device=gpu, clip=True, split=True)
    try:
        assert a.workspace_bytes() == b.workspace_bytes()
    finally:
        a.close()
        b.close()
    with pytest.raises(capi.LrmError, match="split needs clip"):
        mapper.DeviceMapper(di, 64, 2000, device=gpu, anchored=True, split=True)
    bufs = mapper.SplitBuffers(16, 100)
    cig = (capi.Cigar * 1)()
    opt = capi.map_options(anchored=1, split=1)
    rc = lib.lrm_split_batch(di.handle, reads.ctypes.data, reads.shape[1], lens.ctypes.data, 1, C.cast(cig, C.c_void_p),
                             base["meta"].ctypes.data, base["meta_r"].ctypes.data, capi.Params(1, 20, 300), capi.GactParams(*GACT),
                             C.byref(opt), C.byref(bufs.out))
    assert rc == -1 and b"needs lrm_map_options.clip" in lib.lrm_last_error()
    total, valid = C.c_uint64(), C.c_uint64()
    rc = lib.lrm_accaln_opt(b"/nonexistent", b"/nonexistent", b"/nonexistent", capi.Params(8, 20, 300), capi.GactParams(*GACT), gpu, 1,
                            C.byref(total), C.byref(valid), C.byref(opt))
    assert rc == -1 and b"split needs lrm_map_options.clip" in lib.lrm_last_error()


# ---------------------------------------------------------------------------------------------------------
# what it is for
# ---------------------------------------------------------------------------------------------------------
def _placed(meta_r, meta, r):
    return (meta_r == 1) & (meta["seq_id"] == r["seq"]) & (meta["strand"] == r["strand"])


def test_the_other_half_of_a_chimera_is_placed(ref3):
    seqs, hi, di = ref3
    di.set_map_options()
    a = synth.reads(seqs, 300, 6000, synth.ONT, seed=51)
    b = synth.reads(seqs, 300, 4000, synth.ONT, seed=52)
    n = 300
    reads, lens = _concat([[_piece(a, i), _piece(b, i)] for i in range(n)])
    buf = reads.copy()
    res = mapper.map_batch(di, buf, lens, clip=True)
    sp = mapper.split_batch(di, buf, lens, res)
    on_a, on_b = _placed(res["meta_r"], res["meta"], a), _placed(res["meta_r"], res["meta"], b)
    good, cover = 0, []
    for i in range(n):
        if not (on_a[i] or on_b[i]):
            continue
        other = b if on_a[i] else a
        ps = int(res["meta"]["strand"][i])
        ops = mapper.ops_of(res, i)
        aligned = sum(c in b"=XI" for c in ops)
        hit = False
        for s in np.flatnonzero(sp["seg"]["read"] == i):
            if not sp["seg"]["flags"][s] & split_ref.SEG_ALIGNED:
                continue
            aligned += sum(c in b"=XI" for c in mapper.ops_of(sp, s))
            strand = ps ^ int(sp["meta"]["strand"][s])
            hit |= (int(sp["meta"]["seq_id"][s]) == other["seq"][i] and strand == other["strand"][i] and
                    abs(int(sp["meta"]["off"][s]) - int(other["pos"][i])) <= 60)
        good += hit
        cover.append(aligned / int(lens[i]))
    placed = int((on_a | on_b).sum())
    print("chimeras 6 kbp + 4 kbp: %d placed, other part reported at its true place for %d, median cover %.3f" %
          (placed, good, np.median(cover)))
    assert placed >= 0.95 * n and good >= 0.9 * placed and np.median(cover) >= 0.95


def test_junk_is_not_reported_and_untouched_reads_have_no_segments(ref3):
    seqs, hi, di = ref3
    di.set_map_options()
    rng = np.random.default_rng(9)
    r = synth.reads(seqs, 1000, 3000, synth.ONT, seed=71)
    reads, lens = _concat([[_random(rng, 300), _piece(r, i), _random(rng, 600)] for i in range(1000)])
    buf = reads.copy()
    res = mapper.map_batch(di, buf, lens, clip=True)
    sp = mapper.split_batch(di, buf, lens, res)
    reported = int(((sp["seg"]["flags"] & split_ref.SEG_ALIGNED) != 0).sum())
    print("1000 reads with 300 + 600 junk bases: %d segments, %d reported" % (len(sp["seg"]), reported))
    assert len(sp["seg"]) >= 1500 and reported <= 10
    plain = synth.reads(seqs, 500, 5000, synth.ONT, seed=72)
    buf = plain["reads"].copy()
    res = mapper.map_batch(di, buf, plain["lens"], clip=True)
    assert len(mapper.split_batch(di, buf, plain["lens"], res)["seg"]) == 0


def test_short_segments_show_where_placement_falls_off(ref3):
    seqs, hi, di = ref3
    di.set_map_options()
    host = synth.reads(seqs, 400, 3000, synth.ONT, seed=81)
    line = []
    for ln in (150, 200, 250, 300, 400):
        tail = synth.reads(seqs, 400, ln, synth.ONT, seed=82 + ln)
        reads, lens = _concat([[_piece(host, i), _piece(tail, i)] for i in range(400)])
        buf = reads.copy()
        res = mapper.map_batch(di, buf, lens, clip=True)
        sp = mapper.split_batch(di, buf, lens, res, split_min_len=100)
        ok = 0
        for s in np.flatnonzero((sp["seg"]["flags"] & split_ref.SEG_ALIGNED) != 0):
            i = int(sp["seg"]["read"][s])
            ok += (int(sp["meta"]["seq_id"][s]) == tail["seq"][i] and abs(int(sp["meta"]["off"][s]) - int(tail["pos"][i])) <= 60)
        line.append((ln, len(sp["seg"]), ok))
    print("tails of 400 ONT reads (bases, segments, placed at the true locus): %s" % line)
    assert line[-1][2] >= line[0][2] and line[-1][2] >= 200


# ---------------------------------------------------------------------------------------------------------
# SAM
# ---------------------------------------------------------------------------------------------------------
def test_accaln_prints_supplementary_records(gpu, tmp_path):
    seqs = [synth.reference(110_000, seed=41), synth.reference(50_000, seed=42)]
    fa = tmp_path / "ref.fa"
    with open(fa, "wb") as f:
        for nm, s in zip((b"chrA", b"chrB"), seqs):
            f.write(b">" + nm + b"\n" + bytes(s) + b"\n")
    assert lib.lrm_accidx(str(fa).encode(), 32, 10, 1) == 0
    hi = index.HostIndex.read(str(fa))
    mta = hi.mta()
    a = synth.reads(seqs, 120, 1500, synth.ONT, seed=9)
    b = synth.reads(seqs, 120, 1000, synth.ONT, seed=10)
    reads, lens = _concat([[_piece(a, i), _piece(b, i)] if i % 4 else [_piece(a, i)] for i in range(120)])
    recs = [(b"q%d" % i, bytes(reads[i, :lens[i]]), bytes(33 + (i + j) % 40 for j in range(int(lens[i])))) for i in range(len(lens))]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@" + nm + b"\n" + s + b"\n+\n" + q + b"\n" for nm, s, q in recs))
    out = {}
    for name, opt in (("split", capi.map_options(anchored=1, clip=1, split=1)), ("clip", capi.map_options(anchored=1, clip=1)),
                      ("off", capi.map_options(anchored=1, clip=1, split=0, split_min_len=60))):
        sam = tmp_path / (name + ".sam")
        total, valid = C.c_uint64(), C.c_uint64()
        capi.check(lib.lrm_accaln_opt(str(fa).encode(), str(fq).encode(), str(sam).encode(), capi.Params(50, 20, 300),
                                      capi.GactParams(*GACT), gpu, 77, C.byref(total), C.byref(valid), C.byref(opt)), "lrm_accaln_opt")
        out[name] = (open(sam).read(), total.value, valid.value)
    assert out["off"][0] == out["clip"][0]
    assert out["split"][1:] == out["clip"][1:] and out["split"][1] == len(lens)
    di = index.DeviceIndex.upload(hi, gpu)
    try:
        buf = reads.copy()
        res = mapper.map_batch(di, buf, lens, clip=True)
        sp = mapper.split_batch(di, buf, lens, res)
    finally:
        di.close()
    want = sam_ref.header(mta, 77)
    reported = 0
    for i, (nm, s, q) in enumerate(recs):
        prim = dict(ops=mapper.ops_of(res, i), score=int(res["score"][i]), meta_r=int(res["meta_r"][i]), seq_id=int(res["meta"]["seq_id"][i]),
                    off=int(res["meta"]["off"][i]), strand=int(res["meta"]["strand"][i]))
        segs = [dict(start=int(sp["seg"]["start"][x]), len=int(sp["seg"]["len"][x]), flags=int(sp["seg"]["flags"][x]),
                     row=bytes(sp["rows"][x, :sp["seg"]["len"][x]]).decode(), ops=mapper.ops_of(sp, x), score=int(sp["score"][x]),
                     seq_id=int(sp["meta"]["seq_id"][x]), off=int(sp["meta"]["off"][x]), strand=int(sp["meta"]["strand"][x]))
                for x in np.flatnonzero(sp["seg"]["read"] == i)]
        reported += sum(bool(g["flags"] & split_ref.SEG_ALIGNED) for g in segs)
        want += split_ref.records(nm.decode(), bytes(buf[i, :lens[i]]).decode(), q.decode(), mta, prim, segs)
    got = out["split"][0]
    assert got == want
    lines = [ln.split("\t") for ln in got.splitlines() if ln[0] != "@"]
    assert len(lines) == len(lens) + reported and reported >= 60
    # SA:Z on both sides names the other record's place
    by_name = {}
    for ln in lines:
        by_name.setdefault(ln[0], []).append(ln)
    for group in by_name.values():
        if len(group) == 1:
            assert not group[0][-1].startswith("SA:Z")
            continue
        prim_entry = "%s,%s," % (group[0][2], group[0][3])
        for sup in group[1:]:
            assert int(sup[1]) & 2048 and sup[-1].startswith("SA:Z:" + prim_entry)
            assert "%s,%s,%s," % (sup[2], sup[3], "-" if int(sup[1]) & 16 else "+") in group[0][-1]
            assert len(sup[9]) == len(sup[10])
