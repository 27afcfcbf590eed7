"""Difference events on the GPU (docs/GACT_SPEC.md, "Difference events and MD:Z"): aln_diff_kernel on constructed stores at
every edge of its lanes and steps, every word against tests/md_ref.py; the capacity rule; the offsets scan; the stage behind
the three extension modes of DeviceMapper and behind the host pipeline's groups; what the other outputs must not notice; NM:i
and MD:Z of the accaln flow."""
import ctypes as C

import numpy as np
import pytest

import md_ref
import workloads
from longreadmapper_amd import capi, index, mapper, synth, textio
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu
GACT = (320, 120, 128)
SMALL = dict(lc_long_max=13)
ALPHABET = np.frombuffer(b"=XIDS", dtype=np.uint8)
FILL = 0xABABABAB
NO_ROOM = capi.DIFF_NO_ROOM


@pytest.fixture(scope="module")
def ont(gpu):
    sc = workloads.scenario("ont-2k")
    di = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL)
    yield sc, di, bytes(sc["hi"].content())
    di.close()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _want(row, content):
    ops, score, meta_r, loc = row[:4]
    if len(row) > 4 and row[4] is not None:
        ops = ops[:max(row[4], 0)]
    return md_ref.events(ops, content, loc, score, meta_r)


def _kernel_events(di, content, rows, stride, base_off, cap=None):
    """lrm_aln_diff_dev over rows = [(ops, score, meta_r, loc, n_ops or None)] laid out at `stride` from a base pointer moved by
    base_off bytes; every byte of the store that is not an op byte of a row is 'X'.  The offsets are the prefix sums of the
    reference's counts, the event buffer is filled with 0xAB.  -> (offsets, the whole buffer, the reference's events per row)"""
    import torch
    n = len(rows)
    flat = np.full(n * stride + base_off + 64, ord("X"), dtype=np.uint8)
    n_ops = np.zeros(n, dtype=np.int32)
    meta = np.zeros(n, dtype=mapper.META_DT)
    want = [_want(r, content) for r in rows]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(w) for w in want])
    for i, row in enumerate(rows):
        ops = row[0]
        assert len(ops) <= stride
        flat[base_off + i * stride:base_off + i * stride + len(ops)] = np.frombuffer(ops, dtype=np.uint8)
        n_ops[i] = len(ops) if len(row) < 5 or row[4] is None else row[4]
        meta["loc"][i] = row[3]
    total = int(off[n])
    cap = total if cap is None else cap
    d_store, d_n = torch.from_numpy(flat).cuda(), torch.from_numpy(n_ops).cuda()
    d_score = torch.from_numpy(np.array([r[1] for r in rows], dtype=np.int32)).cuda()
    d_mr = torch.from_numpy(np.array([r[2] for r in rows], dtype=np.int32)).cuda()
    d_meta = torch.from_numpy(meta.view(np.uint8).reshape(n, -1).copy()).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ev = torch.from_numpy(np.full(total + 64, FILL, dtype=np.uint32).view(np.int32)).cuda()
    capi.check(lib.lrm_aln_diff_dev(di.handle, d_store.data_ptr() + base_off, stride, d_n.data_ptr(), d_score.data_ptr(), d_mr.data_ptr(),
                                    d_meta.data_ptr(), n, d_off.data_ptr(), cap, d_ev.data_ptr(), _stream()), "lrm_aln_diff_dev")
    torch.cuda.synchronize()
    return off, d_ev.cpu().numpy().view(np.uint32), want


def _put(row, at, piece):
    assert 0 <= at and at + len(piece) <= len(row)
    return row[:at] + piece + row[at + len(piece):]


def _edge_rows():
    """Runs of 'D' that end on, start on and straddle columns 16 (a lane edge), 1024 and 2048 (step edges); 'D' and 'I' runs
    side by side across them; 'X' columns either side."""
    rows = []
    base = (b"=" * 7 + b"X") * 257
    base = base[:2049]
    for e in (16, 1024, 2048):
        for at, ln in ((e - 2, 4), (e - 3, 3), (e, 3), (e - 1, 1), (e, 1), (e - 1, 2), (e - 17, 34)):
            if 0 <= at and at + ln <= len(base):
                rows.append(_put(base, at, b"D" * ln))
        for piece in (b"DDII", b"IIDD", b"DID", b"XDX", b"DXD", b"DSD", b"DND"):
            for at in range(e - len(piece), e + 1):
                if at + len(piece) <= len(base):
                    rows.append(_put(base, at, piece))
    return rows


N_OPS = [0, 1, 15, 16, 17, 63, 64, 1023, 1024, 1025, 2049]


def _constructed_rows(content, stride):
    rng = np.random.default_rng(stride)
    L = len(content)
    rows = []
    for m in N_OPS:
        rows.append((bytes(rng.choice(ALPHABET, size=m, p=[0.6, 0.1, 0.1, 0.1, 0.1])), 5, 1))
        rows.append((bytes(rng.choice(ALPHABET, size=m)), 5, 1))
        rows += [(c * m, 5, 1) for c in (b"X", b"D", b"=", b"I", b"S")]
    rows += [(r, 3, 1) for r in _edge_rows()]
    rows = [r + (int(1000 + 37 * k),) for k, r in enumerate(rows)]                 # meta.loc at every residue mod 16
    assert {r[3] % 16 for r in rows} == set(range(16))
    live = bytes(rng.choice(ALPHABET, size=1500))
    span = sum(live.count(c) for c in b"=XD")
    rows += [(live, 5, 1, L - span),                                             # ends on the text's last byte
             (live, 5, 1, L - span + 1),                                         # ... and one beyond it: that base is 0
             (b"=" * 30 + b"XD", 5, 1, L - 20),                                   # its events lie beyond the text altogether
             # rows without an alignment between live rows: their store rows hold op bytes all the same
             (live, 5, 1, 77), (b"D" * 2000, 5, 0, 5), (live, 5, 1, 78), (b"X" * 2000, -1, 1, 5), (live, 7, 1, 79),
             (b"X" * 2000, 5, 1, 5, 0), (live, 0, 1, 80), (b"D" * 40, 5, 1, 5, -1), (live[:777], 5, 1, 81)]
    return rows


@pytest.mark.parametrize("stride,base_off", [(2052, 4), (2064, 0), (2051, 1)])
def test_kernel_on_constructed_stores(ont, stride, base_off):
    _, di, content = ont
    rows = _constructed_rows(content, stride)
    off, buf, want = _kernel_events(di, content, rows, stride, base_off)
    total = int(off[-1])
    assert (buf[total:] == FILL).all()                              # nothing at or beyond off[n]
    bad = [(i, len(rows[i][0])) for i in range(len(rows)) if buf[int(off[i]):int(off[i + 1])].tolist() != want[i]]
    assert not bad, (stride, base_off, len(bad), bad[:5])
    assert len(rows) > 150 and total > 20000
    k = [r[0] for r in rows].index(b"X" * 2049)
    ev = buf[int(off[k]):int(off[k + 1])]
    assert len(ev) == 2049 and not (ev >> 8).any()                  # all 'X': kind 0, no '=' before any
    assert bytes((ev & 0xFF).astype(np.uint8)) == content[rows[k][3]:rows[k][3] + 2049]
    k = [r[0] for r in rows].index(b"D" * 1025)
    ev = buf[int(off[k]):int(off[k + 1])]
    assert ((ev >> 8) & 3).tolist() == [1] + [2] * 1024


def test_capacity(ont):
    """cap in the middle of a read: the reads whose events end at or before cap are complete, the others leave the fill."""
    _, di, content = ont
    rows = _constructed_rows(content, 2064)
    full_off, _, want = _kernel_events(di, content, rows, 2064, 0)
    total = int(full_off[-1])
    k = next(i for i in range(len(rows) // 2, len(rows)) if len(want[i]) > 3)
    cap = int(full_off[k]) + len(want[k]) // 2
    off, buf, _ = _kernel_events(di, content, rows, 2064, 0, cap=cap)
    fitted = 0
    for i in range(len(rows)):
        got = buf[int(off[i]):int(off[i + 1])]
        if int(off[i + 1]) <= cap:
            assert got.tolist() == want[i], i
            fitted += len(want[i]) > 0
        else:
            assert (got == FILL).all(), i
    assert (buf[total:] == FILL).all() and fitted > 10 and (buf[int(full_off[k]):] == FILL).all()
    _, buf, _ = _kernel_events(di, content, rows, 2064, 0, cap=0)
    assert (buf == FILL).all()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025, 5000])
def test_offsets_scan(ont, n):
    import torch
    rng = np.random.default_rng(n)
    s = np.zeros(max(n, 1), dtype=mapper.SUMMARY_DT)
    s["n_x"][:n], s["n_del"][:n] = rng.integers(0, 1 << 20, n), rng.integers(0, 1 << 20, n)
    s["n_eq"], s["n_ins"] = 7, 9                                     # (not counted)
    if n >= 255:
        s["n_x"][3], s["n_del"][3], s["n_x"][n - 1] = 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF
    d_sum = torch.from_numpy(s.view(np.uint8).reshape(len(s), -1).copy()).cuda()
    d_off = torch.from_numpy(np.full(n + 2, 0x5555555555555555, dtype=np.int64)).cuda()
    capi.check(lib.lrm_aln_diff_offsets_dev(d_sum.data_ptr(), n, d_off.data_ptr(), _stream()), "lrm_aln_diff_offsets_dev")
    torch.cuda.synchronize()
    got = d_off.cpu().numpy().view(np.uint64)
    want = np.zeros(n + 1, dtype=np.uint64)
    want[1:] = np.cumsum(s["n_x"][:n].astype(np.uint64) + s["n_del"][:n].astype(np.uint64))
    assert np.array_equal(got[:n + 1], want) and got[n + 1] == 0x5555555555555555
    if n == 5000:
        assert int(want[-1]) > 1 << 32


# ---------------------------------------------------------------------------------------------------------
# the stage behind the extension modes
# ---------------------------------------------------------------------------------------------------------
MODES = {"classic": {}, "anchored": dict(anchored=True), "clip": dict(clip=True)}


def _device_run(di, gpu, sc, md, **kw):
    import torch
    n, stride = sc["reads"].shape
    dm = mapper.DeviceMapper(di, n, stride - 1, sc["seed_len"], sc["thres"], device=gpu, md=md, summary=True, **kw)
    d_reads = torch.from_numpy(sc["reads"]).cuda()
    d_lens = torch.from_numpy(sc["lens"].astype(np.int32)).cuda()
    dm.seed(d_reads, d_lens)
    dm.extend(d_reads, d_lens)
    torch.cuda.synchronize()
    res = dm.results(n)
    diff = dm.diff_records(n) if md else None
    dm.close()
    return res, d_reads.cpu().numpy(), diff


@pytest.fixture(scope="module")
def device_records(ont, gpu):
    """mode -> (results, reads as the extension left them, (offsets, events))"""
    sc, di, _ = ont
    di.set_map_options()
    return {mode: _device_run(di, gpu, sc, True, **kw) for mode, kw in MODES.items()}


def _ops(res, i):
    return bytes(res["ops"][i, :max(int(res["n_ops"][i]), 0)])


def _want_of(res, content, i):
    return md_ref.events(_ops(res, i), content, int(res["meta"]["loc"][i]), int(res["score"][i]), int(res["meta_r"][i]))


@pytest.mark.parametrize("mode", list(MODES))
def test_device_mapper_events(ont, gpu, device_records, mode):
    sc, di, content = ont
    res, reads_after, (off, ev) = device_records[mode]
    n = len(sc["lens"])
    s = res["summary"]
    assert np.array_equal(np.diff(off.astype(np.int64)), s["n_x"].astype(np.int64) + s["n_del"]) and off[0] == 0 and len(ev) == off[n]
    mapped = 0
    for i in range(n):
        got = ev[int(off[i]):int(off[i + 1])]
        assert got.tolist() == _want_of(res, content, i), (mode, i)
        ops, loc = _ops(res, i), int(res["meta"]["loc"][i])
        if not md_ref.aligned(ops, int(res["score"][i]), int(res["meta_r"][i])):
            assert len(got) == 0
            continue
        mapped += 1
        text = textio.md_text(got, int(s["n_eq"][i]))
        assert text == md_ref.md(ops, content, loc), (mode, i)
        span = sum(ops.count(c) for c in b"=XD")
        read = bytes(reads_after[i, :sc["lens"][i]])
        assert md_ref.target_from_md(read, md_ref.m_cigar(ops), text) == content[loc:loc + span], (mode, i)
    assert mapped > 50
    # a mapper without the stage: the same bytes everywhere else
    plain, plain_reads, _ = _device_run(di, gpu, sc, False, **MODES[mode])
    assert set(plain) == set(res)
    for key in plain:
        assert np.array_equal(plain[key], res[key]), key
    assert np.array_equal(plain_reads, reads_after)


# ---------------------------------------------------------------------------------------------------------
# the host boundary
# ---------------------------------------------------------------------------------------------------------
LAYOUTS = {"rows": {}, "dense": dict(dense_results=1), "text": dict(cigar_text=1), "text-keep": dict(cigar_text=1, keep_reads=1)}


def _same_outputs(a, b, reads_a, reads_b, what):
    for key in ("best", "n_ops", "score", "meta", "meta_r"):
        assert np.array_equal(a[key], b[key]), (what, key)
    assert a["is_text"] == b["is_text"] and ("ops_off" in a) == ("ops_off" in b)
    if "ops_off" in a:
        assert np.array_equal(a["ops_off"], b["ops_off"]), what
    for i in range(len(a["n_ops"])):
        if a["is_text"]:
            assert mapper.text_of(a, i) == mapper.text_of(b, i), (what, i)
        else:
            assert mapper.ops_of(a, i) == mapper.ops_of(b, i), (what, i)
    assert np.array_equal(reads_a, reads_b), what


def _same_events(res, want_off, want_ev, order=None, what=""):
    """every read's slice equals the device mapper's; the slices are disjoint and cover md_needed"""
    n = len(res["md_cnt"])
    spans = []
    for i in range(n):
        k = i if order is None else int(order[i])
        o, c = int(res["md_off"][i]), int(res["md_cnt"][i])
        assert o != NO_ROOM and c == int(want_off[k + 1]) - int(want_off[k]), (what, i)
        assert np.array_equal(res["md_events"][o:o + c], want_ev[int(want_off[k]):int(want_off[k + 1])]), (what, i)
        if c:
            spans.append((o, o + c))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), what
    assert res["md_needed"] == int(res["md_cnt"].sum()) == int(want_off[-1]), what
    assert not spans or spans[-1][1] <= res["md_needed"], what


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mode", ["classic", "clip"])
def test_map_batch_events(ont, device_records, layout, mode):
    sc, di, content = ont
    want_off, want_ev = device_records[mode][2]
    opts = dict(LAYOUTS[layout], sub_batches=3, group_subs=1)             # three extension groups
    kw = dict(clip=True) if mode == "clip" else {}
    r0 = sc["reads"].copy()
    plain = mapper.map_batch(di, r0, sc["lens"], sc["seed_len"], sc["thres"], options=opts, **kw)
    assert "md_off" not in plain
    for summary in (False, True):
        r1 = sc["reads"].copy()
        res = mapper.map_batch(di, r1, sc["lens"], sc["seed_len"], sc["thres"], options=opts, md=True, summary=summary, mapq=summary, **kw)
        _same_events(res, want_off, want_ev, what=(layout, mode, summary))
        assert ("summary" in res) == summary == ("mapq" in res)
        if summary:
            assert np.array_equal(res["summary"], device_records[mode][0]["summary"])
        _same_outputs(res, plain, r1, r0, (layout, mode, summary))
    if layout == "rows":
        for i in range(len(sc["lens"])):
            o, c = int(res["md_off"][i]), int(res["md_cnt"][i])
            want = md_ref.events(mapper.ops_of(res, i), content, int(res["meta"]["loc"][i]), int(res["score"][i]), int(res["meta_r"][i]))
            assert res["md_events"][o:o + c].tolist() == want, i


def test_group_handle_and_two_batches_in_flight(ont, gpu, device_records):
    sc, di, _ = ont
    want_off, want_ev = device_records["clip"][2]
    dg = index.DeviceIndex.upload_multi(sc["hi"], [gpu, gpu], **SMALL)
    try:
        r0, r1 = sc["reads"].copy(), sc["reads"].copy()
        plain = mapper.map_batch(dg, r0, sc["lens"], sc["seed_len"], sc["thres"], clip=True)
        res = mapper.map_batch(dg, r1, sc["lens"], sc["seed_len"], sc["thres"], clip=True, md=True, mapq=True)
        _same_events(res, want_off, want_ev, what="group")              # every share into the one buffer
        _same_outputs(res, plain, r1, r0, "group")
    finally:
        dg.close()
    # two batches in flight on one handle: the second is the first reversed, classic mode, text layout
    want_off, want_ev = device_records["classic"][2]
    order = np.arange(len(sc["lens"]))[::-1]
    ra, rb = sc["reads"].copy(), np.ascontiguousarray(sc["reads"][order])
    la, lb = sc["lens"], np.ascontiguousarray(sc["lens"][order])
    opts = dict(cigar_text=1, sub_batches=2, group_subs=1)
    pa = mapper.map_batch_submit(di, ra, la, sc["seed_len"], sc["thres"], options=opts, md=True)
    pb = mapper.map_batch_submit(di, rb, lb, sc["seed_len"], sc["thres"], options=opts, md=True, summary=True)
    pc = mapper.map_batch_submit(di, sc["reads"].copy(), la, sc["seed_len"], sc["thres"], options=opts)
    a, b, c = pa.wait(), pb.wait(), pc.wait()
    _same_events(a, want_off, want_ev, what="first")
    _same_events(b, want_off, want_ev, order=order, what="second")
    assert "md_off" not in c
    for i in range(len(la)):
        assert mapper.text_of(a, i) == mapper.text_of(c, i) == mapper.text_of(b, int(np.flatnonzero(order == i)[0]))


def test_capacity_below_the_need(ont, device_records):
    sc, di, _ = ont
    want_off, want_ev = device_records["classic"][2]
    need = int(want_off[-1])
    opts = dict(sub_batches=4, group_subs=1)
    for cap in (need - 1, need // 2, 0):
        res = mapper.map_batch(di, sc["reads"].copy(), sc["lens"], sc["seed_len"], sc["thres"], options=opts, md=True, md_cap=cap)
        assert res["md_needed"] == need                              # the wait returned 0 and the total is the batch's
        assert np.array_equal(res["md_cnt"], np.diff(want_off.astype(np.int64)))
        no_room = res["md_off"] == NO_ROOM
        assert no_room.any() and (cap > 0) == bool((~no_room).any())
        for i in np.flatnonzero(~no_room):
            o, c = int(res["md_off"][i]), int(res["md_cnt"][i])
            assert o + c <= cap and np.array_equal(res["md_events"][o:o + c], want_ev[int(want_off[i]):int(want_off[i + 1])]), (cap, i)
    res = mapper.map_batch(di, sc["reads"].copy(), sc["lens"], sc["seed_len"], sc["thres"], options=opts, md=True, md_cap=need)
    _same_events(res, want_off, want_ev, what="exact cap")


def test_pinned_event_buffer(ont, device_records):
    """events_out in pinned memory: every group's events are copied straight into it, no staging ring."""
    sc, di, _ = ont
    want_off, want_ev = device_records["clip"][2]
    need = int(want_off[-1])
    ev = mapper.pinned_empty(need + 16, np.uint32)
    try:
        ev[:] = FILL
        res = mapper.map_batch(di, sc["reads"].copy(), sc["lens"], sc["seed_len"], sc["thres"], options=dict(cigar_text=1, sub_batches=3, group_subs=1),
                               clip=True, md=True, md_cap=need, md_events=ev)
        assert res["md_events"] is ev
        _same_events(res, want_off, want_ev, what="pinned")
        assert (ev[need:] == FILL).all()
    finally:
        mapper.pinned_free(ev)


# ---------------------------------------------------------------------------------------------------------
# the accaln flow
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flow_files(gpu, tmp_path_factory):
    """The 150-read set-up of test_accaln_sam_matches_oracle: two sequences, a read shorter than a seed."""
    tmp = tmp_path_factory.mktemp("md")
    seqs = [synth.reference(90_000, seed=31), synth.reference(40_000, seed=32)]
    fa = tmp / "ref.fa"
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
    fq = tmp / "reads.fq"
    with open(fq, "wb") as f:
        for i in range(len(lens)):
            s = bytes(r["reads"][i, :lens[i]])
            f.write(b"@read%d extra\n" % i + s + b"\n+\n" + bytes([33 + (i + j) % 40 for j in range(len(s))]) + b"\n")
    reads = np.zeros((len(lens), int(lens.max()) + 1), dtype=np.uint8)
    for i, l in enumerate(lens):
        reads[i, :l] = r["reads"][i, :l]
    hi = index.HostIndex.read(str(fa))
    di = index.DeviceIndex.upload(hi, gpu, **SMALL)
    yield tmp, fa, fq, reads, lens, bytes(hi.content()), di
    di.close()


@pytest.mark.parametrize("mode,mapq", [("classic", 0), ("clip", 1)])
def test_accaln_md(flow_files, gpu, mode, mapq):
    tmp, fa, fq, reads, lens, content, di = flow_files
    opt = capi.map_options(anchored=1, clip=1) if mode == "clip" else None
    total, valid = C.c_uint64(), C.c_uint64()
    head = (str(fa).encode(), str(fq).encode())
    tail = (capi.Params(64, 20, 300), capi.GactParams(*GACT), gpu, 7, C.byref(total), C.byref(valid), C.byref(opt) if opt is not None else None, mapq)
    # md off: byte for byte the file of the flow that was there before
    capi.check(lib.lrm_accaln_mapq(*head, str(tmp / "old.sam").encode(), *tail), "lrm_accaln_mapq")
    capi.check(lib.lrm_accaln_md(*head, str(tmp / "off.sam").encode(), *tail, 0), "lrm_accaln_md")
    old = open(tmp / "old.sam").read()
    assert open(tmp / "off.sam").read() == old
    assert textio.accaln(str(fa), str(fq), str(tmp / "on.sam"), 64, gact=GACT, device=gpu, rg_id=7, options=opt, mapq=mapq, md=True)[0] == 150
    on = open(tmp / "on.sam").read()
    # the reference: the same reads through map_batch (op bytes in rows), md_ref over them
    res = mapper.map_batch(di, reads.copy(), lens, 20, 300, GACT, options={}, **(dict(clip=True) if mode == "clip" else {}))
    body, plain = on.splitlines(), old.splitlines()
    assert len(body) == len(plain) and [l for l in body if l.startswith("@")] == [l for l in plain if l.startswith("@")]
    body, plain = [l for l in body if not l.startswith("@")], [l for l in plain if not l.startswith("@")]
    assert len(body) == 150
    tagged = 0
    for i, (a, b) in enumerate(zip(body, plain)):
        ops = mapper.ops_of(res, i)
        want = md_ref.md(ops, content, int(res["meta"]["loc"][i]), int(res["score"][i]), int(res["meta_r"][i]))
        if want is None:
            assert a == b and "MD:Z" not in a, i
            continue
        assert a == b + "\tNM:i:%d\tMD:Z:%s" % (md_ref.nm(ops), want), (mode, i)
        tagged += 1
    assert tagged > 120
