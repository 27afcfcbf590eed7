"""Alignment summary records on the GPU (docs/GACT_SPEC.md, "Alignment summary and PAF"): aln_summary_kernel on constructed
stores at every edge of its lanes and steps, every field against tests/aln_summary_ref.py; the stage behind the three
extension modes of DeviceMapper and behind the host pipeline's groups; what the other outputs must not notice; the PAF flow
against lines printed from the oracle's results."""
import ctypes as C

import numpy as np
import pytest

import aln_summary_ref as ref
import anchored_ref
import clip_ref
import orc
import workloads
from longreadmapper_amd import capi, index, mapper, synth
from longreadmapper_amd.capi import lib

pytestmark = pytest.mark.gpu
GACT = (320, 120, 128)
SMALL = dict(lc_long_max=13)
ALPHABET = np.frombuffer(b"=XIDS", dtype=np.uint8)


def _same_records(got, rows, what=""):
    """got: SUMMARY_DT records; rows: [(ops, score, meta_r)]"""
    assert len(got) == len(rows)
    bad = []
    for i, (ops, score, meta_r) in enumerate(rows):
        want = ref.record(ops, score, meta_r)
        have = {f: int(got[f][i]) for f in ref.FIELDS}
        if have != want:
            bad.append((i, len(ops), have, want))
    assert not bad, (what, len(bad), bad[:3])


@pytest.fixture(scope="module")
def ont(gpu):
    sc = workloads.scenario("ont-2k")
    di = index.DeviceIndex.upload(sc["hi"], gpu, **SMALL)
    yield sc, di
    di.close()


def _kernel_records(di, rows, stride, base_off):
    """lrm_aln_summary_dev over rows = [(ops, score, meta_r, n_ops or None)] laid out at `stride` from a base pointer moved by
    base_off bytes; every byte of the store that is not an op byte of a row is 'I'."""
    import torch
    n = len(rows)
    flat = np.full(n * stride + base_off + 64, ord("I"), dtype=np.uint8)
    n_ops = np.zeros(n, dtype=np.int32)
    for i, row in enumerate(rows):
        ops = row[0]
        assert len(ops) <= stride
        flat[base_off + i * stride:base_off + i * stride + len(ops)] = np.frombuffer(ops, dtype=np.uint8)
        n_ops[i] = len(ops) if len(row) < 4 or row[3] is None else row[3]
    d_store = torch.from_numpy(flat).cuda()
    d_n = torch.from_numpy(n_ops).cuda()
    d_score = torch.from_numpy(np.array([r[1] for r in rows], dtype=np.int32)).cuda()
    d_mr = torch.from_numpy(np.array([r[2] for r in rows], dtype=np.int32)).cuda()
    d_out = torch.full((n + 1, 32), 0xAB, dtype=torch.uint8, device="cuda")
    capi.check(lib.lrm_aln_summary_dev(di.handle, d_store.data_ptr() + base_off, stride, d_n.data_ptr(), d_score.data_ptr(),
                                       d_mr.data_ptr(), n, d_out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "lrm_aln_summary_dev")
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[n] == 0xAB).all()                                   # nothing behind the last record
    return out[:n].reshape(-1).view(mapper.SUMMARY_DT)


def _put(row, at, piece):
    assert 0 <= at and at + len(piece) <= len(row)
    return row[:at] + piece + row[at + len(piece):]


def _edge_rows():
    """Every kind of run straddling, ending on and starting on column 16 (a lane edge) and column 1024 (a step edge)."""
    rows = []
    base = (b"=" * 7 + b"X") * 257
    base = base[:2049]
    for e in (16, 1024, 2048):
        for op in (b"I", b"D"):
            for at, ln in ((e - 2, 4), (e - 3, 3), (e, 3), (e - 1, 1), (e, 1), (e - 1, 2)):
                if at + ln <= len(base):
                    rows.append(_put(base, at, op * ln))
            # two runs a column apart across the edge, and a foreign byte between two runs
            rows.append(_put(base, e - 2, op + op + b"=" + op)[:2049] if e + 2 <= 2049 else base)
            rows.append(_put(base, e - 1, op + b"=" + op)[:2049] if e + 2 <= 2049 else base)
            rows.append(_put(base, e - 1, op + b"N")[:2049] if e + 1 <= 2049 else base)
        for at in (e - 3, e - 2, e - 1, e):                        # a 'D' run directly followed by an 'I' run, and the reverse
            if at + 4 <= len(base):
                rows.append(_put(base, at, b"DDII"))
                rows.append(_put(base, at, b"IIDD"))
                rows.append(_put(base, at + 1, b"DI"))
        for k in (e - 1, e, e + 1):                                # the end of the left 'S' run, the start of the right one
            if k <= len(base):
                rows.append(b"S" * k + base[k:])
                rows.append(base[:k] + b"S" * (len(base) - k))
                if k + 5 <= len(base):
                    rows.append(b"S" * k + base[k:len(base) - 5] + b"S" * 5)
    return rows


N_OPS = [0, 1, 15, 16, 17, 63, 64, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize("stride,base_off", [(2052, 4), (2064, 0), (2051, 1)])
def test_kernel_on_constructed_stores(ont, stride, base_off):
    """Rows at 4-byte but not 16-byte boundaries from a base moved by 4; aligned rows; rows at odd addresses."""
    _, di = ont
    rng = np.random.default_rng(stride)
    rows = []
    for m in N_OPS:
        rows.append((bytes(rng.choice(ALPHABET, size=m, p=[0.6, 0.1, 0.1, 0.1, 0.1])), 5, 1))
        rows.append((bytes(rng.choice(ALPHABET, size=m)), 5, 1))
        rows.append((b"I" * m, 5, 1))
        rows.append((b"S" * m, 5, 1))
        rows.append((b"S" * (m // 2) + b"=" * (m - m // 2), 0, 1))
    rows += [(r, 3, 1) for r in _edge_rows()]
    # rows without an alignment between live rows: their store rows hold op bytes all the same
    live = bytes(rng.choice(ALPHABET, size=1500))
    rows += [(live, 5, 1), (b"I" * 2000, 5, 0), (live, 5, 1), (b"D" * 2000, -1, 1), (live, 7, 1), (b"X" * 2000, 5, 1, 0), (live, 0, 1),
             (b"=" * 40, 5, 1, -1), (live[:777], 5, 1)]
    got = _kernel_records(di, rows, stride, base_off)
    want_rows = [(r[0] if len(r) < 4 else b"", r[1], r[2]) for r in rows]
    _same_records(got, want_rows, (stride, base_off))
    assert len(rows) > 150
    # spot checks by hand
    k = rows.index((b"I" * 2049, 5, 1))
    assert (got["n_ins"][k], got["ins_runs"][k], got["clip_left"][k], got["clip_right"][k]) == (2049, 1, 0, 0)
    k = rows.index((b"S" * 1025, 5, 1))
    assert (got["clip_left"][k], got["clip_right"][k], got["n_eq"][k]) == (1025, 0, 0)


def test_kernel_does_not_read_past_a_row(ont):
    """300 rows of random lengths up to 3 000, the bytes behind n_ops in every row filled with 'I'."""
    _, di = ont
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(0, 3001, 296)] + [3000, 2999, 1, 0]
    rows = [(bytes(rng.choice(ALPHABET, size=m, p=[0.7, 0.08, 0.08, 0.08, 0.06])), 2, 1) for m in lengths]
    got = _kernel_records(di, rows, 3004, 0)
    _same_records(got, rows, "random batch")
    assert int(got["n_ins"].sum()) == sum(r[0].count(b"I") for r in rows)
    # a prefix of every row: the rest of the row's own op bytes is behind n_ops now
    cut = [(r[0], 2, 1, len(r[0]) * 2 // 3) for r in rows]
    got = _kernel_records(di, cut, 3004, 0)
    _same_records(got, [(r[0][:r[3]], 2, 1) for r in cut], "prefixes")


# ---------------------------------------------------------------------------------------------------------
# the stage behind the extension modes
# ---------------------------------------------------------------------------------------------------------
MODES = {"classic": {}, "anchored": dict(anchored=True), "clip": dict(clip=True)}


def _device_run(di, gpu, sc, summary, **kw):
    import torch
    n, stride = sc["reads"].shape
    dm = mapper.DeviceMapper(di, n, stride - 1, sc["seed_len"], sc["thres"], device=gpu, summary=summary, **kw)
    d_reads = torch.from_numpy(sc["reads"]).cuda()
    d_lens = torch.from_numpy(sc["lens"].astype(np.int32)).cuda()
    dm.seed(d_reads, d_lens)
    dm.extend(d_reads, d_lens)
    torch.cuda.synchronize()
    res = dm.results(n)
    if summary:
        assert np.array_equal(dm.summary_records(n), res["summary"])
    dm.stats()
    dm.close()
    return res, d_reads.cpu().numpy()


def _rows_of(res):
    return [(bytes(res["ops"][i, :max(int(res["n_ops"][i]), 0)]), int(res["score"][i]), int(res["meta_r"][i])) for i in range(len(res["n_ops"]))]


@pytest.fixture(scope="module")
def device_records(ont, gpu):
    """mode -> (results with summary, reads as the extension left them)"""
    sc, di = ont
    di.set_map_options()
    return {mode: _device_run(di, gpu, sc, True, **kw) for mode, kw in MODES.items()}


@pytest.mark.parametrize("mode", list(MODES))
def test_device_mapper_records(ont, gpu, device_records, mode):
    sc, di = ont
    res, reads_after = device_records[mode]
    s = res["summary"]
    _same_records(s, _rows_of(res), mode)
    mapped = (res["meta_r"] != 0) & (res["score"] != -1)
    assert mapped.sum() > 50
    nm = s["n_x"].astype(np.int64) + s["n_ins"] + s["n_del"]
    assert np.array_equal(nm[mapped], res["score"][mapped])
    assert not any(s[f][~mapped].any() for f in ref.FIELDS)
    q = s["clip_left"].astype(np.int64) + s["n_eq"] + s["n_x"] + s["n_ins"] + s["clip_right"]
    assert np.array_equal(q[mapped], sc["lens"][mapped])                       # every query base is in exactly one column
    if mode == "clip":
        assert np.array_equal(s["clip_left"], res["clip"]["left"]) and np.array_equal(s["clip_right"], res["clip"]["right"])
    else:
        assert not s["clip_left"].any() and not s["clip_right"].any()
    # a mapper without the stage: the same bytes everywhere else
    plain, plain_reads = _device_run(di, gpu, sc, False, **MODES[mode])
    assert "summary" not in plain
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


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mode", ["classic", "clip"])
def test_map_batch_records(ont, device_records, layout, mode):
    sc, di = ont
    want = device_records[mode][0]["summary"]
    opts = dict(LAYOUTS[layout], sub_batches=3, group_subs=1)             # three extension groups
    kw = dict(clip=True) if mode == "clip" else {}
    r0 = sc["reads"].copy()
    plain = mapper.map_batch(di, r0, sc["lens"], sc["seed_len"], sc["thres"], options=opts, **kw)
    assert "summary" not in plain
    for mapq in (False, True):
        r1 = sc["reads"].copy()
        res = mapper.map_batch(di, r1, sc["lens"], sc["seed_len"], sc["thres"], options=opts, summary=True, mapq=mapq, **kw)
        assert np.array_equal(res["summary"], want), (layout, mode, mapq)
        assert ("mapq" in res) == mapq
        _same_outputs(res, plain, r1, r0, (layout, mode, mapq))
    if layout == "rows":
        _same_records(res["summary"], [(mapper.ops_of(res, i), int(res["score"][i]), int(res["meta_r"][i])) for i in range(len(sc["lens"]))])
    if mapq:
        r2 = sc["reads"].copy()
        only = mapper.map_batch(di, r2, sc["lens"], sc["seed_len"], sc["thres"], options=opts, mapq=True, **kw)
        assert np.array_equal(only["mapq"], res["mapq"]) and "summary" not in only


def test_group_handle_and_two_batches_in_flight(ont, gpu, device_records):
    sc, di = ont
    want = device_records["clip"][0]["summary"]
    dg = index.DeviceIndex.upload_multi(sc["hi"], [gpu, gpu], **SMALL)
    try:
        r0, r1 = sc["reads"].copy(), sc["reads"].copy()
        plain = mapper.map_batch(dg, r0, sc["lens"], sc["seed_len"], sc["thres"], clip=True)
        res = mapper.map_batch(dg, r1, sc["lens"], sc["seed_len"], sc["thres"], clip=True, summary=True, mapq=True)
        assert np.array_equal(res["summary"], want)                          # every share written in place
        _same_outputs(res, plain, r1, r0, "group")
    finally:
        dg.close()
    # two batches in flight on one handle: the second is the first reversed, classic mode, text layout
    want = device_records["classic"][0]["summary"]
    order = np.arange(len(sc["lens"]))[::-1]
    ra, rb = sc["reads"].copy(), np.ascontiguousarray(sc["reads"][order])
    la, lb = sc["lens"], np.ascontiguousarray(sc["lens"][order])
    opts = dict(cigar_text=1, sub_batches=2, group_subs=1)
    pa = mapper.map_batch_submit(di, ra, la, sc["seed_len"], sc["thres"], options=opts, summary=True)
    pb = mapper.map_batch_submit(di, rb, lb, sc["seed_len"], sc["thres"], options=opts, summary=True, mapq=True)
    pc = mapper.map_batch_submit(di, sc["reads"].copy(), la, sc["seed_len"], sc["thres"], options=opts)
    a, b, c = pa.wait(), pb.wait(), pc.wait()
    assert np.array_equal(a["summary"], want) and np.array_equal(b["summary"], want[order]) and "summary" not in c
    for i in range(len(la)):
        assert mapper.text_of(a, i) == mapper.text_of(c, i) == mapper.text_of(b, int(np.flatnonzero(order == i)[0]))


# ---------------------------------------------------------------------------------------------------------
# the PAF flow
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flow_files(gpu, tmp_path_factory):
    """The 150-read set-up of test_accaln_sam_matches_oracle: two sequences, a read shorter than a seed."""
    tmp = tmp_path_factory.mktemp("paf")
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
    rng = np.random.default_rng(2)
    for i in range(5, 150, 6):                     # ends that do not align: the clipped run has something to clip
        k = int(lens[i]) // 4
        r["reads"][i, :k] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, k)]
    fq = tmp / "reads.fq"
    with open(fq, "wb") as f:
        for i in range(len(lens)):
            s = bytes(r["reads"][i, :lens[i]])
            f.write(b"@read%d extra\n" % i + s + b"\n+\n" + bytes([33 + (i + j) % 40 for j in range(len(s))]) + b"\n")
    hi = index.HostIndex.read(str(fa))
    return tmp, fa, fq, r["reads"], lens, hi, orc.OracleIndex.from_host_index(hi)


@pytest.mark.parametrize("mode", ["classic", "clip"])
def test_accaln_paf_matches_oracle(flow_files, gpu, mode):
    tmp, fa, fq, all_reads, lens, hi, oi = flow_files
    mta = hi.mta()
    pairs = [(o, l) for _, o, l in mta]
    paf = tmp / ("out-%s.paf" % mode)
    total, valid = C.c_uint64(), C.c_uint64()
    opt = capi.map_options(anchored=1, clip=1) if mode == "clip" else None
    capi.check(lib.lrm_accaln_paf(str(fa).encode(), str(fq).encode(), str(paf).encode(), capi.Params(64, 20, 300), capi.GactParams(*GACT),
                                  gpu, C.byref(total), C.byref(valid), C.byref(opt) if opt is not None else None, 0), "lrm_accaln_paf")
    got = open(paf).read()
    want, n_valid = "", 0
    for lo in range(0, len(lens), 64):             # the oracle per batch, exactly like the host loop
        bl = lens[lo:lo + 64]
        reads = np.zeros((len(bl), int(bl.max()) + 1), dtype=np.uint8)
        for i, l in enumerate(bl):
            reads[i, :l] = all_reads[lo + i, :l]
        best, _ = oi.seed_batch(reads, bl)
        ext = oi.extend_batch(reads, bl, best, GACT)
        anc = clip_ref.extend_clipped_batch(hi.content(), pairs, reads, bl, ext["meta"], ext["meta_r"], GACT) if mode == "clip" else None
        for i, l in enumerate(bl):
            ops, score, off = bytes(ext["ops"][i, :max(int(ext["n_ops"][i]), 0)]), int(ext["score"][i]), int(ext["meta"]["off"][i])
            if anc is not None and anc[i] is not None:
                ops, score, off = anc[i]["ops"], int(anc[i]["score"]), int(anc[i]["off"])
            sid = int(ext["meta"]["seq_id"][i])
            want += ref.paf_line("read%d" % (lo + i), int(l), int(ext["meta"]["strand"][i]), mta[sid][0], mta[sid][2], off, ops, score,
                                 int(ext["meta_r"][i]))
            n_valid += int(score >= 0 and ext["meta_r"][i] != 0)
    assert got == want, next((a, b) for a, b in zip(got.splitlines() + [""], want.splitlines() + [""]) if a != b)
    assert total.value == len(lens) and valid.value == n_valid
    lines = [l.split("\t") for l in got.splitlines()]
    assert len(lines) > 120 and not got.startswith("@")
    for f in lines:
        qlen, qs, qe, tlen, ts, te = int(f[1]), int(f[2]), int(f[3]), int(f[6]), int(f[7]), int(f[8])
        assert 0 <= qs < qe <= qlen and ts <= te <= tlen, f[:12]
        assert int(f[9]) <= int(f[10]) and f[11] == "255"
    assert sum(f[4] == "-" for f in lines) > 20
    if mode == "clip":
        assert sum(int(f[2]) > 0 or int(f[3]) < int(f[1]) for f in lines) > 15


def test_accaln_paf_with_mapq_and_refusal(flow_files, gpu):
    tmp, fa, fq, _, lens, _, _ = flow_files
    total, valid = C.c_uint64(), C.c_uint64()
    args = (str(fa).encode(), str(fq).encode())
    tail = (capi.Params(64, 20, 300), capi.GactParams(*GACT), gpu, C.byref(total), C.byref(valid))
    capi.check(lib.lrm_accaln_paf(*args, str(tmp / "mq.paf").encode(), *tail, None, 1), "lrm_accaln_paf")
    capi.check(lib.lrm_accaln_paf(*args, str(tmp / "plain.paf").encode(), *tail, None, 0), "lrm_accaln_paf")
    mq, plain = open(tmp / "mq.paf").read().splitlines(), open(tmp / "plain.paf").read().splitlines()
    assert len(mq) == len(plain) > 120
    for a, b in zip(mq, plain):
        fa_, fb = a.split("\t"), b.split("\t")
        assert fa_[:11] == fb[:11] and fa_[12:17] == fb[12:17] and 0 <= int(fa_[11]) <= 60
        assert fa_[17].startswith("v1:i:") and fa_[18].startswith("v2:i:") and len(fb) == 17
    opt = capi.map_options(anchored=1, clip=1, split=1)
    rc = lib.lrm_accaln_paf(*args, str(tmp / "split.paf").encode(), *tail, C.byref(opt), 0)
    assert rc == -1 and b"split" in lib.lrm_last_error()
