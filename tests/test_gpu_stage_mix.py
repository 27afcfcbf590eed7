"""Every stage on one mapper and on one file (tests/stage_mix.py; the premises: tests/test_stage_mix_cpu.py).

Mapping quality, the clipped extension, split, secondary, summary, difference events and pileup each have a test that switches
that stage on alone.  Here one DeviceMapper has all of them on, over reads that are at once a secondary candidate and the
source of segments, and every output it returns is compared -- byte for byte -- with the mapper that has only that stage, and
with the CPU references: in both orders of the second passes, with and without a segment workspace, in chunks, on a used
mapper, and next to a second pass that failed for lack of room.  Then the host second passes over one map_batch result, in both
orders and three layouts, against the device path; the file flow with split and secondary on together against the flows that
have one of them; and the refusal of a rival walk over survivor lists that are no longer the batch's.

What is compared of an output is every byte the contract defines: op rows up to n_ops, gathered rows up to their length,
lrm_seq_meta of the rows with a locus (include/lrm_accel.h, "Written extents")."""
import ctypes as C

import numpy as np
import pytest

import aln_summary_ref
import pileup_ref
import sam_ref
import stage_mix as S
from longreadmapper_amd import capi, index, mapper, synth, textio
from longreadmapper_amd.capi import lib
from longreadmapper_amd.records import ENTRY_DT

pytestmark = pytest.mark.gpu
MAPQ_FIELDS = ("n1", "n2", "radius", "mapq", "phase", "flags")
ANCHOR_FIELDS = ("text_pos", "read_pos", "len", "delta", "left_ops", "flags")
META_FIELDS = ("loc", "off", "seq_id", "strand")
STALE = "did not run the seed stage of this batch with the phase output"


@pytest.fixture(scope="module")
def world(gpu):
    w = S.world()
    ref = S.references()
    di = index.DeviceIndex.upload(w["hi"], gpu, **S.SMALL)
    yield w, ref, di
    di.close()


def _full(w, **more):
    return dict(mapq=True, clip=True, split=True, secondary=True, summary=True, md=True, pileup=(0, w["con_len"]), **more)


def _solo(w):
    """a mapper per stage, with only what that stage needs (the clipped extension is what the full mapper extends with)"""
    return {"clip": dict(clip=True), "mapq": dict(clip=True, mapq=True), "summary": dict(clip=True, summary=True),
            "md": dict(clip=True, md=True), "pileup": dict(clip=True, pileup=(0, w["con_len"])),
            "split": dict(clip=True, split=True), "secondary": dict(clip=True, mapq=True, secondary=True)}


# ---------------------------------------------------------------------------------------------------------------------
# running a mapper, and everything it returns
# ---------------------------------------------------------------------------------------------------------------------
def _upload(rows, shift=0):
    """the rows in device memory behind a base moved `shift` bytes into its allocation -> (the allocation, the (n, stride) view)"""
    import torch
    n, stride = rows.shape
    alloc = torch.zeros(shift + n * stride, dtype=torch.uint8, device="cuda")
    view = alloc[shift:].view(n, stride)
    view.copy_(torch.from_numpy(rows).cuda())
    return alloc, view


def _defined(g, k):
    """The defined bytes of an extension's outputs for k rows (g: name -> array, `ops` in rows) -> {name: bytes}"""
    n_ops, meta_r = np.asarray(g["n_ops"][:k]), np.asarray(g["meta_r"][:k])
    on = meta_r != 0
    out = dict(n_ops=n_ops.tobytes(), score=np.asarray(g["score"][:k]).tobytes(), meta_r=meta_r.tobytes(),
               meta=b"".join(np.ascontiguousarray(g["meta"][f][:k][on]).tobytes() for f in META_FIELDS),
               ops=b"".join(bytes(g["ops"][i, :max(int(n_ops[i]), 0)]) for i in range(k)))
    for name in ("anchor", "clip", "best", "mapq", "summary"):
        if name in g:
            out[name] = np.ascontiguousarray(g[name][:k]).tobytes()
    return out


def _rows_of(rows, lens):
    return b"".join(bytes(rows[s, :int(lens[s])]) for s in range(len(lens)))


def _collect(dm, n, alloc):
    """Everything mapper dm returns for its last batch -> ({name: bytes}, {name: arrays})"""
    res = dm.results(n)
    sp = res.pop("split", None)
    snap = {"res." + k: v for k, v in _defined(res, n).items()}
    objs = dict(res=res, reads=alloc.cpu().numpy())
    snap["reads"] = objs["reads"].tobytes()
    if dm.diff_off is not None:
        off, ev = dm.diff_records(n)
        objs["diff"] = (off, ev)
        snap["diff.off"], snap["diff.events"] = off.tobytes(), ev.tobytes()
    if dm.pileup is not None:
        objs["pileup"] = dm.pileup_columns()
        snap["pileup"] = objs["pileup"].tobytes()
    if sp is not None:
        k = len(sp["seg"])
        objs["split"] = sp
        snap.update({"split." + name: v for name, v in _defined(sp, k).items()})
        snap["split.seg"], snap["split.lens"] = sp["seg"].tobytes(), sp["lens"].tobytes()
        snap["split.rows"] = _rows_of(sp["rows"], sp["lens"])
    if dm.sec is not None:
        sec = dm.secondary_results()
        k = len(sec["table"])
        objs["secondary"] = sec
        snap.update({"secondary." + name: v for name, v in _defined(sec, k).items()})
        snap["secondary.table"], snap["secondary.lens"], snap["secondary.rival"] = sec["table"].tobytes(), sec["lens"].tobytes(), sec["rival"].tobytes()
        snap["secondary.rows"] = _rows_of(sec["rows"], sec["lens"])
        assert not any(sec["rows"][s, int(sec["lens"][s]):].any() for s in range(k)), "secondary rows: zeros behind the read"
    return snap, objs


def _stages(dm, rows, lens, order=(), shift=0):
    """seed, extend, then the second passes in `order` over the rows at a moved base; stats() behind every stage raises if a
    kernel set the workspace's error word -> (snapshot, objects, the read buffer as the extension left it)"""
    import torch
    n = len(lens)
    alloc, d_reads = _upload(rows, shift)
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    dm.seed(d_reads, d_lens, n)
    torch.cuda.synchronize()
    dm.stats()
    assert np.array_equal(d_reads.cpu().numpy(), rows), "the seed stage wrote into the read buffer"
    dm.extend(d_reads, d_lens, n)
    torch.cuda.synchronize()
    dm.stats()
    extended = alloc.cpu().numpy()
    for stage in order:
        k = dm.split(d_reads, d_lens, n) if stage == "split" else dm.secondary(d_reads, d_lens, n)
        torch.cuda.synchronize()
        dm.stats()
        assert k > 0
    snap, objs = _collect(dm, n, alloc)
    assert np.array_equal(objs["reads"], extended), "a second pass moved the read buffer"
    return snap, objs, extended


def _fresh(world, gpu, kw, order=(), shift=0):
    w, ref, di = world
    dm = mapper.DeviceMapper(di, w["n"], S.MAX_LEN, device=gpu, **kw)
    try:
        return _stages(dm, w["reads"], w["lens"], order, shift)
    finally:
        dm.close()


@pytest.fixture(scope="module")
def solo(world, gpu):
    """the snapshot of every solo mapper over the batch, computed once"""
    w, ref, di = world
    di.set_map_options()
    order = {"split": ("split",), "secondary": ("secondary",)}
    return {name: _fresh(world, gpu, kw, order.get(name, ()))[0] for name, kw in _solo(w).items()}


def _same_as_solo(full, solo, stages=None, skip=()):
    """every output a solo mapper returns is what the full mapper returns under the same name; together they are all of it"""
    seen = set()
    for name in stages or solo:
        for key, want in solo[name].items():
            if key.split(".")[0] in skip:
                continue
            assert key in full and full[key] == want, ("full mapper", key, "differs from the mapper with only", name)
            seen.add(key)
    if stages is None:
        assert all(len(v) > 0 for v in full.values()), [k for k, v in full.items() if not len(v)]
        assert seen =={k for k in full if k.split(".")[0] not in skip}, sorted(set(full) - seen)


# ---------------------------------------------------------------------------------------------------------------------
# against the references of tests/stage_mix.py
# ---------------------------------------------------------------------------------------------------------------------
def _ext_is(g, k, want, what):
    for f in ("meta_r", "n_ops", "score"):
        assert np.array_equal(g[f][:k], want[f]), (what, f, np.flatnonzero(g[f][:k] != want[f])[:6].tolist())
    on = want["meta_r"] != 0
    for f in META_FIELDS:
        assert np.array_equal(g["meta"][f][:k][on].astype(np.int64), np.asarray(want[f])[on].astype(np.int64)), (what, "meta", f)
    for i in range(k):
        assert bytes(g["ops"][i, :max(int(want["n_ops"][i]), 0)]) == want["ops"][i], (what, "ops of row", i)
    for c, f in enumerate(ANCHOR_FIELDS):
        assert np.array_equal(g["anchor"][f][:k].astype(np.int64), want["anchor"][:, c]), (what, "anchor", f)
    assert np.array_equal(g["clip"]["left"][:k], want["clip_left"]) and np.array_equal(g["clip"]["right"][:k], want["clip_right"]), (what, "clip")


def _is_the_reference(objs, ref, rows, lens, shift, pileup_of=None):
    n = len(lens)
    res = objs["res"]
    for f in ("key", "val", "bucket"):
        assert np.array_equal(res["best"][f], ref["best"][f]), ("best", f)
    for f in MAPQ_FIELDS:
        assert np.array_equal(res["mapq"][f], ref["mapq"][f]), ("mapq", f)
    _ext_is(res, n, ref["clipped"], "primary")
    for f in aln_summary_ref.FIELDS:
        assert np.array_equal(res["summary"][f], [s[f] for s in ref["summary"]]), ("summary", f)
    off, ev = objs["diff"]
    assert np.array_equal(off, ref["diff_off"]) and np.array_equal(ev, ref["diff_events"]), "difference events"
    want_cols = (pileup_of or ref["pileup"]).columns()
    assert pileup_ref.same(objs["pileup"], want_cols), ("pileup", pileup_ref.first_difference(objs["pileup"], want_cols))
    # the read buffer: the reverse-strand reads turned round, every other byte as it was
    want_rows = rows.copy()
    for i in range(n):
        want_rows[i, :lens[i]] = ref["oriented"][i, :lens[i]]
    assert not objs["reads"][:shift].any() and np.array_equal(objs["reads"][shift:].reshape(rows.shape), want_rows), "read buffer"
    # split
    sp, want = objs["split"], ref["split"]
    k = len(want["table"])
    assert len(sp["seg"]) == k
    reported = (want["ext"]["meta_r"] != 0) & ((want["ext"]["anchor"][:, 5] & capi.ANCHOR_ANCHORED) != 0)
    for s, (read, start, ln, right) in enumerate(want["table"]):
        g = sp["seg"][s]
        assert (int(g["read"]), int(g["start"]), int(g["len"]), int(g["flags"])) == (read, start, ln, right | (capi.SEG_ALIGNED if reported[s] else 0)), ("segment", s)
        assert np.array_equal(sp["rows"][s, :ln], want["rows"][s, :ln]), ("segment row", s)
    assert np.array_equal(sp["lens"], want["lens"])
    for f in ("key", "val", "bucket"):
        assert np.array_equal(sp["best"][f], want["best"][f]), ("segment best", f)
    _ext_is(sp, k, want["ext"], "split")
    # secondary
    sec, want = objs["secondary"], ref["secondary"]
    k = len(want["cand"])
    t = sec["table"]
    assert len(t) == k and np.array_equal(t["read"], want["cand"]) and np.array_equal(t["hits"], ref["rival"][want["cand"], 1])
    assert np.array_equal(t["flags"], want["flags"]) and not t["_pad"].any(), "secondary table"
    for f in ("key", "val", "bucket"):
        assert np.array_equal(sec["rival"][f], want["best"][f]), ("rival", f)
    assert np.array_equal(sec["lens"], want["lens"])
    for s in range(k):
        ln = int(want["lens"][s])
        assert np.array_equal(sec["rows"][s, :ln], want["rows"][s, :ln]), ("candidate row", s)
    _ext_is(sec, k, want["ext"], "secondary")


# ---------------------------------------------------------------------------------------------------------------------
# device entries
# ---------------------------------------------------------------------------------------------------------------------
MATRIX = {                                    # name -> (seg_rows, order of the second passes)
    "own-split-secondary": (None, ("split", "secondary")),
    "own-secondary-split": (None, ("secondary", "split")),
    "shared-secondary-split": (0, ("secondary", "split")),        # the documented order: split() seeds the primary's workspace again
    "chunks-split-secondary": (16, ("split", "secondary")),
    "chunks-secondary-split": (16, ("secondary", "split")),
}


@pytest.mark.parametrize("case", list(MATRIX))
def test_full_mapper_equals_every_solo_mapper_and_the_references(world, gpu, solo, case):
    w, ref, di = world
    di.set_map_options()
    seg_rows, order = MATRIX[case]
    assert seg_rows is None or seg_rows == 0 or len(ref["split"]["table"]) > 3 * seg_rows          # several chunks
    snap, objs, _ = _fresh(world, gpu, _full(w, seg_rows=seg_rows), order)
    _same_as_solo(snap, solo)
    _is_the_reference(objs, ref, w["reads"], w["lens"], 0)


@pytest.mark.parametrize("seg_rows", [None, 0], ids=["own", "shared"])
def test_a_used_full_mapper(world, gpu, solo, seg_rows):
    """the batch, then every third read of it at another base offset, then the batch again: the third run is the first, the
    pileup is the sum of the three, the workspaces have not grown"""
    w, ref, di = world
    di.set_map_options()
    order = ("secondary", "split")
    rows2, lens2, pick = S.every_third()
    dm = mapper.DeviceMapper(di, w["n"], S.MAX_LEN, device=gpu, **_full(w, seg_rows=seg_rows))
    try:
        first, objs1, _ = _stages(dm, w["reads"], w["lens"], order)
        size = (dm.workspace_bytes(), int(lib.lrm_workspace_bytes(dm.ws_seg)) if dm.ws_seg else 0)
        second, objs2, _ = _stages(dm, rows2, lens2, order, shift=5)
        third, objs3, _ = _stages(dm, w["reads"], w["lens"], order)
        assert (dm.workspace_bytes(), int(lib.lrm_workspace_bytes(dm.ws_seg)) if dm.ws_seg else 0) == size
    finally:
        dm.close()
    _same_as_solo(first, solo, skip=("pileup",))
    for key in first:
        if key != "pileup":
            assert third[key] == first[key], (key, "third run differs from the first")
    # the second batch's primary outputs are those of its reads in the first; its second passes found those reads' work
    r1, r2 = objs1["res"], objs2["res"]
    for key in ("n_ops", "score", "meta_r", "best", "mapq", "summary", "anchor", "clip"):
        assert r2[key].tobytes() == np.ascontiguousarray(r1[key][pick]).tobytes(), ("second batch", key)
    for j, i in enumerate(pick):
        assert bytes(r2["ops"][j, :max(int(r2["n_ops"][j]), 0)]) == ref["clipped"]["ops"][i], ("second batch, ops", j)
    assert np.array_equal(pick[objs2["secondary"]["table"]["read"]], np.intersect1d(ref["secondary"]["cand"], pick))
    assert [int(pick[r]) for r in objs2["split"]["seg"]["read"]] == [t[0] for t in ref["split"]["table"] if t[0] % 3 == 0]
    # the accumulator: first + second + first, by the reference (the record of a read is a function of the read alone)
    cl = ref["clipped"]
    total = pileup_ref.Pileup(0, w["con_len"])
    for i in list(range(w["n"])) * 2 + [int(i) for i in pick]:
        total.add(cl["ops"][i], bytes(ref["oriented"][i, :w["lens"][i]]), int(cl["loc"][i]), int(cl["score"][i]), int(cl["meta_r"][i]))
    assert pileup_ref.same(objs1["pileup"], ref["pileup"].columns())
    assert pileup_ref.same(objs3["pileup"], total.columns()), pileup_ref.first_difference(objs3["pileup"], total.columns())
    _is_the_reference(objs3, ref, w["reads"], w["lens"], 0, pileup_of=total)


@pytest.mark.parametrize("seg_rows", [None, 0], ids=["own", "shared"])
def test_a_secondary_call_without_room_leaves_the_split_call_alone(world, gpu, solo, seg_rows):
    import torch
    w, ref, di = world
    di.set_map_options()
    k = len(ref["secondary"]["cand"])
    dm = mapper.DeviceMapper(di, w["n"], S.MAX_LEN, device=gpu, **_full(w, seg_rows=seg_rows, sec_cap=k - 1))
    try:
        alloc, d_reads = _upload(w["reads"])
        d_lens = torch.from_numpy(w["lens"].astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        with pytest.raises(capi.LrmError, match="room for %d" % (k - 1)) as e:
            dm.secondary(d_reads, d_lens)
        torch.cuda.synchronize()
        assert e.value.rc == -3 and e.value.n_sec == k and dm.n_sec == 0
        assert not any(bool(t.any()) for t in dm.sec.values())                 # no result array was written
        assert dm.split(d_reads, d_lens) == len(ref["split"]["table"])
        torch.cuda.synchronize()
        dm.stats()
        snap, _ = _collect(dm, w["n"], alloc)
    finally:
        dm.close()
    _same_as_solo(snap, solo, stages=[name for name in solo if name != "secondary"])


def test_a_split_call_without_room_leaves_the_secondary_call_alone(world, gpu, solo):
    import torch
    w, ref, di = world
    di.set_map_options()
    k = len(ref["split"]["table"])
    dm = mapper.DeviceMapper(di, w["n"], S.MAX_LEN, device=gpu, **_full(w, seg_cap=k - 1))
    try:
        alloc, d_reads = _upload(w["reads"])
        d_lens = torch.from_numpy(w["lens"].astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        with pytest.raises(capi.LrmError, match="segments, room for %d" % (k - 1)) as e:
            dm.split(d_reads, d_lens)
        torch.cuda.synchronize()
        assert e.value.rc == -3 and e.value.n_seg == k and dm.n_seg == 0
        assert not any(bool(t.any()) for t in dm.seg.values())                 # no result array was written
        assert dm.secondary(d_reads, d_lens) == len(ref["secondary"]["cand"])
        torch.cuda.synchronize()
        dm.stats()
        snap, _ = _collect(dm, w["n"], alloc)
    finally:
        dm.close()
    _same_as_solo(snap, solo, stages=[name for name in solo if name != "split"])


# ---------------------------------------------------------------------------------------------------------------------
# the stale walk is refused
# ---------------------------------------------------------------------------------------------------------------------
def _no_launch(dm):
    return all(launches == 0 for _, launches in dm.timing().values())


def test_secondary_behind_a_split_on_the_same_workspace_is_refused(world, gpu, solo):
    """seg_rows=0: split() seeds its segments on the primary's workspace, whose survivor lists are then the segments'"""
    import torch
    w, ref, di = world
    di.set_map_options()
    dm = mapper.DeviceMapper(di, w["n"], S.MAX_LEN, device=gpu, mapq=True, clip=True, split=True, secondary=True, seg_rows=0)
    try:
        alloc, d_reads = _upload(w["reads"])
        d_lens = torch.from_numpy(w["lens"].astype(np.int32)).cuda()
        dm.seed(d_reads, d_lens)
        dm.extend(d_reads, d_lens)
        assert dm.split(d_reads, d_lens) == len(ref["split"]["table"])
        torch.cuda.synchronize()
        dm.set_timing(True)
        with pytest.raises(capi.LrmError, match=STALE) as e:
            dm.secondary(d_reads, d_lens)
        assert e.value.rc == -1 and dm.n_sec == 0 and _no_launch(dm)
        torch.cuda.synchronize()
        assert not any(bool(t.any()) for t in dm.sec.values())
        dm.set_timing(False)
        dm.stats()
        # the next batch in the documented order
        snap, _, _ = _stages(dm, w["reads"], w["lens"], ("secondary", "split"))
    finally:
        dm.close()
    _same_as_solo(snap, solo, stages=["clip", "mapq", "split", "secondary"])


def test_rival_behind_another_seed_call_is_refused(world, gpu):
    import torch
    w, ref, di = world
    di.set_map_options()
    n = w["n"]
    rows2, lens2, pick = S.every_third()
    dm = mapper.DeviceMapper(di, n, S.MAX_LEN, device=gpu, mapq=True)
    try:
        _, d_reads = _upload(w["reads"])
        d_lens = torch.from_numpy(w["lens"].astype(np.int32)).cuda()
        _, d_reads2 = _upload(rows2)
        d_lens2 = torch.from_numpy(lens2.astype(np.int32)).cuda()
        other_best, other_mapq = torch.zeros_like(dm.best), torch.zeros_like(dm.mapq)
        stream = dm._stream()

        def seed_again(reads, lens, k, best, mapq):
            capi.check(lib.lrm_seed_batch_mapq_dev(di.handle, dm.ws, reads.data_ptr(), reads.stride(0), lens.data_ptr(), k, dm.max_len,
                                                   capi.Params(k, dm.seed_len, dm.thres), best.data_ptr(), mapq.data_ptr() if mapq is not None else None,
                                                   stream), "lrm_seed_batch_mapq_dev")

        def refused(k=n):
            dm.set_timing(True)
            with pytest.raises(capi.LrmError, match=STALE):
                dm.rival(d_lens, k)
            assert _no_launch(dm)
            dm.set_timing(False)

        def rival():
            dm.seed(d_reads, d_lens)
            out = dm.rival(d_lens, n).cpu().numpy().view(np.uint64).reshape(-1, 3)
            dm.stats()
            return out

        want = rival()
        assert np.array_equal(want, ref["rival"])
        seed_again(d_reads, d_lens, n, dm.best, None)                          # the same batch into the same best[], without the phase output
        refused()
        assert np.array_equal(rival(), want)
        seed_again(d_reads2, d_lens2, len(lens2), other_best, other_mapq)      # another batch into another best[]
        refused()
        assert np.array_equal(rival(), want)
        seed_again(d_reads, d_lens, n, other_best, other_mapq)                 # the same batch into another best[]
        refused()
        dm.seed(d_reads, d_lens)
        refused(n - 1)                                                         # the seeded best[], another n
        assert np.array_equal(dm.rival(d_lens, n).cpu().numpy().view(np.uint64).reshape(-1, 3), want)
        torch.cuda.synchronize()
        dm.stats()
    finally:
        dm.close()


# ---------------------------------------------------------------------------------------------------------------------
# host second passes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_path(world, gpu):
    w, ref, di = world
    di.set_map_options()
    snap, objs, _ = _fresh(world, gpu, _full(w), ("secondary", "split"))
    return objs


HOST_LAYOUTS = {"rows": {}, "cigar-text-keep-reads": dict(cigar_text=1, keep_reads=1), "dense": dict(dense_results=1)}


def _alignment_is(got, s, ops, aligned, text, what):
    if text:
        assert mapper.text_of(got, s).decode() == (sam_ref.rle(ops) if aligned else "*"), (what, s)
    else:
        assert mapper.ops_of(got, s) == ops, (what, s)


@pytest.mark.parametrize("order", [("split", "secondary"), ("secondary", "split")], ids=["split-secondary", "secondary-split"])
@pytest.mark.parametrize("layout", list(HOST_LAYOUTS))
def test_host_second_passes_equal_the_device_path(world, gpu, device_path, layout, order):
    w, ref, di = world
    di.set_map_options()
    opts = HOST_LAYOUTS[layout]
    text = bool(opts.get("cigar_text"))
    n, lens, dev = w["n"], w["lens"], device_path
    rm = w["reads"].copy()
    res = mapper.map_batch(di, rm, lens, options=dict(opts), clip=True, mapq=True, summary=True, md=True)
    oriented = dev["reads"].reshape(rm.shape)
    assert np.array_equal(rm, w["reads"] if opts.get("keep_reads") else oriented) and not np.array_equal(w["reads"], oriented)
    # the primary pass with mapq, summary and events on at once is the device path's
    prim = dev["res"]
    for key in ("best", "n_ops", "score", "meta_r", "mapq", "summary"):
        assert np.ascontiguousarray(res[key]).tobytes() == prim[key].tobytes(), key
    off, ev = dev["diff"]
    for i in range(n):
        _alignment_is(res, i, bytes(prim["ops"][i, :max(int(prim["n_ops"][i]), 0)]), prim["meta_r"][i] != 0 and prim["score"][i] != -1, text, "primary")
        assert np.array_equal(res["md_events"][int(res["md_off"][i]):int(res["md_off"][i]) + int(res["md_cnt"][i])], ev[int(off[i]):int(off[i + 1])]), i
    before = rm.copy()
    got = {}
    for stage in order:
        if stage == "split":
            got["split"] = mapper.split_batch(di, rm, lens, res, options=dict(opts))
        else:
            got["secondary"] = mapper.secondary_batch(di, rm, lens, res, options=dict(opts), clip=True)
        assert np.array_equal(rm, before), (stage, "moved the caller's read buffer")
    for stage, table in (("split", "seg"), ("secondary", "table")):
        out, g = dev[stage], got[stage]
        k = len(out[table])
        assert k >= 20 and len(g[table]) == k
        # (the split pass's lrm_anchor records come through the host pipeline, which leaves the four padding bytes of a record
        #  as they were in its device mirror: the fields, as tests/test_gpu_split.py compares them)
        for name in (table, "best" if stage == "split" else "rival", "clip") + (("anchor",) if stage == "secondary" else ()):
            assert np.ascontiguousarray(g[name][:k]).tobytes() == out[name].tobytes(), (stage, name)
        for f in ANCHOR_FIELDS:
            assert np.array_equal(g["anchor"][f][:k], out["anchor"][f]), (stage, "anchor", f)
        for name in ("lens", "n_ops", "score", "meta_r"):
            assert np.array_equal(g[name][:k], out[name]), (stage, name)
        on = out["meta_r"] != 0
        for f in META_FIELDS:
            assert np.array_equal(g["meta"][f][:k][on], out["meta"][f][on]), (stage, "meta", f)
        assert ("ops_off" in g) == bool(opts) and bool(g.get("is_text")) == text
        for s in range(k):
            ln = int(out["lens"][s])
            assert np.array_equal(g["rows"][s, :ln], out["rows"][s, :ln]), (stage, "row", s)
            _alignment_is(g, s, bytes(out["ops"][s, :max(int(out["n_ops"][s]), 0)]), out["meta_r"][s] != 0 and out["score"][s] != -1, text, stage)


# ---------------------------------------------------------------------------------------------------------------------
# file flow
# ---------------------------------------------------------------------------------------------------------------------
def _flag(line):
    return int(line.split("\t")[1])


def _without(text, bit):
    """A SAM text without the lines whose FLAG has `bit`; without the supplementary lines (2048) the primary lines lose the
    SA:Z tag that names them too -- it is the tail of the line (docs/GACT_SPEC.md, "Split reads")"""
    out = []
    for line in text.splitlines():
        if line.startswith("@"):
            out.append(line)
        elif not _flag(line) & bit:
            out.append(line.split("\tSA:Z:")[0] if bit == 2048 else line)
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def flow(world, gpu, tmp_path_factory):
    w, ref, di = world
    tmp = tmp_path_factory.mktemp("stage_mix")
    fa, fq = tmp / "ref.fa", tmp / "reads.fq"
    with open(fa, "wb") as f:
        for name, seq in zip((b"chrP", b"chrQ"), w["seqs"]):
            f.write(b">" + name + b"\n")
            for at in range(0, len(seq), 60):
                f.write(bytes(seq[at:at + 60]) + b"\n")
    assert lib.lrm_accidx(str(fa).encode(), 32, S.HLEN, 1) == 0
    with open(fq, "wb") as f:
        for i in range(w["n"]):
            s = bytes(w["reads"][i, :w["lens"][i]])
            f.write(b"@r%d\n" % i + s + b"\n+\n" + bytes(33 + (i + j) % 40 for j in range(len(s))) + b"\n")
    so = capi.SecondaryOptions(C.sizeof(capi.SecondaryOptions), 0, 0, 1, 0, 1, 0, 0)
    with_split, without = capi.map_options(anchored=1, clip=1, split=1), capi.map_options(anchored=1, clip=1)
    runs = {"S+X": dict(options=with_split, secondary=so), "X": dict(options=without, secondary=so), "S": dict(options=with_split, mapq=1),
            "md+S": dict(options=with_split, mapq=1, md=True), "md": dict(options=without, mapq=1, md=True)}
    out = {}
    for name, kw in runs.items():                  # batches of 64: the second passes run on three batches, two of them in flight
        counts = textio.accaln(fa, fq, tmp / (name + ".sam"), 64, device=gpu, rg_id=7, **kw)
        out[name] = (open(tmp / (name + ".sam")).read(), counts)
    return out


def test_file_flow_with_split_and_secondary_is_both_flows(world, flow, device_path):
    w, ref, di = world
    both, sec_only, split_only = flow["S+X"][0], flow["X"][0], flow["S"][0]
    assert flow["S+X"][1] == flow["X"][1] == flow["S"][1] and flow["S"][1][0] == w["n"]
    assert _without(both, 256) == split_only
    assert _without(both, 2048) == sec_only
    # SA:Z stands on the lines of the reads with supplementary lines, and on no other
    lines = [x for x in both.splitlines() if not x.startswith("@")]
    with_sup = {x.split("\t")[0] for x in lines if _flag(x) & 2048}
    assert {x.split("\t")[0] for x in lines if "\tSA:Z:" in x} == with_sup and "\tSA:Z:" not in sec_only
    # whose lines: the reads the device path reports segments and secondaries for
    sp, sec, prim = device_path["split"], device_path["secondary"], device_path["res"]
    mapped = (prim["meta_r"] != 0) & (prim["score"] != -1)
    want_sup = {"r%d" % r for r, fl in zip(sp["seg"]["read"], sp["seg"]["flags"]) if fl & capi.SEG_ALIGNED and mapped[r]}
    want_sec = {"r%d" % r for r, fl in zip(sec["table"]["read"], sec["table"]["flags"]) if fl & capi.SEC_ALIGNED}
    assert with_sup == want_sup and {x.split("\t")[0] for x in lines if _flag(x) & 256} == want_sec
    # a class (c) read: primary, supplementary, secondary, directly behind one another
    by_name = {}
    for at, x in enumerate(lines):
        by_name.setdefault(x.split("\t")[0], []).append((at, _flag(x)))
    assert len(by_name) == w["n"]
    chimeras = 0
    for i in np.flatnonzero(w["cls"] == "c"):
        name = "r%d" % i
        group = by_name[name]
        assert [at for at, _ in group] == list(range(group[0][0], group[0][0] + len(group))), name
        kinds = [fl & (2048 | 256) for _, fl in group]
        assert kinds == [0] + [2048] * kinds.count(2048) + [256] * kinds.count(256) and kinds.count(256) <= 1, (name, kinds)
        chimeras += kinds.count(2048) >= 1 and kinds.count(256) == 1
    print("class (c) reads with a supplementary and a secondary line: %d of %d" % (chimeras, (w["cls"] == "c").sum()))
    assert chimeras >= 8


def test_file_flow_md_tags_do_not_depend_on_split(world, flow):
    with_split, plain = flow["md+S"][0], flow["md"][0]
    assert flow["md+S"][1] == flow["md"][1]
    assert _without(with_split, 2048) == plain
    tags = lambda text: [(x.split("\t")[0], [f for f in x.split("\t")[11:] if f[:5] in ("NM:i:", "MD:Z:")])
                         for x in text.splitlines() if not x.startswith("@") and not _flag(x) & 2048]
    a, b = tags(with_split), tags(plain)
    assert a == b and sum(len(t) == 2 for _, t in a) >= 150
    assert any(_flag(x) & 2048 for x in with_split.splitlines() if not x.startswith("@"))
