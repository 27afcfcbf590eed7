"""The device entries on hostile buffers and on used workspaces (tests/hostile_buffers.py).

Every stage -- seed, mapping quality, the three extension entries on the byte kernels and on the bit-sliced one, split with
and without a workspace of its own, secondary -- runs the same batch in every layout of hostile_buffers.LAYOUTS, at an
aligned and at a moved base, with n below the rows of every array and every output tensor in 0xA5 fill.  Asserted per run:
every output of the rows < n equals the CPU references (tests/test_hostile_buffers_cpu.py: those are functions of the reads
alone), the read buffer changes in the bases of the reverse-strand reads only, no output is written outside its rows < n, no
op row behind its last op byte (hostile_buffers.op_extent: tighter than the extent include/lrm_accel.h grants).  Then the host boundary on the same layouts,
and the same batch on a workspace that has just run a larger, different one."""
import numpy as np
import pytest

import hostile_buffers as H
from longreadmapper_amd import capi, index, mapper
from longreadmapper_amd.records import ANCHOR_DT, CLIP_DT, ENTRY_DT, MAPQ_DT, META_DT, SECONDARY_DT, SEGMENT_DT, units16

pytestmark = pytest.mark.gpu
MAPQ_FIELDS = ("n1", "n2", "radius", "mapq", "phase", "flags")
ANCHOR_FIELDS = ("text_pos", "read_pos", "len", "delta", "left_ops", "flags")
CONFIGS = {                                   # name -> (DeviceMapper options, extension mode, second pass)
    "seed": (dict(), None, None),
    "classic": (dict(mapq=True), "classic", None),
    "anchored": (dict(mapq=True, anchored=True), "anchored", None),
    "clipped": (dict(mapq=True, clip=True), "clipped", None),
    "split-own": (dict(clip=True, split=True), "clipped", "split"),
    "split-shared": (dict(clip=True, split=True, seg_rows=0), "clipped", "split"),
    "secondary": (dict(mapq=True, clip=True, secondary=True), "clipped", "secondary"),
}
IMPLS = {"byte": 0, "bitsliced": 4}           # lrm_map_options.gact_impl: the automatic choice (byte kernels at this size), bit-sliced
CASES = [("seed", "byte")] + [(c, i) for c in CONFIGS if c != "seed" for i in IMPLS]


@pytest.fixture(scope="module")
def world(gpu):
    b = H.batch()
    rows = H.build(b, "plain").rows[:b["n"]].copy()
    ref = H.references(b, rows, b["lens"])
    di = index.DeviceIndex.upload(b["hi"], gpu)
    Guarded = H.guarded(mapper.DeviceMapper)
    yield b, ref, di, Guarded
    di.close()


def _fields(got, want, names, what):
    for f in names:
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:6].tolist())


def _check_extension(dm, tensors, k, ext, mode, lens, what):
    """The k rows of an extension's outputs (tensors: name -> tensor) against extension_ref `ext`, guards and op extents
    -> {name: bytes}, what must be the same whatever the layout and whatever the workspace ran before"""
    snap = {}
    n_ops = dm.check_guards(tensors["n_ops"], k, (what, "n_ops")).copy().view(np.int32).reshape(-1)
    score = dm.check_guards(tensors["score"], k, (what, "score")).copy().view(np.int32).reshape(-1)
    meta_r = dm.check_guards(tensors["meta_r"], k, (what, "meta_r")).copy().view(np.int32).reshape(-1)
    meta = dm.check_guards(tensors["meta"], k, (what, "meta")).copy().reshape(-1).view(META_DT)
    _fields(dict(n_ops=n_ops, score=score, meta_r=meta_r), ext, ("meta_r", "n_ops", "score"), what)
    on = meta_r != 0
    for f in ("loc", "off", "seq_id", "strand"):
        assert np.array_equal(meta[f][on].astype(np.int64), np.asarray(ext[f])[on].astype(np.int64)), (what, "meta", f)
    snap.update(n_ops=n_ops.tobytes(), score=score.tobytes(), meta_r=meta_r.tobytes(),
                meta=b"".join(meta[f][on].tobytes() for f in ("loc", "off", "seq_id", "strand")))
    store = dm.check_guards(tensors["store"], k, (what, "store"))
    assert store.shape[1] >= units16(2 * H.M) + 48
    ops = []
    for i in range(k):
        m = max(int(n_ops[i]), 0)
        assert bytes(store[i, :m]) == ext["ops"][i], (what, "ops of row", i)
        end = H.op_extent(mode, m, bool(on[i]) and score[i] == -1, int(lens[i]))
        assert (store[i, end:] == H.FILL).all(), (what, "op row %d: %d ops, written behind byte %d" % (i, m, end),
                                                  (np.flatnonzero(store[i] != H.FILL)[-1]))
        ops.append(bytes(store[i, :m]))
    snap["ops"] = b"".join(ops)
    if "anchor" in tensors and tensors["anchor"] is not None:
        anchor = dm.check_guards(tensors["anchor"], k, (what, "anchor")).copy().reshape(-1).view(ANCHOR_DT)
        for c, f in enumerate(ANCHOR_FIELDS):
            assert np.array_equal(anchor[f].astype(np.int64), ext["anchor"][:, c]), (what, "anchor", f)
        snap["anchor"] = anchor.tobytes()
    if "clip" in tensors and tensors["clip"] is not None:
        clip = dm.check_guards(tensors["clip"], k, (what, "clip")).copy().reshape(-1).view(CLIP_DT)
        assert np.array_equal(clip["left"], ext["clip_left"]) and np.array_equal(clip["right"], ext["clip_right"]), (what, "clip")
        snap["clip"] = clip.tobytes()
    return snap


def _primary_tensors(dm):
    return dict(store=dm.store, n_ops=dm.n_ops, score=dm.score, meta=dm.meta, meta_r=dm.meta_r, anchor=dm.anchor, clip=dm.clip)


def _untouched(dm, tensors, what):
    for name, t in tensors.items():
        if t is not None:
            dm.check_guards(t, 0, (what, name, "not an output of this stage"))


def run_stages(dm, b, ref, buf, config, what, on_seed=None):
    """seed [, extend [, split | secondary]] of a config on mapper dm over Buffer buf, everything asserted -> the snapshot;
    on_seed(): called behind the seed stage"""
    import torch
    _, mode, second = CONFIGS[config]
    n, lens = b["n"], b["lens"]
    alloc = torch.from_numpy(buf.alloc).cuda()
    d_reads = alloc[buf.shift:].view(n + H.D, buf.stride)
    d_lens = torch.from_numpy(buf.lens.astype(np.int32)).cuda()
    assert d_reads.data_ptr() % 16 == buf.shift and d_reads.stride(0) == buf.stride >= dm.max_len >= int(buf.lens.max())
    snap = {}

    # ---- seed (and mapping quality)
    dm.seed(d_reads, d_lens, n)
    torch.cuda.synchronize()
    dm.stats()                                            # raises if the sticky kernel-error word of the workspace is set
    if on_seed:
        on_seed()
    assert np.array_equal(alloc.cpu().numpy(), buf.alloc), (what, "the seed stage wrote into the read buffer")
    best = dm.check_guards(dm.best, n, (what, "best")).copy().reshape(-1).view(ENTRY_DT)
    _fields(best, ref["best"], ("key", "val", "bucket"), (what, "best"))
    snap["best"] = best.tobytes()
    if dm.mapq is not None:
        mq = dm.check_guards(dm.mapq, n, (what, "mapq")).copy().reshape(-1).view(MAPQ_DT)
        _fields(mq, ref["mapq"], MAPQ_FIELDS, (what, "mapq"))
        snap["mapq"] = b"".join(mq[f].tobytes() for f in MAPQ_FIELDS)
    _untouched(dm, _primary_tensors(dm), (what, "seed"))
    if mode is None:
        return snap

    # ---- extension: the decoy rows of best[] are valid entries too
    dm.best[n:n + H.D] = dm.best[n - H.D:n].clone()
    best_before = dm.raw_of(dm.best)
    dm.extend(d_reads, d_lens, n)
    torch.cuda.synchronize()
    dm.stats()
    assert np.array_equal(dm.raw_of(dm.best), best_before), (what, "the extension wrote best[]")
    snap.update(_check_extension(dm, _primary_tensors(dm), n, ref[mode], mode, lens, (what, mode)))
    # the read buffer: the bases of the reverse-strand reads turned round, every other byte of the allocation as it was
    want_alloc = buf.alloc.copy()
    want_rows = want_alloc[buf.shift:].reshape(n + H.D, buf.stride)
    for i in range(n):
        want_rows[i, :lens[i]] = ref["oriented"][i, :lens[i]]
    after = alloc.cpu().numpy()
    assert np.array_equal(after, want_alloc), (what, "read buffer", np.flatnonzero(after != want_alloc)[:6].tolist())
    if second is None:
        return snap
    primary_before = [dm.raw_of(t) for t in _primary_tensors(dm).values() if t is not None]

    # ---- the second passes
    if second == "split":
        want = ref["split"]
        k = dm.split(d_reads, d_lens, n)
        torch.cuda.synchronize()
        g = dm.seg
        assert k == len(want["table"]) >= 3
        seg = dm.check_guards(g["seg"], k, (what, "seg")).copy().reshape(-1).view(SEGMENT_DT)
        reported = (want["ext"]["meta_r"] != 0) & ((want["ext"]["anchor"][:, 5] & capi.ANCHOR_ANCHORED) != 0)
        for s, (read, start, ln, right) in enumerate(want["table"]):
            assert (int(seg["read"][s]), int(seg["start"][s]), int(seg["len"][s]), int(seg["flags"][s])) == \
                (read, start, ln, right | (capi.SEG_ALIGNED if reported[s] else 0)), (what, "segment", s)
        written = lambda ln: units16(ln)                  # the gather's last store ends on the next multiple of 16
        table = seg
    else:
        want = ref["secondary"]
        k = dm.secondary(d_reads, d_lens, n)
        torch.cuda.synchronize()
        g = dm.sec
        assert k == len(want["cand"]) >= 3
        table = dm.check_guards(g["table"], k, (what, "table")).copy().reshape(-1).view(SECONDARY_DT)
        assert np.array_equal(table["read"], want["cand"]) and np.array_equal(table["hits"], ref["rival"][want["cand"], 1])
        assert np.array_equal(table["flags"], want["flags"]) and not table["_pad"].any(), (what, "table")
        rival = dm.check_guards(g["rival"], k, (what, "rival")).copy().reshape(-1).view(ENTRY_DT)
        _fields(rival, want["best"], ("key", "val", "bucket"), (what, "rival"))
        snap["rival"] = rival.tobytes()
        written = lambda ln: g["rows"].shape[1]           # zeros to the row's end
    dm.stats()
    snap["table"] = table.tobytes()
    got_lens = dm.check_guards(g["lens"], k, (what, "lens")).copy().view(np.uint32).reshape(-1)
    assert np.array_equal(got_lens, want["lens"]), (what, "lens")
    if second == "split":
        seg_best = dm.check_guards(g["best"], k, (what, "seg best")).copy().reshape(-1).view(ENTRY_DT)
        _fields(seg_best, want["best"], ("key", "val", "bucket"), (what, "seg best"))
        snap["seg_best"] = seg_best.tobytes()
    rows = dm.check_guards(g["rows"], k, (what, "rows"))
    for s in range(k):
        ln = int(want["lens"][s])
        assert np.array_equal(rows[s, :ln], want["rows"][s, :ln]), (what, "row", s)
        assert not rows[s, ln:written(ln)].any() and (rows[s, written(ln):] == H.FILL).all(), (what, "behind row", s)
    snap["rows"] = b"".join(bytes(rows[s, :want["lens"][s]]) for s in range(k))
    sub = _check_extension(dm, g, k, want["ext"], "clipped", want["lens"], (what, second))
    snap.update({second + "_" + name: v for name, v in sub.items()})
    # the stage leaves the primary's outputs and the reads alone
    for t, was in zip([t for t in _primary_tensors(dm).values() if t is not None], primary_before):
        assert np.array_equal(dm.raw_of(t), was), (what, second, "a primary output moved")
    assert np.array_equal(alloc.cpu().numpy(), want_alloc), (what, second, "read buffer")
    return snap


def fresh_run(world, gpu, config, layout, shift, n_max=None, max_len=H.M):
    b, ref, di, Guarded = world
    dm = Guarded(di, n_max or b["n"] + H.D, max_len, device=gpu, **CONFIGS[config][0])
    try:
        return run_stages(dm, b, ref, H.build(b, layout, shift), config, (config, layout, shift))
    finally:
        dm.close()


@pytest.fixture(scope="module")
def plain_snaps(world, gpu):
    """the snapshot of every case in the plain layout (today's: stride M + 1, zeros) from a new mapper, computed once; the
    caller has set the kernel choice `impl` names"""
    cache = {}

    def get(config, impl):
        if (config, impl) not in cache:
            cache[(config, impl)] = fresh_run(world, gpu, config, "plain", 0)
        return cache[(config, impl)]
    return get


@pytest.mark.parametrize("layout", H.LAYOUTS)
@pytest.mark.parametrize("config,impl", CASES)
def test_results_are_a_function_of_the_reads_and_writes_stay_inside(world, gpu, map_options, plain_snaps, config, impl, layout):
    map_options(world[2], gact_impl=IMPLS[impl])
    want = plain_snaps(config, impl)
    for shift in (0, H.shift_of(layout)):
        got = fresh_run(world, gpu, config, layout, shift)
        assert sorted(got) == sorted(want)
        for name in want:
            assert got[name] == want[name], (config, impl, layout, shift, name, "differs from the plain layout's")


# ---------------------------------------------------------------------------------------------------------------------
# the host boundary
# ---------------------------------------------------------------------------------------------------------------------
HOST_OPTS = {"rows": {}, "dense": dict(dense_results=1), "cigar-text": dict(cigar_text=1), "keep-reads": dict(keep_reads=1),
             "sub-batches": dict(sub_batches=3)}


@pytest.mark.parametrize("layout", ["abutting", "text-pad-1", "ff-pad"])
@pytest.mark.parametrize("opts", list(HOST_OPTS))
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_boundary_on_hostile_buffers(world, gpu, layout, opts, pinned):
    import sam_ref
    b, ref, di, _ = world
    di.set_map_options()
    n, lens = b["n"], b["lens"]
    buf = H.build(b, layout, 0 if pinned else H.shift_of(layout))
    if pinned:
        mem = mapper.pinned_empty(len(buf.alloc))
        mem[:] = buf.alloc
        buf = H.Buffer(mem, buf.shift, buf.stride, buf.lens)
    try:
        before = buf.alloc.copy()
        rows = buf.rows[:n]
        res = mapper.map_batch(di, rows, lens, options=dict(HOST_OPTS[opts]), clip=True, mapq=True)
        want = ref["clipped"]
        _fields(res["best"], ref["best"], ("key", "val", "bucket"), (layout, opts, "best"))
        _fields(res["mapq"], ref["mapq"], MAPQ_FIELDS, (layout, opts, "mapq"))
        _fields(res, want, ("meta_r", "n_ops", "score"), (layout, opts))
        for f in ("loc", "off", "seq_id", "strand"):
            assert np.array_equal(res["meta"][f].astype(np.int64), np.asarray(want[f]).astype(np.int64)), (layout, opts, f)
        for i in range(n):
            if HOST_OPTS[opts].get("cigar_text"):
                assert mapper.text_of(res, i).decode() == (sam_ref.rle(want["ops"][i]) if want["score"][i] != -1 else "*"), i
            else:
                assert mapper.ops_of(res, i) == want["ops"][i], (layout, opts, i)
        expect = before.copy()
        if not HOST_OPTS[opts].get("keep_reads"):
            view = expect[buf.shift:].reshape(n + H.D, buf.stride)
            for i in range(n):
                view[i, :lens[i]] = ref["oriented"][i, :lens[i]]
        assert np.array_equal(buf.alloc, expect), (layout, opts, np.flatnonzero(buf.alloc != expect)[:6].tolist())
    finally:
        if pinned:
            mapper.pinned_free(buf.alloc)


# ---------------------------------------------------------------------------------------------------------------------
# a used workspace
# ---------------------------------------------------------------------------------------------------------------------
DIRTY_N, DIRTY_LEN = 96, 6000


def _dirty_batch(b):
    """96 reads of 6000 bases, both strands, ONT noise: a third across the 250-copy family (thousands of hits per phase: the
    workgroup table in several passes, the redo list), a third with a non-ACGT byte (flagged: the bit-sliced path hands them
    over), a third with 40 exact bases of the family's element (one or two 250-hit seeds per phase: one workgroup pass)."""
    rng = np.random.default_rng(77)
    seqs = b["seqs"]
    rows = np.zeros((DIRTY_N, DIRTY_LEN + 1), dtype=np.uint8)
    for i in range(DIRTY_N):
        seq = 0 if i % 3 == 0 else 1
        src = bytes(seqs[seq]) if i % 2 == 0 else bytes(H.anchored_ref.revcomp(seqs[seq]))
        at = int(rng.integers(0, len(src) - DIRTY_LEN - DIRTY_LEN // 6 - 64))
        rd = bytearray(H._noisy(rng, src, at, DIRTY_LEN, *H.ONT)[0])
        if i % 3 == 1:
            for p in rng.integers(0, DIRTY_LEN, 1 + i % 4):
                rd[int(p)] = ord("N")
        if i % 3 == 2:
            rd[1000:1040] = bytes(b["elem"][100:140])
        rows[i, :DIRTY_LEN] = np.frombuffer(bytes(rd), dtype=np.uint8)
    return rows, np.full(DIRTY_N, DIRTY_LEN, dtype=np.uint32)


def _clean_batch(b):
    """96 exact reads of 900 bases: every one decides in phase 0"""
    rng = np.random.default_rng(78)
    src = bytes(b["seqs"][1])
    rows = np.zeros((DIRTY_N, DIRTY_LEN + 1), dtype=np.uint8)
    for i in range(DIRTY_N):
        at = int(rng.integers(19_000, 43_000))
        rows[i, :900] = np.frombuffer(src[at:at + 900], dtype=np.uint8)
    return rows, np.full(DIRTY_N, 900, dtype=np.uint32)


def _run_plainly(dm, rows, lens, second):
    """every stage of the mapper over a batch, nothing asserted: what the workspace keeps is what matters -> the seed stage's stats"""
    import torch
    d_reads, d_lens = torch.from_numpy(rows).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    dm.seed(d_reads, d_lens)
    st = dm.stats()                                       # (of the batch's own seed stage: a split on this workspace seeds again)
    dm.extend(d_reads, d_lens)
    if second == "split":
        dm.split(d_reads, d_lens)
    elif second == "secondary":
        dm.secondary(d_reads, d_lens)
    torch.cuda.synchronize()
    dm.stats()
    return st


@pytest.mark.parametrize("config,impl", [c for c in CASES if c[0] != "seed"])
def test_a_used_workspace_gives_the_answers_of_a_new_one(world, gpu, map_options, plain_snaps, config, impl):
    b, ref, di, Guarded = world
    map_options(di, gact_impl=IMPLS[impl], seed_rounds=0)
    want = plain_snaps(config, impl)
    opts, mode, second = CONFIGS[config]
    dirty, clean = _dirty_batch(b), _clean_batch(b)
    dm = Guarded(di, DIRTY_N, DIRTY_LEN, device=gpu, **opts)
    try:
        dm.set_timing(True)
        st = _run_plainly(dm, *dirty, second)
        assert st["vote_tier2_items"] > 0 and st["vote_tier3_items"] > 0 and st["vote_redo_items"] > 0, st
        launches = []
        # behind every stage of the dirtying batch; behind itself; behind the dirtying batch's seed and extension alone; behind
        # reads that all decide in phase 0
        for step, (before, layout) in enumerate(((None, "plain"), (None, "text-pad-1"), ((dirty, None), "plain"), ((clean, second), "plain"))):
            if before:
                _run_plainly(dm, *before[0], before[1])
            dm.refill()
            dm.timing()
            with dm.batch_max_len(H.M):                   # the smaller batch on the larger workspace: d_lens[i] <= max_len <= stride
                got = run_stages(dm, b, ref, H.build(b, layout, H.shift_of(layout) if step else 0), config, (config, impl, "used", step),
                                 on_seed=lambda: launches.append(dm.timing()["seed_search_kernel"][1]))
            for name in want:
                assert got[name] == want[name], (config, impl, step, layout, name, "differs from a fresh mapper's")
        # The round policy looks at the workspace's last seed call: one round behind at least 64 reads of which fewer than 2 %
        # decided in phase 0, else two.  Step 0 follows the dirtying batch (96 reads, none decided: one round) -- unless the
        # split stage seeded its few segments on this same workspace in between (two); step 1 follows the hostile batch or
        # its segments (fewer than 64 reads: two); step 2 the dirtying batch's seed stage (one); step 3 the clean batch or,
        # with the workspace shared, the hostile batch's segments (two)
        print("seed_search_kernel launches per step: %s" % launches)
        assert launches == [2 if config == "split-shared" else 1, 2, 1, 2], launches
    finally:
        dm.close()


def test_a_used_host_handle_gives_the_answers_of_a_new_one(world, gpu):
    b, ref, di, _ = world
    di.set_map_options()
    n, lens = b["n"], b["lens"]
    d2 = index.DeviceIndex.upload(b["hi"], gpu)
    try:
        dirty_rows, dirty_lens = _dirty_batch(b)
        big = mapper.map_batch(d2, dirty_rows, dirty_lens, clip=True, mapq=True)
        assert (big["meta_r"] != 0).sum() >= DIRTY_N // 2
        for layout in ("plain", "text-pad-1", "abutting"):
            used, new = H.build(b, layout), H.build(b, layout)
            a = mapper.map_batch(d2, used.rows[:n], lens, clip=True, mapq=True)
            c = mapper.map_batch(di, new.rows[:n], lens, clip=True, mapq=True)
            for key in ("best", "n_ops", "score", "meta_r", "mapq"):
                assert a[key].tobytes() == c[key].tobytes(), (layout, key)
            _fields(a, ref["clipped"], ("meta_r", "n_ops", "score"), (layout, "used handle"))
            for i in range(n):
                assert mapper.ops_of(a, i) == mapper.ops_of(c, i) == ref["clipped"]["ops"][i], (layout, i)
            assert np.array_equal(used.alloc, new.alloc)
    finally:
        d2.close()
