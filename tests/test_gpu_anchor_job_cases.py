"""The job rows of the anchored extension at their edges (tests/anchor_job_cases.py: the anchor's place j over every residue
mod 16, the bytewise tails, the AN_CHUNK edges, both strands, three row strides) against tests/anchored_ref.py and
tests/clip_ref.py.  A wrong byte in a job row is a changed CIGAR."""
import numpy as np
import pytest

import anchor_job_cases as ajc
import anchored_ref
import clip_ref
from longreadmapper_amd import index, mapper
from test_gpu_anchored import _check_against_ref
from test_gpu_clip import _check, _device_run

pytestmark = pytest.mark.gpu
GACT = (320, 120, 128)


@pytest.fixture(scope="module")
def planted(gpu):
    """The sequence uploaded, the cases, and the reference of the batch, computed once."""
    s = ajc.seq()
    hi = index.HostIndex.build([s], hlen=8)
    di = index.DeviceIndex.upload(hi, gpu)
    mta = [(o, l) for _, o, l in hi.mta()]
    S, ls = mta[0]
    cs = ajc.cases()
    max_len = max(c["n"] for c in cs)
    reads, lens, keys = ajc.batch(cs, S, ls, max_len + 1)
    best = np.zeros(len(cs), dtype=mapper.ENTRY_DT)
    best["key"] = keys
    di.set_map_options()
    oriented = reads.copy()
    classic = mapper.extend_batch(di, oriented, lens, best, GACT)
    for i, c in enumerate(cs):                                         # the classic path resolves what the cases planned
        assert classic["meta_r"][i] == 1 and int(classic["meta"]["loc"][i]) == S + c["start"], c["name"]
        assert classic["meta"]["strand"][i] == c["strand"] and bytes(oriented[i, :c["n"]]) == bytes(c["fwd"]), c["name"]
    want = anchored_ref.extend_batch(hi.content(), mta, oriented, lens, classic["meta"], classic["meta_r"], GACT)
    for w, c in zip(want, cs):                                         # ... and the reference anchors where they planted
        assert (w["len"], w["delta"], w["read_pos"]) == (ajc.RUN, 0, c["j"]) and w["flags"] & anchored_ref.ANCHORED, c["name"]
    want_clip = [clip_ref.apply_clip(w, int(lens[i]), 0, 0) for i, w in enumerate(want)]
    yield di, S, ls, cs, max_len, best, want, want_clip
    di.close()


@pytest.mark.parametrize("impl", [0, 4])
@pytest.mark.parametrize("stride_at", [0, 1, 2])
def test_job_rows_at_their_edges(planted, map_options, gpu, impl, stride_at):
    di, S, ls, cs, max_len, best, want, want_clip = planted
    stride = ajc.strides(max_len)[stride_at]
    reads, lens, keys = ajc.batch(cs, S, ls, stride)
    assert np.array_equal(keys, best["key"])
    fwd = np.zeros_like(reads)
    for i, c in enumerate(cs):
        fwd[i, :c["n"]] = c["fwd"]
    map_options(di, gact_impl=impl)
    # the device path: ops, score, meta and the anchor records
    dev, rd = _device_run(di, gpu, reads, lens, best, GACT, anchored=True)
    assert np.array_equal(rd, fwd)
    _check_against_ref(dev, want, dev["anchor"])
    dev, rd = _device_run(di, gpu, reads, lens, best, GACT, clip=True)
    assert np.array_equal(rd, fwd)
    _check(dev, want_clip, dev["anchor"], dev["clip"])
    # the host path
    rd = reads.copy()
    got = mapper.extend_batch(di, rd, lens, best, GACT, anchored=True)
    assert np.array_equal(rd, fwd)
    _check_against_ref(got, want)
    rd = reads.copy()
    got = mapper.extend_batch(di, rd, lens, best, GACT, clip=True)
    assert np.array_equal(rd, fwd)
    _check(got, want_clip)
