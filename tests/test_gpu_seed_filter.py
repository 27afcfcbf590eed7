"""seed_search_kernel behind the presence bitmap of the seed table's lines (seed_kernels.hip: sd_issue_filtered;
index_tables.hip: sd_filter_build) on the batches of tests/seed_filter_cases.py.

Every batch runs on two handles made in one process, the first with LRM_SD_FILTER_KB unset (the bitmap is built: the
handle's verbose line says so, with its size and set fraction) and the second with LRM_SD_FILTER_KB=0 (no bitmap: the
kernel fetches every line).  What the seed stage leaves -- key, count and bucket of both vote entries of every (read,
phase) (lrm_debug_vote_results), best[], and how many items the vote routed to each tier (by cnt[] and hits[] of the
lists) -- must be equal between the two, and equal to brute force (tests/test_gpu_seed_writeout.py: census + vote_top2
per phase, best[] from the CPU oracle).  The vote of a phase counts every hit of every survivor of that phase, so a lost,
doubled or misplaced survivor changes it; the survivor lists themselves have no tap of their own.

Two legs.  "natural": the table as the plan makes it (40 kbp: 2^17 lines), one bit per line, 16 KiB.  "g3": one bit per
EIGHT lines.  With the natural plan eight lines hold 2.4 cores and 91 % of such bits would be set, which the builder's rule
(keep the bitmap only if at most half of its bits are set) refuses; so this leg makes the table sparse with LRM_SD_BITS=21
(0.02 cores per line) and caps the bitmap at 32 KiB = 2^18 bits.

LRM_SS_ITEMS 1024 and 4096 select the kernel's other two instantiations behind the bitmap (another count of iterations per
wavefront, another workgroup boundary); the default 2048 is what every other case runs."""
import contextlib
import os
import re
import tempfile

import numpy as np
import pytest

import constructed as K
import orc
import seed_filter_cases as F
import test_gpu_seed_writeout as W
from longreadmapper_amd import capi, index

pytestmark = pytest.mark.gpu

S, THRES = F.S, F.THRES
LEGS = {"natural": (dict(), 1, 16 * 1024), "g3": (dict(LRM_SD_BITS="21", LRM_SD_FILTER_KB="32"), 8, 32 * 1024)}
LINE = re.compile(r"\[lrm\] seed filter: (\d+) bytes, one bit per (\d+) lines, ([0-9.]+) % of the bits set\n")


@contextlib.contextmanager
def _environ(**env):
    """LRM_* as given (None: unset) while a handle is made -- a handle reads them once, when it is created -- and what the
    process writes to stderr meanwhile."""
    old = {k: os.environ.get(k) for k in env}
    said = []
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        try:
            for k, v in env.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            os.dup2(tmp.fileno(), 2)
            yield said
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            tmp.seek(0)
            said.append(tmp.read().decode(errors="replace"))


class _World:
    def __init__(self):
        self.seq = F.forward()
        self.hi = index.HostIndex.build([np.frombuffer(self.seq, dtype=np.uint8)], hlen=8)
        assert bytes(self.hi.content()) == K.index_text([self.seq])
        K.check_sa(self.hi.content(), self.hi.sa())
        sa = self.hi.sa().astype(np.int64)
        self.rank = np.empty(len(sa), dtype=np.int64)
        self.rank[sa] = np.arange(len(sa))
        self.oi = orc.OracleIndex.from_host_index(self.hi)
        self.cen = K.census(self.hi.content(), S)
        self.cases, self.handles = {}, {}

    def case(self, name):
        """Batch, brute-force votes of every phase, the oracle's best[]: computed once per batch, never changed."""
        if name not in self.cases:
            reads = F.batch(name, self.seq)
            arr, lens = F.rows(reads)
            top, n_surv = W._top2_all_phases(reads, S, THRES, self.cen, self.rank)
            best, _ = self.oi.seed_batch(arr, lens, S, THRES)
            nseeds = lens.astype(np.int64) // (S + 1)
            decided0 = (nseeds > 0) & (5 * (top[:, 0, 1] + top[:, 0, 4]).astype(np.int64) > 3 * nseeds)
            self.cases[name] = ((arr, lens), (top, best, decided0), n_surv)
        return self.cases[name]

    def pair(self, gpu, leg):
        """(handle with the bitmap, handle without) of a leg; the first one's verbose line is checked here."""
        if leg not in self.handles:
            env, per_bit, size = LEGS[leg]
            base = dict(LRM_SD_BITS=None, LRM_SD_FILTER_KB=None, LRM_HOST_VERBOSE="1")
            opts = dict(seed_table=1, seed_table_len=S, seed_table_share=4, lc_long_max=13)
            with _environ(**{**base, **env}) as said:
                with_f = index.DeviceIndex.upload(self.hi, gpu, **opts)
            with _environ(**{**base, **env, "LRM_SD_FILTER_KB": "0"}) as said0:
                without = index.DeviceIndex.upload(self.hi, gpu, **opts)
            self.handles[leg] = (with_f, without)
            m = LINE.search(said[0])
            assert m, said[0]                                        # the bitmap was built and kept
            assert (int(m.group(1)), int(m.group(2))) == (size, per_bit), m.group(0)
            assert 5.0 < float(m.group(3)) <= 50.0, m.group(0)
            assert "seed table:" in said0[0] and "seed filter" not in said0[0], said0[0]
            for di in self.handles[leg]:
                t = di.tables()
                assert (t["seed_table_len"], t["seed_table_share"], t["seed_table_slot_bytes"]) == (S, 4, 8)
                assert t["seed_table_bits"] == (21 if leg == "g3" else 17)
                di.set_map_options(seed_rounds=1)                    # all phases in one launch: the shared-lines loop
        return self.handles[leg]

    def close(self):
        for pair in self.handles.values():
            for di in pair:
                di.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


@pytest.mark.parametrize("batch", F.BATCHES)
@pytest.mark.parametrize("leg", list(LEGS))
def test_bitmap_changes_nothing(gpu, world, leg, batch):
    (arr, lens), want, n_surv = world.case(batch)
    if batch == "random":
        assert not n_surv.any()
    with_f, without = world.pair(gpu, leg)
    got_f, best_f, st_f = W._device(with_f, gpu, arr, lens, S, THRES)
    got_0, best_0, st_0 = W._device(without, gpu, arr, lens, S, THRES)
    assert np.array_equal(got_f, got_0), (leg, batch, np.argwhere((got_f != got_0).any(axis=2))[:8].tolist())
    assert np.array_equal(best_f, best_0), (leg, batch)
    for f in ("vote_tier2_items", "vote_tier3_items", "reads_decided_phase0"):       # the vote's routing goes by cnt[] and hits[]
        assert st_f[f] == st_0[f], (leg, batch, f, st_f[f], st_0[f])
    W._compare(got_f, best_f, want, 1, (leg, batch, "bitmap"))
    W._compare(got_0, best_0, want, 1, (leg, batch, "no bitmap"))


@pytest.mark.parametrize("batch", ["stretch", "lengths", "ont"])
@pytest.mark.parametrize("ss_items", [1024, 4096])
def test_other_workgroup_sizes(gpu, world, monkeypatch, ss_items, batch):
    (arr, lens), want, _ = world.case(batch)
    pair = world.pair(gpu, "natural")
    monkeypatch.setenv("LRM_SS_ITEMS", str(ss_items))
    try:
        for di in pair:
            capi.lib.lrm_debug_reload_env(di.handle)           # the map overrides are read again; the tables stay
            di.set_map_options(seed_rounds=1)
        got_f, best_f, _ = W._device(pair[0], gpu, arr, lens, S, THRES)
        got_0, best_0, _ = W._device(pair[1], gpu, arr, lens, S, THRES)
    finally:
        monkeypatch.delenv("LRM_SS_ITEMS")
        for di in pair:
            capi.lib.lrm_debug_reload_env(di.handle)
            di.set_map_options(seed_rounds=1)
    assert np.array_equal(got_f, got_0) and np.array_equal(best_f, best_0), (ss_items, batch)
    W._compare(got_f, best_f, want, 1, (ss_items, batch, "bitmap"))
    W._compare(got_0, best_0, want, 1, (ss_items, batch, "no bitmap"))
