"""seed_search_kernel's line fetch behind the presence bitmap on the batches of tests/seed_lines_cases.py: a crowded table
line that is line 0 of the table (eight entries in the line, eight more beside it, the overflow mark set), random reads
none of whose seeds is in the text, and reads whose last quad, wavefront and iteration hold one, two or three seeds.

As in tests/test_gpu_seed_filter.py, whose comparison this reuses: every batch runs on a handle with the bitmap and on one
made with LRM_SD_FILTER_KB=0, and both vote entries of every (read, phase), best[] and the vote's tier routing must be
equal between the two and equal to brute force.

Three legs, by the number of table lines.  The launcher takes the form that addresses a line by a 32-bit offset while the
table and the line of zeros at its end lie below 2^32 bytes (lrm_sd_off32: at most 2^25 lines): "natural" (the plan's 2^17
lines) and "small" (LRM_SD_BITS=16, another table size and another offset of the line of zeros) run it, "wide"
(LRM_SD_BITS=26, a table of 4 GiB) runs the form with 64-bit line addresses that longer tables keep."""
import re

import numpy as np
import pytest

import constructed as K
import orc
import seed_lines_cases as L
import test_gpu_seed_filter as TF
import test_gpu_seed_writeout as W
from longreadmapper_amd import index

pytestmark = pytest.mark.gpu

S, THRES = L.S, L.THRES
# leg: (environment, table bits, bitmap bytes, lines per bit)
LEGS = {"natural": (dict(), 17, 16 * 1024, 1), "small": (dict(LRM_SD_BITS="16"), 16, 8 * 1024, 1),
        "wide": (dict(LRM_SD_BITS="26"), 26, 4096 * 1024, 2)}


class _World:
    def __init__(self):
        self.seq = L.forward()
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
            reads = L.batch(name, self.seq)
            arr, lens = L.rows(reads)
            top, n_surv = W._top2_all_phases(reads, S, THRES, self.cen, self.rank)
            best, _ = self.oi.seed_batch(arr, lens, S, THRES)
            nseeds = lens.astype(np.int64) // (S + 1)
            decided0 = (nseeds > 0) & (5 * (top[:, 0, 1] + top[:, 0, 4]).astype(np.int64) > 3 * nseeds)
            self.cases[name] = ((arr, lens), (top, best, decided0), n_surv)
        return self.cases[name]

    def pair(self, gpu, leg):
        """(handle with the bitmap, handle without) of a leg."""
        if leg not in self.handles:
            env, bits, size, per_bit = LEGS[leg]
            base = dict(LRM_SD_BITS=None, LRM_SD_FILTER_KB=None, LRM_HOST_VERBOSE="1")
            opts = dict(seed_table=1, seed_table_len=S, seed_table_share=4, lc_long_max=13)
            with TF._environ(**{**base, **env}) as said:
                with_f = index.DeviceIndex.upload(self.hi, gpu, **opts)
            with TF._environ(**{**base, **env, "LRM_SD_FILTER_KB": "0"}) as said0:
                without = index.DeviceIndex.upload(self.hi, gpu, **opts)
            self.handles[leg] = (with_f, without)
            m = TF.LINE.search(said[0])
            assert m and "not kept" not in said[0], said[0]          # the bitmap was built and kept
            assert (int(m.group(1)), int(m.group(2))) == (size, per_bit), m.group(0)
            assert "seed table:" in said0[0] and "seed filter" not in said0[0], said0[0]
            # the crowded line: eight entries beside it at the least (sixteen asked for room in eight slots)
            side = int(re.search(r"(\d+) side entries", said[0]).group(1))
            assert side >= 8, said[0]
            for di in self.handles[leg]:
                t = di.tables()
                assert (t["seed_table_len"], t["seed_table_share"], t["seed_table_slot_bytes"]) == (S, 4, 8)
                assert t["seed_table_bits"] == bits
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


@pytest.mark.parametrize("batch", L.BATCHES)
@pytest.mark.parametrize("leg", list(LEGS))
def test_line_fetch_changes_nothing(gpu, world, leg, batch):
    (arr, lens), want, n_surv = world.case(batch)
    if batch == "random":
        assert not n_surv.any()                                      # no survivor by brute force: none on the device (below)
    else:
        assert n_surv.any()
    with_f, without = world.pair(gpu, leg)
    got_f, best_f, st_f = W._device(with_f, gpu, arr, lens, S, THRES)
    got_0, best_0, st_0 = W._device(without, gpu, arr, lens, S, THRES)
    assert np.array_equal(got_f, got_0), (leg, batch, np.argwhere((got_f != got_0).any(axis=2))[:8].tolist())
    assert np.array_equal(best_f, best_0), (leg, batch)
    for f in ("vote_tier2_items", "vote_tier3_items", "reads_decided_phase0"):       # the vote's routing goes by cnt[] and hits[]
        assert st_f[f] == st_0[f], (leg, batch, f, st_f[f], st_0[f])
    W._compare(got_f, best_f, want, 1, (leg, batch, "bitmap"))
    W._compare(got_0, best_0, want, 1, (leg, batch, "no bitmap"))
    if batch == "random":
        assert not got_f[:, :, [1, 4]].any(), (leg, "a vote for a read without a seed in the text")
