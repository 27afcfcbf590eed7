"""The counting build of gact_bs_kernel (lrm_workspace_set_counting, stats()["bs_*"]) against a model of the kernel's
control flow, on constructed batches: ONT-profile reads over a random text the test lays out itself (gact_cases.batch_of),
T = 320, O = 120, W = 128 unless a test says otherwise.

The model (tests/bs_flow.py, `_wave`) is written from the stream-word formulas of gact_bs_kernels.hip, not from its output: a stream word
of the query whose bit 0 is read base a_hi holds a lane's free-exit point iff 0 <= a_hi - tq < 32, a word of the text
starting at b_lo iff 0 <= tt - b_lo < 32, for lanes that have a tile -- a lane without one holds none.  Pass 1 starts at
anti-diagonal S0 (the wavefront's largest tq + tt, rounded up to 32) with the words a_hi = A0, A0 - 32, A0 - 64 and
b_lo = B0 - 31, B0 + 1, B0 + 33 (A0 = S0/2 + 32, B0 = S0 - A0), shifts a word in every 32 pairs, and runs a pair masked
iff some word in the window holds a free-exit point at the pair's even step.  Pass 2 recomputes block c (anti-diagonals
32c .. 32c + 31) in full width iff one of a_hi = 16(c + 1) + 31 - {0, 32, 64}, b_lo = 16c - 32 + {0, 32, 64} does, on the
32-point window otherwise, and leaves the blocks from c on out when no lane's walk has a step at or beyond 32c.
Which tiles a lane runs (tq, tt, and the anti-diagonal of the walk's last step) comes from the reference alignment of
its read: tests/gact_ref.py's per-tile trace, whose ops are checked against the oracle's.  Lanes take reads from a
queue in lane order; a fenced read leaves its lane asking again."""
import zlib

import numpy as np
import pytest

import gact_cases
import gact_ref
import orc
from bs_flow import _holds, _tile, _wave, _model  # noqa: F401  (the model, shared with the company tests)
from longreadmapper_amd import capi, index, mapper

pytestmark = pytest.mark.gpu

T, O, W = 320, 120, 128
BS_K = gact_cases.BS_K
ONT = (0.04, 0.03, 0.03)                      # synth.ONT: substitutions, insertions, deletions
FENCED_KEY = (1 << 64) - 5                    # a wrapped diagonal: locus_resolve fences the read (meta_r = 0)
BITSLICED = 4


def _pairs(lengths, tag):
    """Square pairs, a function of (tag, k, length) alone: batches of one tag share their first reads."""
    out = []
    for k, n in enumerate(lengths):
        ref = gact_cases.rnd(n + 300, tag, k)
        q = gact_cases._mutate(np.random.default_rng([zlib.crc32(tag.encode()), k, n]), ref, *ONT)
        assert len(q) >= n
        out.append((q[:n], ref[:n]))
    return out


_REF = {}                                     # (q, d, gact) -> ((score, ops), tiles): computed once per module run


def _reference(pairs, gact):
    """Per read: (score, ops) of the oracle and the tiles [(tq, tt, anti-diagonal of the walk's last step)]."""
    new = [p for p in pairs if p + (gact,) not in _REF]
    for (q, d), (score, ops, trace) in zip(new, gact_ref.align_many(new, *gact)):
        o_score, o_ops, _ = orc.gact(q, d, *gact)
        assert (o_score, o_ops) == (score, ops)
        at, row = 0, []
        for t in trace:
            a = b = 0
            while (a, b) != t["stop"]:
                last_step = a + b
                op = ops[at]
                at += 1
                a, b = a + (op != ord("D")), b + (op != ord("I"))
            row.append((t["tq"], t["tt"], last_step))
        assert at + trace.tail == len(ops)
        _REF[(q, d, gact)] = ((score, ops), row)
    return [_REF[p + (gact,)][0] for p in pairs], [_REF[p + (gact,)][1] for p in pairs]


class _Batch:
    def __init__(self, gpu, pairs, fenced=()):
        b = gact_cases.batch_of(pairs)
        self.pairs, self.fenced = pairs, set(fenced)
        self.keys = np.array([FENCED_KEY if k in self.fenced else key for k, key in enumerate(b["keys"])], dtype=np.uint64)
        self.arr, self.lens = gact_cases.read_matrix(b["reads"])
        self.hi = index.HostIndex.build(b["seqs"], hlen=8)
        self.di = index.DeviceIndex.upload(self.hi, gpu)
        self.gpu = gpu
        self._ref = {}

    def reference(self, gact):
        if gact not in self._ref:
            self._ref[gact] = _reference(self.pairs, gact)
        return self._ref[gact]

    def run(self, gact, counting, waves=0):
        """-> (results, what stats() gained over the call) of one extend() on a workspace of its own."""
        import torch
        n = len(self.lens)
        self.di.set_map_options(gact_impl=BITSLICED, bs_waves=waves)
        dm = mapper.DeviceMapper(self.di, n, self.arr.shape[1] - 1, gact=gact, device=self.gpu)
        try:
            dm.set_counting(counting)
            dm.best[:n, 0] = torch.from_numpy(self.keys.view(np.int64)).cuda()
            before = dm.stats()
            dm.extend(torch.from_numpy(self.arr).cuda(), torch.from_numpy(self.lens.astype(np.int32)).cuda())
            torch.cuda.synchronize()
            after = dm.stats()
            return dm.results(n), {k: after[k] - before[k] for k in after}
        finally:
            dm.close()
            self.di.set_map_options()

    def check_results(self, got, gact):
        want, _ = self.reference(gact)
        for k, (score, ops) in enumerate(want):
            if k in self.fenced:
                assert (int(got["meta_r"][k]), int(got["score"][k]), int(got["n_ops"][k])) == (0, -1, 0), k
                continue
            assert int(got["meta_r"][k]) == 1 and int(got["score"][k]) == score and int(got["n_ops"][k]) == len(ops), k
            assert bytes(got["ops"][k, :len(ops)]) == ops, k

    def check_counters(self, st, waves, gact):
        _, tiles = self.reference(gact)
        want = _model(tiles, self.fenced, waves, gact)
        got = {k: st[k] for k in want if k != "blocks_per_tile_sum"}
        print(got)
        assert got == {k: v for k, v in want.items() if k != "blocks_per_tile_sum"}
        assert st["bs_blocks_windowed"] + st["bs_blocks_full"] + st["bs_blocks_skipped"] == want["blocks_per_tile_sum"]
        return want

    def close(self):
        self.di.close()


@pytest.fixture(scope="module")
def lockstep(gpu):
    b = _Batch(gpu, _pairs([700] * 128, "lockstep"))
    yield b
    b.close()


def test_lockstep_batch_is_windowed_wherever_no_tile_ends(lockstep):
    """128 reads of 700 bases, two full wavefronts: the first two tiles of every read are whole (n - i >= T, m - j >= T), and
    the model asserts that no block of a wave-tile of whole tiles is full-width; the counts equal the model's exactly."""
    got, st = lockstep.run((T, O, W), True)
    lockstep.check_results(got, (T, O, W))
    want = lockstep.check_counters(st, 2, (T, O, W))
    assert want["bs_blocks_windowed"] >= 2 * 2 * 12 and want["bs_blocks_full"] > 0
    assert want["bs_pass1_pairs_plain"] > want["bs_pass1_pairs_masked"] > 0


def test_exhausted_lanes_carry_no_free_exit_point(gpu):
    """65 reads: the second wavefront has one live lane and 63 that never get a read; its counts are those of the one."""
    b = _Batch(gpu, _pairs([700] * 65, "lockstep"))
    try:
        got, st = b.run((T, O, W), True)
        b.check_results(got, (T, O, W))
        want = b.check_counters(st, 2, (T, O, W))
        _, tiles = b.reference((T, O, W))
        alone = _model(tiles[64:], (), 1, (T, O, W))
        assert alone["bs_blocks_windowed"] >= 2 * 12 and alone["bs_blocks_windowed"] < want["bs_blocks_windowed"]
    finally:
        b.close()


def test_fenced_lanes_carry_no_free_exit_point(gpu):
    """Every 7th of 100 reads fenced, one wavefront: a fenced read leaves its lane without a tile for a round of the queue
    (or for good, at the end of the batch) next to lanes in whole tiles."""
    b = _Batch(gpu, _pairs([700] * 100, "lockstep"), fenced=range(0, 100, 7))
    try:
        got, st = b.run((T, O, W), True, waves=1)
        b.check_results(got, (T, O, W))
        want = b.check_counters(st, 1, (T, O, W))
        assert want["bs_blocks_windowed"] > want["bs_blocks_full"] > 0
    finally:
        b.close()


@pytest.fixture(scope="module")
def unequal(gpu):
    lengths = [int(x) for x in np.random.default_rng(41).integers(330, 2001, size=96)]
    lengths[:3] = [330, 2000, 641]
    b = _Batch(gpu, _pairs(lengths, "unequal"))
    yield b
    b.close()


def test_unequal_lengths_through_refills(unequal):
    """96 reads of 330 .. 2000 bases on one wavefront: 32 reads wait in the queue, lanes run dry at different times."""
    got, st = unequal.run((T, O, W), True, waves=1)
    unequal.check_results(got, (T, O, W))
    want = unequal.check_counters(st, 1, (T, O, W))
    nblk = (2 * (T - O) + BS_K - 1) // BS_K
    assert want["bs_refill_rounds"] > 3 and st["bs_wave_tiles"] * nblk >= want["blocks_per_tile_sum"]
    assert st["bs_blocks_windowed"] + st["bs_blocks_full"] + st["bs_blocks_skipped"] == want["blocks_per_tile_sum"]


def test_narrow_band_is_full_width_throughout(lockstep):
    """W = 64: every step is the masked one and every block full-width, whatever the lanes hold."""
    got, st = lockstep.run((T, O, 64), True)
    lockstep.check_results(got, (T, O, 64))
    lockstep.check_counters(st, 2, (T, O, 64))
    assert st["bs_blocks_windowed"] == 0 and st["bs_pass1_pairs_plain"] == 0 and st["bs_blocks_full"] > 0


def test_counting_off_counts_nothing_and_changes_nothing(lockstep, unequal):
    for b, waves in ((lockstep, 0), (unequal, 1)):
        on, st_on = b.run((T, O, W), True, waves)
        off, st_off = b.run((T, O, W), False, waves)
        assert all(st_off[k] == 0 for k in capi.BS_COUNTERS) and st_on["bs_wave_tiles"] > 0
        assert st_off["gact_tiles"] == st_on["gact_tiles"] > 0
        for key in ("n_ops", "score", "meta_r", "meta", "best"):
            assert on[key].tobytes() == off[key].tobytes(), key
        for k, n_ops in enumerate(on["n_ops"]):
            assert on["ops"][k, :n_ops].tobytes() == off["ops"][k, :n_ops].tobytes(), k
