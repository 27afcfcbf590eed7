"""seed_search_kernel's shared-lines loop with two line fetches in flight per lane (seed_kernels.hip): the fetch of position
j + 256 leaves before the line of position j is searched, in two register sets that change roles, and a wavefront's count
of iterations is worked out in front of the loop.  What can go wrong is at the ends: a last iteration that is partial, a
count of iterations that is odd or even, a workgroup with one position, a quad of four lanes with one, two or three seeds.

Reads on a synth.reference text, seed length 20 (the seed table's length), with len - 20 = 1 ... 4097 positions around every
multiple of a wavefront (64), of an iteration (256) and of a workgroup (1024 / 2048 / 4096 by LRM_SS_ITEMS), clean and with
10 % substitutions; lengths 19 and 20 have no seed.  Compared per (read, phase) with the brute-force vote of
tests/constructed.py (as tests/test_gpu_seed_writeout.py does: on a clean read every position is a survivor and votes for
one bucket, so a lost, doubled or misplaced survivor changes val1 of its phase; the vote sorts its hits, so the order of a
list does not show) and best[] with the CPU oracle.  seed_rounds 2 and a handle with two positions per table line
(6-byte slots) take the loops with one fetch in flight, which must be as they were."""
import numpy as np
import pytest

import constructed as K
import orc
import test_gpu_seed_writeout as W
from longreadmapper_amd import capi, index, synth

pytestmark = pytest.mark.gpu

S, THRES = 20, 300
# positions with a seed (len - S): 1, 2, 3 mod 4 at every edge; 66 and 2050 are the 2 mod 4 ones; 700 and 1300 give
# wavefronts an odd count of iterations above one (3 and 5, 6: a whole double step, then a last one without a partner)
POSITIONS = (1, 63, 64, 65, 66, 255, 256, 257, 700, 1300, 2047, 2048, 2049, 2050, 4095, 4097)
TEXT = 60_000


def _noisy(read, rng, rate=0.10):
    a = np.frombuffer(read, dtype=np.uint8).copy()
    hit = rng.random(len(a)) < rate
    a[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[(K._CODE[a[hit]] + rng.integers(1, 4, size=int(hit.sum()))) % 4]
    return bytes(a)


class _World:
    def __init__(self):
        ref = synth.reference(TEXT, seed=23)
        self.seq = bytes(ref)
        self.hi = index.HostIndex.build([ref], hlen=10)
        sa = self.hi.sa().astype(np.int64)
        self.rank = np.empty(len(sa), dtype=np.int64)
        self.rank[sa] = np.arange(len(sa))
        self.oi = orc.OracleIndex.from_host_index(self.hi)
        self.cen = K.census(self.hi.content(), S)
        self.cases = {}

    def reads(self, name):
        rng = np.random.default_rng(7)
        clean = [self.seq[131 * i:131 * i + p + S] for i, p in enumerate(POSITIONS)]
        if name == "edges":                       # every length clean, the longer ones noisy too, and the two without a seed
            return clean + [_noisy(r, rng) for r in clean if len(r) >= 255] + [self.seq[500:500 + S], self.seq[900:900 + S - 1]]
        if name == "one":
            return [clean[-1]]
        if name == "three":
            return [clean[3], _noisy(clean[-2], rng), clean[8]]
        out = []                                  # "seventy": the grid n * blocks_per_read crosses one wavefront's worth of workgroups
        for k in range(70):
            p = POSITIONS[k % len(POSITIONS)]
            r = self.seq[211 * k:211 * k + p + S]
            out.append(_noisy(r, rng) if k % 3 == 2 else r)
        return out

    def case(self, name):
        """Batch, brute-force votes of every phase, the oracle's best[]: computed once per batch, never changed."""
        if name not in self.cases:
            reads = self.reads(name)
            arr = np.zeros((len(reads), max(len(r) for r in reads) + 1), dtype=np.uint8)
            for i, r in enumerate(reads):
                arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
            lens = np.array([len(r) for r in reads], dtype=np.uint32)
            top, n_surv = W._top2_all_phases(reads, S, THRES, self.cen, self.rank)
            best, _ = self.oi.seed_batch(arr, lens, S, THRES)
            nseeds = lens.astype(np.int64) // (S + 1)
            decided0 = (nseeds > 0) & (5 * (top[:, 0, 1] + top[:, 0, 4]).astype(np.int64) > 3 * nseeds)
            if name == "edges":                   # the batch is what it is built to be
                for i, p in enumerate(POSITIONS):
                    assert int(n_surv[i].sum()) == p, (p, int(n_surv[i].sum()))          # clean: every position survives
                noisy = n_surv[len(POSITIONS):-2].sum(axis=1)
                assert (noisy > 0).all() and (noisy < [p for p in POSITIONS if p + S >= 255]).all()
                assert not n_surv[-2:].any() and not decided0.all()                     # (seed_rounds 2 has a second round)
            self.cases[name] = ((arr, lens), (top, best, decided0))
        return self.cases[name]


@pytest.fixture(scope="module")
def world():
    return _World()


# (batch, LRM_SS_ITEMS, seed_table_share, seed_rounds): share 4 is the table form with the pipelined loop's own instantiation,
# share 2 (two positions per line, 6-byte slots) the generic one; seed_rounds 2 launches np = 1 and np = P - 1
CASES = [("edges", None, 4, 1), ("edges", 1024, 4, 1), ("edges", 2048, 4, 1), ("edges", 4096, 4, 1), ("edges", None, 4, 2),
         ("edges", None, 2, 1), ("edges", 4096, 2, 1), ("one", None, 4, 1), ("three", 1024, 4, 1), ("seventy", None, 4, 1),
         ("seventy", 4096, 4, 1)]


@pytest.mark.parametrize("batch,ss_items,share,rounds", CASES)
def test_pipelined_loop(gpu, world, monkeypatch, batch, ss_items, share, rounds):
    (arr, lens), want = world.case(batch)
    if ss_items:
        monkeypatch.setenv("LRM_SS_ITEMS", str(ss_items))
    di = index.DeviceIndex.upload(world.hi, gpu, seed_table=1, seed_table_len=S, seed_table_share=share)
    try:
        t = di.tables()
        assert t["seed_table_len"] == S and t["seed_table_share"] == share and t["seed_table_slot_bytes"] == (8 if share == 4 else 6)
        capi.lib.lrm_debug_reload_env(di.handle)               # the overrides are read once per handle
        di.set_map_options(seed_rounds=rounds)
        got, best, _ = W._device(di, gpu, arr, lens, S, THRES)
    finally:
        di.close()
    W._compare(got, best, want, rounds, (batch, ss_items, share, rounds))
