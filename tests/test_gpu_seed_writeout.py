"""seed_search_kernel's survivor lists (seed_kernels.hip: the LDS lists of a workgroup, their write-out by phase) through
every launch form, against brute force.

What the vote kernels leave per (read, phase) -- key, count and bucket of both entries (lrm_debug_vote_results) -- is
compared with the brute-force top two of tests/constructed.py (census + vote_top2), which knows nothing of the device,
and best[] with the CPU oracle.  On a clean read every seed survives and votes for one bucket, so one lost, duplicated or
misplaced survivor record changes val1 of its phase.

One text (tests/constructed.py: plant) with a 120-base repeat in three copies (1 < rr < thres) and a 24-mer in 310 copies
(rr >= thres = 300; with thres = 2 the first kind is over the threshold too).  One batch per seed length S:

  * clean reads (substrings of the text's unique tail) with len - S = 63, 64, 65 (one wavefront, its edge, a second one),
    2047, 2048, 2049 (one workgroup, its edge, a second workgroup with ONE position), 4096 (two full workgroups: 97 - 98
    survivors of every phase in each, more than a wavefront copies in one round) and 6200 (three workgroups;
    2048 % 21 != 0, so every workgroup starts at another phase);
  * a read through the repeats, a noisy read (12 % substitutions), reads of length 0, S - 1 and S (no seed position);
  * reads that phase 0 does NOT decide, so that the second round of the two-round policy (phases 1 .. S) has work: five
    blocks of the tail in reverse order (24 / 22 / 20 / 18 / 16 % of the read: the top two hold 46 % of the seeds, every seed
    survives) and two blocks of 29 % around 42 % of random bases (every survivor is in one of the top two).

seed_rounds 1 runs all phases in one launch (np = S + 1), seed_rounds 2 phase 0 alone (np = 1: ONE list of up to SS_ITEMS
entries) and then phases 1 .. S (np = S) for the reads phase 0 left open: there only those reads' later phases are
compared.  S = 20 is the seed table's length (the loop of shared table lines); S = 16 and 24 on the same handle take the
generic loop with P = 17 and 25."""
import numpy as np
import pytest

import constructed as K
import orc
from longreadmapper_amd import capi, index, mapper
from longreadmapper_amd.records import ENTRY_DT

pytestmark = pytest.mark.gpu

POSITIONS = (63, 64, 65, 2047, 2048, 2049, 4096, 6200)      # len - S of the clean reads
TAIL = 7000                                                 # unique bases behind the planted strings


def _text():
    rng = np.random.default_rng(90)
    rep, hot = K._filler(rng, 120), K._filler(rng, 24)
    spec = [dict(name="rep", seq=rep, copies=3), dict(name="hot", seq=hot, copies=310)]
    body = K.plant(spec, seed=9, k=16)
    pl = K.plant(spec, seed=9, k=16, length=len(body.seq) + TAIL)
    assert pl.seq[:len(body.seq) - 100] == body.seq[:len(body.seq) - 100]
    return pl, len(pl.seq) - TAIL


def _reads(seq, tail0, S):
    """The batch for seed length S -> (list of reads, index of the first read phase 0 must leave open)."""
    rng = np.random.default_rng(91)
    tail = seq[tail0:]
    reads = [tail[17 * i:17 * i + p + S] for i, p in enumerate(POSITIONS)]
    reads.append(seq[:3000])                                                     # through the three copies of the repeat
    noisy = np.frombuffer(tail[300:5300], dtype=np.uint8).copy()
    hit = rng.random(len(noisy)) < 0.12
    noisy[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[(K._CODE[noisy[hit]] + rng.integers(1, 4, size=int(hit.sum()))) % 4]
    reads.append(bytes(noisy))
    reads += [b"", tail[:S - 1], tail[:S]]
    first_open = len(reads)
    for total in (4096 + S, 6200 + S):
        cuts = np.cumsum([0] + [total * pct // 100 for pct in (16, 18, 20, 22)] + [total])
        cuts[-1] = total
        reads.append(b"".join(tail[cuts[b]:cuts[b + 1]] for b in (4, 3, 2, 1, 0)))
        a = total * 29 // 100
        reads.append(tail[a + 40:2 * a + 40] + K._filler(rng, total - 2 * a) + tail[:a])
    return reads, first_open


def _top2_all_phases(reads, S, thres, cen, rank):
    """Brute force: (n, S + 1, 6) uint64, the vote of every phase of every read (constructed.phase0_hits for every phase:
    seed j = ph, ph + P, ... below len - S gives, when 0 < count < thres, the keys pos - j in suffix-array row order)."""
    P = S + 1
    out = np.zeros((len(reads), P, 6), dtype=np.uint64)
    n_surv = np.zeros((len(reads), P), dtype=np.int64)
    for i, r in enumerate(reads):
        nj = max(len(r) - S, 0)
        if nj == 0:
            continue
        codes = K._codes(np.frombuffer(r, dtype=np.uint8), S)[:nj]
        cnt = cen.count_codes(codes)
        first = cen.first_positions(codes)
        for ph in range(P):
            keys = []
            for j in range(ph, nj, P):
                c = int(cnt[j])
                if c == 1 and thres > 1:
                    keys.append((int(first[j]) - j) & K.U64)
                elif 1 < c < thres:
                    keys += [(p - j) & K.U64 for p in sorted(cen.positions(int(codes[j])), key=lambda x: rank[x])]
                n_surv[i, ph] += 0 < c < thres
            out[i, ph] = [x for e in K.vote_top2(keys)[1] for x in e]
    return out, n_surv


class _World:
    def __init__(self):
        self.pl, self.tail0 = _text()
        self.hi = index.HostIndex.build([self.pl.array()], hlen=8)
        assert bytes(self.hi.content()) == K.index_text([self.pl.seq])
        K.check_sa(self.hi.content(), self.hi.sa())
        sa = self.hi.sa().astype(np.int64)
        self.rank = np.empty(len(sa), dtype=np.int64)
        self.rank[sa] = np.arange(len(sa))
        self.oi = orc.OracleIndex.from_host_index(self.hi)
        self.cen, self.batch, self.want = {}, {}, {}

    def case(self, S, thres):
        """Batch, brute-force votes and the oracle's best[] for (S, thres): computed once, never changed."""
        if S not in self.cen:
            self.cen[S] = K.census(self.hi.content(), S)
            reads, first_open = _reads(self.pl.seq, self.tail0, S)
            arr = np.zeros((len(reads), max(len(r) for r in reads) + 1), dtype=np.uint8)
            for i, r in enumerate(reads):
                arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
            self.batch[S] = (reads, arr, np.array([len(r) for r in reads], dtype=np.uint32), first_open)
        if (S, thres) not in self.want:
            reads, arr, lens, first_open = self.batch[S]
            cen = self.cen[S]
            top, n_surv = _top2_all_phases(reads, S, thres, cen, self.rank)
            best, _ = self.oi.seed_batch(arr, lens, S, thres)
            nseeds = lens.astype(np.int64) // (S + 1)
            decided0 = (nseeds > 0) & (5 * (top[:, 0, 1] + top[:, 0, 4]).astype(np.int64) > 3 * nseeds)
            # the batch has the properties it is built for
            assert cen.count(self.pl.seq[self.pl.where["hot"][0]:][:S]) >= 300
            assert cen.count(self.pl.seq[self.pl.where["rep"][0] + 30:][:S]) == 3
            assert not decided0[first_open:].any() and decided0[:len(POSITIONS)].all()
            if thres > 3:
                for i, p in enumerate(POSITIONS):                  # clean: every position a survivor, one bucket per phase
                    assert int(n_surv[i].sum()) == p and (top[i, :, 1].astype(np.int64) == n_surv[i]).all()
                assert n_surv[6].min() >= 2 * 2048 // (S + 1) > 64 * 2
                assert (n_surv[first_open] >= (4096 // (S + 1)) - 6).all()          # five blocks: four junctions
            self.want[(S, thres)] = (top, best, decided0)
        return self.batch[S], self.want[(S, thres)]


@pytest.fixture(scope="module")
def world():
    return _World()


def _device(di, gpu, arr, lens, S, thres, counting=False):
    import torch
    dm = mapper.DeviceMapper(di, len(lens), int(lens.max()), S, thres, device=gpu)
    try:
        dev = torch.device("cuda", gpu)
        if counting:
            dm.set_counting(True)
        dm.seed(torch.from_numpy(arr).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev))
        torch.cuda.synchronize(dev)
        best = dm.best[:len(lens)].cpu().numpy().reshape(-1).view(ENTRY_DT)
        return dm.debug_vote_results(len(lens)), best, dm.stats()
    finally:
        dm.close()


def _compare(got, best, want, rounds, what):
    top, want_best, decided0 = want
    for i in range(len(top)):
        phases = range(top.shape[1]) if rounds == 1 or not decided0[i] else range(1)
        for ph in phases:
            assert np.array_equal(got[i, ph], top[i, ph]), (what, "read", i, "phase", ph, got[i, ph].tolist(), top[i, ph].tolist())
    assert np.array_equal(best, want_best), (what, "best", np.nonzero(best != want_best)[0].tolist())


# (S, thres, LRM_SS_ITEMS, seed_table_share): share 4 with 8-byte slots is the table form seed_search_kernel has an
# instantiation of its own for, share 2 (6-byte slots) takes the generic one
CONFIGS = [(20, 300, None, 4), (20, 300, 1024, 4), (20, 300, 4096, 4), (20, 2, None, 4), (16, 300, None, 4), (24, 300, None, 4),
           (24, 2, 4096, 4), (20, 300, None, 2), (20, 2, 4096, 2)]


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("S,thres,ss_items,share", CONFIGS)
def test_survivor_lists(gpu, world, monkeypatch, S, thres, ss_items, share, rounds):
    (reads, arr, lens, _), want = world.case(S, thres)
    if ss_items:
        monkeypatch.setenv("LRM_SS_ITEMS", str(ss_items))
    di = index.DeviceIndex.upload(world.hi, gpu, seed_table=1, seed_table_len=20, seed_table_share=share)
    try:
        t = di.tables()
        assert t["seed_table_len"] == 20 and t["seed_table_share"] == share and t["seed_table_slot_bytes"] == (8 if share == 4 else 6)
        capi.lib.lrm_debug_reload_env(di.handle)               # the overrides are read once per handle
        di.set_map_options(seed_rounds=rounds)
        got, best, _ = _device(di, gpu, arr, lens, S, thres)
    finally:
        di.close()
    _compare(got, best, want, rounds, (S, thres, ss_items, share, rounds))


@pytest.mark.parametrize("S", [20, 24])
def test_counting_build(gpu, world, S):
    """The counting instantiation writes the same lists, and its seed counters are what the launch geometry says: every
    position below len - S is evaluated once; in the shared-lines loop (S = the table's length) every lane of a wavefront
    that holds a position takes part in one line fetch."""
    (reads, arr, lens, _), want = world.case(S, 300)
    di = index.DeviceIndex.upload(world.hi, gpu, seed_table=1, seed_table_len=20)
    try:
        side = di.tables()["seed_table_side_entries"]
        di.set_map_options(seed_rounds=1)
        got, best, st = _device(di, gpu, arr, lens, S, 300, counting=True)
    finally:
        di.close()
    _compare(got, best, want, 1, (S, "counting"))
    pos = np.maximum(lens.astype(np.int64) - S, 0)
    assert st["seeds_evaluated"] == int(pos.sum()), (st["seeds_evaluated"], int(pos.sum()))
    if S == 20:
        lanes = int(((pos + 63) // 64 * 64).sum())
        assert st["seed_table_lookups"] >= lanes and (side or st["seed_table_lookups"] == lanes), (st["seed_table_lookups"], lanes, side)
        assert side or st["seed_rank_requests"] == 0
