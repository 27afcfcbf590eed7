"""tests/phase_cases.py on the CPU: every case reaches the edge it is named for, the kill rule holds on its own, and the
oracle -- its phases above 0, its loop over the phase results and the hit list mapq_ref / rival_ref read from its trace --
agrees with the brute-force references on every case.  The GPU file (test_gpu_phase_cases.py) then holds the device to the
same brute-force results, without the oracle."""
import numpy as np
import pytest

import constructed as K
import mapq_ref
import orc
import phase_cases as PC
import rival_ref

S, P = PC.S, PC.P
NAMES = [c["name"] for c in PC.cases()[1]]


@pytest.fixture(scope="module")
def world():
    seqs, cases = PC.cases()
    oi = orc.OracleIndex.build(seqs, hlen=8)
    content = oi.content()
    assert bytes(content) == K.index_text(seqs)
    K.check_sa(content, oi.sa())                          # from here on the oracle's suffix array is THE suffix array
    cen = K.census(content, S)
    sa = oi.sa().astype(np.int64)
    rank = np.empty(len(sa), dtype=np.int64)
    rank[sa] = np.arange(len(sa))
    derived = {}

    def get(name):
        c = next(c for c in cases if c["name"] == name)
        if name not in derived:
            derived[name] = PC.derive(c, cen, rank)
        return c, derived[name]
    return dict(oi=oi, cen=cen, rank=rank, get=get, seqs=seqs, cases=cases)


def test_cases_build_the_same_every_time():
    seqs, cases = PC.cases()
    PC.cases.cache_clear()
    seqs2, cases2 = PC.cases()
    assert seqs == seqs2 and [(c["name"], c["read"], c["aim"]) for c in cases] == [(c["name"], c["read"], c["aim"]) for c in cases2]
    assert len(set(NAMES)) == len(NAMES) and 20_000 <= len(seqs[0]) <= 100_000
    assert all(20 <= len(c["read"]) <= 4097 for c in cases)


def test_phase0_hits_is_phase_0(world):
    c, r = world["get"]("break-at-3")
    assert K.phase0_hits(c["read"], S, c["thres"], world["cen"], world["rank"]) == r["hits"][0] != []


@pytest.mark.parametrize("c", range(P))
def test_kill_rule(world, c):
    """One substituted base of class c in every window of a one-locus read: full counts in phase c + 1 (mod 21), nothing in
    any other phase.  Full is one seed per window, less the last where its j is not below len - S (alnmain.c:353)."""
    at = PC.L_AT
    locus = world["seqs"][0][at:at + 20 * P]
    for n in (20, 7):
        read = PC.kill(locus[:P * n], [(w, c) for w in range(n)])
        spared = (c + 1) % P
        for p in range(P):
            got = PC.phase_hits(read, p, S, 300, world["cen"], world["rank"])
            last = p + P * (n - 1) < len(read) - S
            assert got == ([at] * (n if last else n - 1) if p == spared else []), (c, n, p)
            assert last == (p == 0)


@pytest.mark.parametrize("name", NAMES)
def test_predicate_holds(world, name):
    c, r = world["get"](name)
    c["predicate"](r)
    assert r["d"] == c["aim"]["d"] and r["best"][0] == c["aim"]["key"]
    if "val" in c["aim"]:
        assert r["best"][1] == c["aim"]["val"]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_with_brute_force(world, name):
    c, r = world["get"](name)
    oi = world["oi"]
    tr = oi.seed_read(c["read"], S, c["thres"], trace=True)
    assert tr["best"] == r["best"] and tr["phases"] == r["phases"]
    assert [rec["iter"] for rec in tr["phase_recs"]] == list(range(len(r["tops"])))
    num_seeds = len(c["read"]) // P
    for rec, (v, top) in zip(tr["phase_recs"], r["tops"]):
        assert [rec["top1"], rec["top2"]] == top and rec["v"] == v, (name, rec["iter"])
        assert rec["decided"] == int(5 * v > 3 * num_seeds)
    # the hits of the evidence phases as mapq_ref reads them from the trace, and the two records
    keys, d, best = mapq_ref.hits_of(oi, c["read"], S, c["thres"])
    assert d == r["d"] and best == r["best"] and [int(k) for k in keys] == r["evidence"]
    assert mapq_ref.record(oi, c["read"], S, c["thres"]) == r["rec"]
    assert rival_ref.entry(oi, c["read"], S, c["thres"]) == r["rival"]
