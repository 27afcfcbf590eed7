"""The seed stage's later phases, decide_kernel, and the evidence walks of mapq_vote_kernel and rival_locus_kernel against
brute force on the constructed reads of tests/phase_cases.py.

Nothing here comes from the oracle: the text is planted, its suffix array is proved by check_sa, every hit stream is
census + suffix-array rank, the loop over the phases is phase_cases.decide_ref, the records are mapq_ref.record_of_hits and
rival_ref.rival_of_hits_scalar on those brute-force keys.  One batch holds every case's read (some twice, at other rows) and
further constructed reads; every read is compared exactly, field by field, under every round policy, both vote paths and four
index forms, on device buffers and through the host boundary.  test_phase_cases_cpu.py checks the cases themselves (each
reaches the edge it is named for) and holds the oracle to the same references."""
import numpy as np
import pytest

import constructed as K
import phase_cases as PC
from longreadmapper_amd import capi, index, mapper

pytestmark = pytest.mark.gpu

S, P, THRES = PC.S, PC.P, PC.THRES
SMALL = dict(lc_long_max=13)       # every handle of this module stays small
FORMS = {"default": {}, "seed-table": dict(seed_table=1), "no-seed-table-lc13": dict(seed_table=0, lc_long=13),
         "sa-sampled-4": dict(sa_sampled=4)}
FIELDS = ("n1", "n2", "radius", "mapq", "phase", "flags")
_world = {}


def _rows(reads, width=0):
    arr = np.zeros((len(reads), max(width, max(len(r) for r in reads) + 1)), dtype=np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return arr, np.array([len(r) for r in reads], dtype=np.uint32)


def world():
    """The CPU side, once: the host index of the planted text, the batch, and per read what brute force derives."""
    if _world:
        return _world
    seqs, cases = PC.cases()
    hi = index.HostIndex.build([np.frombuffer(s, dtype=np.uint8) for s in seqs], hlen=8)
    assert bytes(hi.content()) == K.index_text(seqs)
    K.check_sa(hi.content(), hi.sa())
    cen = K.census(hi.content(), S)
    sa = hi.sa().astype(np.int64)
    rank = np.empty(len(sa), dtype=np.int64)
    rank[sa] = np.arange(len(sa))
    at = PC.L_AT
    locus = seqs[0][at:at + 20 * P]
    extra = [dict(name="steer-%d-%d" % (d, h), read=PC.steer(locus, 20, d, h), thres=THRES) for d in (0, 5, 13, 20) for h in (8, 12)]
    items = list(cases) + list(cases[::-3]) + extra        # every case, every third again in reverse order, the extra reads
    derived = {}
    for c in items:
        if c["name"] not in derived:
            derived[c["name"]] = PC.derive(c, cen, rank)
            if "predicate" in c:
                c["predicate"](derived[c["name"]])
    assert len(items) >= 64
    _world.update(hi=hi, items=items, derived=derived)
    return _world


def expected(items, derived):
    """-> dict of arrays for a batch: best (n, 3), rival (n, 3), rec {field: (n,)}, d (n,), votes (n, P, 6), voted (n,);
    passes0: phase 0 passes (5 v > 3 num_seeds there); seeds0 / seeds: seed positions of phase 0 / of all phases"""
    n = len(items)
    out = dict(best=np.zeros((n, 3), dtype=np.uint64), rival=np.zeros((n, 3), dtype=np.uint64), d=np.zeros(n, dtype=np.int64),
               rec={f: np.zeros(n, dtype=np.int64) for f in FIELDS}, votes=np.zeros((n, P, 6), dtype=np.uint64),
               voted=np.zeros(n, dtype=bool), passes0=np.zeros(n, dtype=bool), seeds0=np.zeros(n, dtype=np.int64),
               seeds=np.zeros(n, dtype=np.int64))
    for i, c in enumerate(items):
        r = derived[c["name"]]
        out["best"][i], out["rival"][i], out["d"][i] = r["best"], r["rival"], r["d"]
        for f, x in zip(FIELDS, r["rec"]):
            out["rec"][f][i] = x
        out["voted"][i] = len(c["read"]) >= P              # num_seeds > 0: the phases are voted at all
        out["passes0"][i] = bool(r["tops"]) and 5 * r["tops"][0][0] > 3 * (len(c["read"]) // P)
        out["seeds0"][i] = len(range(0, max(len(c["read"]) - S, 0), P))
        out["seeds"][i] = max(len(c["read"]) - S, 0)
        for p in range(P):
            out["votes"][i, p] = [x for e in K.vote_top2(r["hits"][p])[1] for x in e]
    return out


def _same_best(got, want, what):
    got = np.stack([got["key"], got["val"], got["bucket"]], axis=1) if got.dtype.names else np.asarray(got).view(np.uint64).reshape(-1, 3)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())


def _same_records(got, want, what):
    for f in FIELDS:
        bad = np.flatnonzero(got[f].astype(np.int64) != want[f])
        assert bad.size == 0, (what, f, bad[:8].tolist(), [tuple(int(got[i][g]) for g in FIELDS) for i in bad[:3]],
                               [tuple(int(want[g][i]) for g in FIELDS) for i in bad[:3]])
    assert not got["_pad"].any(), what


@pytest.fixture(scope="module")
def forms(gpu):
    open_ = {}

    def get(name):
        if name not in open_:
            open_[name] = index.DeviceIndex.upload(world()["hi"], gpu, **SMALL, **FORMS[name])
            t = open_[name].tables()
            if "seed_table" in FORMS[name]:                # the seed table really is there / really is not
                assert t["seed_table_len"] == (S if FORMS[name]["seed_table"] else 0)
        return open_[name]
    yield get
    for di in open_.values():
        di.close()


def _device(dm, arr, lens, votes=False):
    """seed (with the mapping-quality stage), then the rival stage, on device buffers -> best, records, rival [, votes]"""
    import torch
    n = len(lens)
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    dm.seed(torch.from_numpy(arr).cuda(), d_lens)
    rival = dm.rival(d_lens, n)
    torch.cuda.synchronize()
    res = dm.results(n)
    st = dm.stats()                                        # raises if the sticky kernel-error word of the workspace is set
    out = dict(best=res["best"].copy(), mapq=res["mapq"].copy(), rival=rival.cpu().numpy().view(np.uint64).reshape(-1, 3), stats=st)
    if votes:
        out["votes"] = dm.debug_vote_results(n)
    return out


def _check_device(got, want, what):
    _same_best(got["best"], want["best"], (what, "best"))
    _same_records(got["mapq"], want["rec"], (what, "mapq"))
    bad = np.flatnonzero((got["rival"] != want["rival"]).any(axis=1))
    assert bad.size == 0, (what, "rival", bad[:8].tolist(), got["rival"][bad[:3]].tolist(), want["rival"][bad[:3]].tolist())


@pytest.mark.parametrize("form", list(FORMS))
def test_best_under_every_round_policy_and_vote_path(gpu, forms, map_options, form):
    w = world()
    di = forms(form)
    arr, lens = _rows([c["read"] for c in w["items"]])
    want = expected(w["items"], w["derived"])
    for rounds in (0, 1, 2):
        for exact in (0, 1):
            map_options(di, seed_rounds=rounds, vote_exact_only=exact)
            _same_best(mapper.seed_batch(di, arr, lens, S, THRES), want["best"], (form, rounds, exact))


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("form", list(FORMS))
def test_records_rival_and_phase_votes_on_device_buffers(gpu, forms, map_options, form, rounds):
    w = world()
    di = forms(form)
    items = w["items"]
    arr, lens = _rows([c["read"] for c in items])
    want = expected(items, w["derived"])
    map_options(di, seed_rounds=rounds)
    dm = mapper.DeviceMapper(di, len(lens), int(lens.max()), S, THRES, device=gpu, mapq=True)
    try:
        got = _device(dm, arr, lens, votes=True)
    finally:
        dm.close()
    _check_device(got, want, (form, rounds))
    mapped = want["best"][:, 1] > 0
    assert np.array_equal(got["mapq"]["phase"][mapped], want["d"][mapped]) and mapped.sum() >= len(items) - 6
    # the reads that pass in phase 0, as the first of two rounds marks them and as the single round counts them
    assert got["stats"]["reads_decided_phase0"] == int(want["passes0"].sum()) >= 20
    # what the vote kernels left per (read, phase): every phase under one round, the phases 0 .. d under two
    for i in np.flatnonzero(want["voted"]):
        last = P - 1 if rounds == 1 else int(want["d"][i])
        for p in range(last + 1):
            assert np.array_equal(got["votes"][i, p], want["votes"][i, p]), \
                (form, rounds, items[i]["name"], int(i), p, got["votes"][i, p].tolist(), want["votes"][i, p].tolist())


@pytest.mark.parametrize("form", list(FORMS))
def test_the_host_boundary_gives_the_same_records(gpu, forms, form):
    w = world()
    di = forms(form)
    arr, lens = _rows([c["read"] for c in w["items"]])
    want = expected(w["items"], w["derived"])
    res = mapper.map_batch(di, arr.copy(), lens, S, THRES, mapq=True, options=dict(sub_batches=3))
    _same_best(res["best"], want["best"], (form, "host best"))
    _same_records(res["mapq"], want["rec"], (form, "host mapq"))


@pytest.mark.parametrize("rounds", [1, 2])
def test_the_second_round_searches_the_undecided_reads_only(gpu, forms, map_options, rounds):
    """The counting build of the seed kernel adds up the seed positions it looks up: under two rounds phase 0 of every read and
    the later phases of the reads phase 0 did not decide; under one round every position.  Results as ever."""
    w = world()
    di = forms("default")
    items = w["items"]
    arr, lens = _rows([c["read"] for c in items])
    want = expected(items, w["derived"])
    map_options(di, seed_rounds=rounds)
    dm = mapper.DeviceMapper(di, len(lens), int(lens.max()), S, THRES, device=gpu, mapq=True)
    try:
        dm.set_counting(True)
        got = _device(dm, arr, lens)
    finally:
        dm.close()
    _check_device(got, want, ("counting", rounds))
    later = want["seeds"] - want["seeds0"]
    assert later[~want["passes0"]].sum() > 0 and later[want["passes0"]].sum() > 0
    assert got["stats"]["seeds_evaluated"] == int(want["seeds"].sum() if rounds == 1 else want["seeds0"].sum() + later[~want["passes0"]].sum())


def _policy_batches():
    """late: no read passes in phase 0; early: most do.  Both of at least 64 reads."""
    w = world()
    names = []
    for c in w["items"]:
        if c["name"] not in names:
            names.append(c["name"])
    by = {c["name"]: c for c in w["items"]}
    d, val = (lambda nm: w["derived"][nm]["d"]), (lambda nm: w["derived"][nm]["best"][1])
    first = [nm for nm in names if d(nm) == 0 and val(nm) > 0]
    later = [nm for nm in names if nm not in first]
    # (what passes in phase 0 is what decide_kernel's first round marks: 5 v > 3 num_seeds there)
    for nm in later:
        t = w["derived"][nm]["tops"]
        assert not t or 5 * t[0][0] <= 3 * (len(by[nm]["read"]) // P)
    late = [by[nm] for nm in later * 2]
    early = [by[nm] for nm in first * 3 + later[:4]]
    assert len(late) >= 64 and len(early) >= 64 and 50 * 3 * len(first) >= len(early)
    return late, early


@pytest.mark.parametrize("order,launches", [("LLL", [2, 1, 1]), ("EEE", [2, 2, 2]), ("LLEE", [2, 1, 1, 2])])
def test_adaptive_round_policy(gpu, forms, map_options, order, launches):
    """seed_rounds = 0: the first call on a workspace takes two rounds, and a call after a batch of at least 64 reads of which
    fewer than 2 % passed in phase 0 takes one.  Whatever the policy picks, and whatever an earlier batch left in the
    workspace (its decided mask, its phase bytes, its survivor lists), the results are the brute-force ones."""
    w = world()
    di = forms("default")
    map_options(di, seed_rounds=0)
    late, early = _policy_batches()
    n_max = max(len(late), len(early))
    max_len = max(len(c["read"]) for c in late + early)
    batch = {k: (v,) + _rows([c["read"] for c in v], max_len + 1) for k, v in (("L", late), ("E", early))}     # one row stride, as the workspace has one max_len
    want = {k: expected(v[0], w["derived"]) for k, v in batch.items()}
    dm = mapper.DeviceMapper(di, n_max, max_len, S, THRES, device=gpu, mapq=True)
    try:
        dm.set_timing(True)
        seen = []
        for step, k in enumerate(order):
            _, arr, lens = batch[k]
            got = _device(dm, arr, lens)
            seen.append(dm.timing()["seed_search_kernel"][1])
            _check_device(got, want[k], (order, step, k))
        assert seen == launches, (order, seen)
    finally:
        dm.close()
