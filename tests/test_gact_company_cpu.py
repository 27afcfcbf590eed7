"""The companies of tests/gact_company.py do what they are for (no GPU): every company's predicate holds on the control-
flow model (tests/bs_flow.py) fed with the reference's traces (tests/gact_ref.py), every case is in the companies the
GPU tests count on, and the sets are a function of nothing but the case set."""
import hashlib

import pytest

import bs_flow
import company_ref
import gact_cases
import gact_company

T, O, W = 320, 120, 128
BS_GROUPS = sorted(company_ref.groups(128))


def test_the_case_set_is_the_one_the_companies_were_laid_out_for():
    groups = company_ref.groups(128)
    cases = [c for g in groups.values() for c in g]
    assert len(cases) == 640 and sum(len(c["q"]) != len(c["d"]) for c in cases) == 259
    assert sum(len(g) for gact, g in groups.items() if gact[2] == 128) == 423
    assert len(gact_cases.cases()) == 745


@pytest.mark.parametrize("tile,alone,beside", [((1, 1), (1, None, 1, None), (305, None, 13, None)),
                                               ((7, 200), (33, 64, 4, 3), (209, 96, 8, 5))])
def test_company_changes_the_path_not_the_walk(tile, alone, beside):
    """The same tile alone in its wavefront and beside one whole-tile lane: pass 1 starts at the wavefront's largest
    tq + tt, so beside a whole tile the (1, 1) tile's sweep starts 608 anti-diagonals beyond its own far corner."""
    last = 2 * (T - O) - 1                   # a walk that runs to the last anti-diagonal: no block is left out
    for lanes, (masked, plain, full, windowed) in (([tile + (last,)], alone), ([tile + (last,), (T, T, last)], beside)):
        rec = {}
        cnt = dict.fromkeys(bs_flow.capi.BS_COUNTERS + ("gact_tiles", "blocks_per_tile_sum"), 0)
        bs_flow._tile(cnt, lanes, (T, O, W), rec)
        if plain is None:                     # the (1, 1) tile: pairs and blocks in all
            assert (rec["masked"] + rec["plain"], len(rec["blocks"])) == (masked, full)
        else:
            assert (rec["masked"], rec["plain"], rec["blocks"].count("F"), rec["blocks"].count("W")) == (masked, plain, full, windowed)
    assert rec["S0"] == 2 * T


def _check(company):
    want, tiles, cnt, record = company_ref.model(company)
    assert company["pred"](tiles, record), company["name"]
    assert len(company["pairs"]) <= gact_company.LANES and cnt["bs_wave_tiles"] == len(record)
    for job, name in company["cases"].items():
        if job not in company["flagged"]:
            assert company["pairs"][job][0] == CASES[name]["q"]
        assert company["pairs"][job][1] == CASES[name]["d"]


CASES = {c["name"]: c for c in gact_cases.cases()}


@pytest.mark.parametrize("gact", BS_GROUPS, ids=lambda g: "%d-%d-%d" % g)
def test_whole_companies(gact):
    cases = company_ref.groups(128)[gact]
    companies = company_ref.companies("whole", gact)
    assert [list(c["cases"].values()) for c in companies] == [[c["name"]] for c in cases]
    for c in companies:
        _check(c)


@pytest.mark.parametrize("gact", [g for g in BS_GROUPS if g[2] == 128], ids=lambda g: "%d-%d-%d" % g)
def test_staircase_companies(gact):
    """Every tile of every case of at most 8 tiles is a wave-tile without a plain pair or a windowed block."""
    cases = company_ref.groups(128)[gact]
    lives = company_ref.lives(gact)
    companies, left = company_ref.companies("staircase", gact)
    assert all(lives[name] > gact_company.STAIR_MAX_TILES for name in left)
    covered = {}
    for c in companies:
        _check(c)
        (name,) = c["cases"].values()
        covered.setdefault(name, set()).update(c["covers"])
    assert set(covered) | set(left) == {c["name"] for c in cases} and not set(covered) & set(left)
    assert all(covered[name] == set(range(lives[name])) for name in covered)


def test_staircase_leaves_out_at_most_26_cases():
    left = [name for gact in BS_GROUPS if gact[2] == 128 for name in company_ref.companies("staircase", gact)[1]]
    assert len(left) <= 26, left
    print("left out of the staircase kind:", len(left))


@pytest.mark.parametrize("gact", sorted(company_ref.groups(None)), ids=lambda g: "%d-%d-%d" % g)
def test_ragged_companies(gact):
    """Every case of the (T, O, W) is in both shuffles, and in one of them neither flagged nor fenced; both store paths
    and every residue mod 64 occur (where the group has the jobs for it)."""
    cases = company_ref.groups(None)[gact]
    companies = company_ref.companies("ragged", gact)
    seen, clear = [], set()
    for c in companies:
        if gact[2] <= 128:
            _check(c)
        seen += list(c["cases"].values())
        clear |= {name for job, name in c["cases"].items() if job not in c["flagged"] | c["fenced"]}
        for job in c["flagged"]:
            assert any(x not in b"ACGT" for x in c["pairs"][job][0])
    assert sorted(seen) == sorted(2 * [c["name"] for c in cases])
    assert clear == {c["name"] for c in cases}
    assert {c["store_stride"] % 16 for c in companies} == {0, 4}
    if len(cases) >= 64:
        assert {o % 64 for c in companies for o in c["toffs"]} == set(range(64))
        assert any(c["flagged"] for c in companies) and any(c["fenced"] for c in companies)


@pytest.mark.parametrize("gact", [g for g in BS_GROUPS if gact_company.packed_plan(g)], ids=lambda g: "%d-%d-%d" % g)
def test_pair_companies(gact):
    """Every case in the low and in the high half of a wavefront of gact3_kernel, beside each kind of partner."""
    cases = company_ref.groups(128)[gact]
    companies = company_ref.companies("pairs", gact)
    assert [c["kind"] for c in companies] == ["pair-" + k for k in gact_company.PARTNERS]
    for c in companies:
        tiles = [r[2] for r in company_ref.align(c["pairs"], gact)]
        assert c["pred"](tiles, None), c["name"]
        halves = {}
        for job, name in c["cases"].items():
            assert c["pairs"][job] == (CASES[name]["q"], CASES[name]["d"]) and c["partner_of"][job] == job ^ 1
            halves.setdefault(name, set()).add(job & 1)
        assert halves == {case["name"]: {0, 1} for case in cases}


def _digest(companies):
    h = hashlib.sha256()
    for c in companies:
        h.update(repr((c["name"], c["gact"], c["pairs"], sorted(c["cases"].items()), c["text"], c["toffs"], c["store_stride"],
                       sorted(c["flagged"]), sorted(c["fenced"]))).encode())
    return h.hexdigest()


def test_company_sets_are_deterministic():
    """Built again from scratch (no cache), every company is the same bytes: the two kinds with a table per group for
    every group, the two with a table per case for the groups of the small tiles."""
    for gact in BS_GROUPS:
        cases, lives = gact_company.groups(128)[gact], company_ref.lives(gact)
        assert _digest(gact_company.ragged(cases, gact)) == _digest(company_ref.companies("ragged", gact))
        if gact_company.packed_plan(gact):
            assert _digest(gact_company.pairs(cases, gact, lives)) == _digest(company_ref.companies("pairs", gact))
        if gact[0] <= 100:
            assert _digest(gact_company.whole(cases, gact, lives)) == _digest(company_ref.companies("whole", gact))
            if gact[2] == 128:
                assert _digest(gact_company.staircase(cases, gact, lives)[0]) == _digest(company_ref.companies("staircase", gact)[0])


def test_company_counts():
    """The sets the GPU tests run."""
    count = {kind: sum(len(company_ref.companies(kind, g)) for g in BS_GROUPS) for kind in ("whole", "ragged")}
    count["staircase"] = sum(len(company_ref.companies("staircase", g)[0]) for g in BS_GROUPS if g[2] == 128)
    count["pairs"] = sum(len(company_ref.companies("pairs", g)) for g in BS_GROUPS if gact_company.packed_plan(g))
    count["ragged, W > 128"] = sum(len(company_ref.companies("ragged", g)) for g in company_ref.groups(None) if g[2] > 128)
    print(count)
    assert count["whole"] == 640 and count["staircase"] >= 397 and count["ragged"] >= 2 * len(BS_GROUPS)
    assert count["pairs"] == 4 * sum(gact_company.packed_plan(g) for g in BS_GROUPS)
