"""The workgroup forms of the vote kernels (vote_kernels.hip: vote_fast_block_kernel; vote_item_block of the exact kernel in one,
two and three or more passes, with and without the key scratch, and with its table in global memory) on the constructed items
of tests/vote_block_cases.py.

What the vote kernels leave per (read, phase) -- key, count and bucket of BOTH entries (lrm_debug_vote_results) -- is compared in
phase 0 with the brute-force reference (constructed.py: census + vote_top2), in every later phase with the oracle's trace, and
best[] of the same call with the oracle's; through the fast kernels and through the exact kernel alone, with the default limits
and with the case's debug limits (lrm_debug_set_vote_limits).  The items the fast kernels hand to the exact kernel
(vote_redo_items) are asserted exactly, (read, phase) item by item, from counting or the harness's sketch counters
(vote_block_cases.settles, _derive).

Before anything runs on the device the case's predicate runs on the CPU (test_vote_block_cases_cpu.py runs all of them without
a device)."""
import numpy as np
import pytest

import vote_block_cases as V
from longreadmapper_amd import index
import test_gpu_vote_rank as vote_rank

pytestmark = pytest.mark.gpu

RUNS = [("fast", 0, False), ("exact", 1, False), ("fast-limits", 0, True), ("exact-limits", 1, True)]


def _seed(di, gpu, reads, exact):
    """-> the six words of every (read, phase), best[], vote_redo_items"""
    assert (V.S, V.THRES) == (vote_rank.S, vote_rank.THRES)
    return vote_rank._vote(di, gpu, reads, exact, with_best=True)


def _all_runs(di, gpu, reads, limits):
    """The four runs of a batch: {run: (votes, best, redo)}; the debug limits go back to (0, 0) whatever happens."""
    out = {}
    try:
        for what, exact, limited in RUNS:
            di.debug_set_vote_limits(*(limits if limited else (0, 0)))
            out[what] = _seed(di, gpu, reads, exact)
    finally:
        di.debug_set_vote_limits(0, 0)
        di.set_map_options()
    return out


def _check_rows(got, best, wants, what):
    """wants[i]: (phase -> six words, best) of row i (vote_block_cases.expected)."""
    for i, (recs, want_best) in enumerate(wants):
        for ph, want in recs.items():
            assert np.array_equal(got[i, ph], want), (what, "row", i, "phase", ph, got[i, ph].tolist(), want.tolist())
        assert (int(best["key"][i]), int(best["val"][i]), int(best["bucket"][i])) == tuple(want_best), (what, "row", i, "best", best[i], want_best)


@pytest.mark.parametrize("gname,cname", V.CASES, ids=[c for _, c in V.CASES])
def test_vote_block(gpu, gname, cname):
    c = V.resolve(gname, cname)
    c["predicate"]()
    wants = [V.expected(r) for r in c["reads"]]
    di = index.DeviceIndex.upload(V.world(gname)["hi"], gpu)
    try:
        runs = _all_runs(di, gpu, [r["seq"] for r in c["reads"]], c["limits"])
    finally:
        di.close()
    for what, (got, best, redo) in runs.items():
        _check_rows(got, best, wants, (cname, what))
        if what.startswith("exact"):
            assert redo == 0, (cname, what, redo)
        else:                                   # every (read, phase) item the rule hands on, and no other (vote_block_cases._derive)
            assert c["redo"] is not None and redo == c["redo"], (cname, what, redo, [(r["settles"], r["redo_items"]) for r in c["reads"]])


# ---- in company ----------------------------------------------------------------------------------------------------------
def _company(gname, rows=33):
    """33 rows on one text: case reads, 700-base substrings of the text (items of the wavefront tier in every phase: asserted
    from the oracle's trace) and empty reads in turn, so that one 16-item group of vote_kernel holds wavefront-tier and workgroup-tier items, which share the
    VoteLds union.  -> (reads, wants)"""
    w = V.world(gname)
    names = sorted(w["text"].reads)
    picked = [names[i * len(names) // 11] for i in range(11)]
    reads, wants = [], []
    for k, nm in enumerate(picked):
        r = w["read"](nm)
        at = w["text"].beyond + 100 * k
        sub = bytes(w["pl"].seq[at:at + 700])
        tr = w["oi"].seed_read(sub, V.S, V.THRES, trace=True)
        for p in range(V.P):
            assert sum(rr for j, rr, _, _ in tr["seeds"] if j % V.P == p and 0 < rr < V.THRES) <= V.T1_LIMIT, (gname, at, p)
        empty = w["oi"].seed_read(b"", V.S, V.THRES, trace=True)
        reads += [r["seq"], sub, b""]
        wants += [V.expected(r), ({rec["iter"]: V.words([rec["top1"], rec["top2"]]) for rec in tr["phase_recs"]}, tr["best"]),
                  ({}, empty["best"])]
    assert len(reads) == rows
    return reads, wants


@pytest.mark.parametrize("gname", [g for g in V.GROUPS if g not in ("no-unique",)])
def test_vote_block_in_company(gpu, gname):
    """Every row of a mixed batch equals its record alone.  Which workgroup takes which item, and what shared memory held
    before, depends on scheduling: company pins answers, not paths."""
    reads, wants = _company(gname)
    di = index.DeviceIndex.upload(V.world(gname)["hi"], gpu)
    try:
        runs = _all_runs(di, gpu, reads, V.LIMITS)
    finally:
        di.close()
    for what, (got, best, redo) in runs.items():
        _check_rows(got, best, wants, (gname, what))
        assert not what.startswith("exact") or redo == 0


def test_more_items_than_workgroups(gpu):
    """2000 rows, list-513 and list-512 in turn: more items than the 768 workgroups of the fast workgroup form, so workgroups
    take several items one after the other (s_list_n, the table, the sketch and s_rk are reused).  Every row equals its record
    alone, and the 513 rows -- no other -- go to the exact kernel.  (Which workgroup takes which item depends on scheduling:
    this pins answers, not paths.)"""
    c = V.resolve("list", "list-at-512-and-513")
    c["predicate"]()
    full, less = c["reads"]
    assert full["settles"][0] is False and less["settles"][0] is True and c["redo"] == 1
    n = 2000
    reads = [full["seq"], less["seq"]] * (n // 2)
    wants = [V.expected(full), V.expected(less)]
    di = index.DeviceIndex.upload(V.world("list")["hi"], gpu)
    try:
        fast = _seed(di, gpu, reads, 0)
        exact = _seed(di, gpu, reads, 1)
    finally:
        di.set_map_options()
        di.close()
    for what, (got, best, redo) in (("fast", fast), ("exact", exact)):
        for k, (recs, want_best) in enumerate(wants):
            for ph, want in recs.items():
                bad = np.nonzero((got[k::2, ph] != want).any(axis=1))[0]
                assert bad.size == 0, (what, "rows", (2 * bad[:8] + k).tolist(), "phase", ph, got[2 * bad[0] + k, ph].tolist(), want.tolist())
            b = best[k::2]
            assert (b["key"] == want_best[0]).all() and (b["val"] == want_best[1]).all() and (b["bucket"] == want_best[2]).all(), (what, k)
        assert redo == (n // 2 if what == "fast" else 0), (what, redo)
