"""Constructed alignments on the CPU: tests/gact_ref.py (the spec in score form, written without the oracle's source)
against the oracle, the bit-slice model and the older single-tile restatement, on tests/gact_cases.py.

What this file establishes is used by tests/test_gpu_gact_constructed.py: the expected values there come from gact_ref,
and by the tests below they are also the oracle's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import constructed
import gact_cases
import gact_ref
import orc
from test_oracle_props import _check_ops, _single_tile_reference

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_SRC = os.path.join(HERE, "models", "gact_bitslice_model.c")
MODEL_LIB = os.path.join(HERE, "models", "libgact_bitslice_model.so")


@pytest.fixture(scope="module")
def model():
    if not os.path.exists(MODEL_LIB) or os.path.getmtime(MODEL_LIB) < os.path.getmtime(MODEL_SRC):
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", MODEL_LIB, MODEL_SRC])
    lib = C.CDLL(MODEL_LIB)
    lib.bsm_gact.restype = C.c_int
    lib.bsm_gact.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                             C.POINTER(C.c_int)]
    ops = np.zeros(1 << 14, dtype=np.uint8)

    def run(q, d, T, O, W, extra):
        n_ops = C.c_int()
        score = lib.bsm_gact(q, len(q), d, len(d), T, O, W, extra, ops.ctypes.data, C.byref(n_ops))
        return score, bytes(ops[:n_ops.value])
    return run


@pytest.fixture(scope="module")
def named():
    """[(case, (score, ops, trace))] of every named case."""
    cs = gact_cases.cases()
    return [(c, gact_ref.align(c["q"], c["d"], c["T"], c["O"], c["W"])) for c in cs]


@pytest.fixture(scope="module")
def exhaustive():
    """{(T, O, W): (pairs, [(score, ops, trace)])} of the square and the ragged exhaustive sets."""
    pairs = gact_cases.exhaustive_square() + gact_cases.exhaustive_ragged()
    return {p: (pairs, gact_ref.align_many(pairs, *p)) for p in gact_cases.EXHAUSTIVE_PARAMS}


def test_the_sets_are_what_the_issue_counts():
    sq, rg = gact_cases.exhaustive_square(), gact_cases.exhaustive_ragged()
    assert len(sq) == 21844 + 4368 and all(len(q) == len(d) for q, d in sq)
    assert len(sq) >= 16384                                     # one batch of them runs under the automatic dispatch
    assert len(rg) == 126 * 126 - sum(4 ** n for n in range(1, 7)) and all(len(q) != len(d) for q, d in rg)
    fam = {}
    for c in gact_cases.cases():
        fam[c["family"]] = fam.get(c["family"], 0) + 1
    assert set(fam) == {"ties", "band", "tile", "exhaustion", "blocks", "random"} and min(fam.values()) >= 25, fam


def test_every_case_reaches_the_edge_it_was_built_for(named):
    missed = [c["name"] for c, (score, ops, trace) in named if c["pred"](score, ops, trace) is not True]
    assert not missed, missed


def test_the_cases_together_see_every_value_and_every_tie(named, exhaustive):
    V, H, ties = set(), set(), set()
    for _, (_, _, trace) in named:
        V |= trace.union("V")
        H |= trace.union("H")
        ties |= trace.union("ties")
    assert V == {-1, 0, 1, 2} and H == {-1, 0, 1, 2}
    assert ties == {"D", "I", "L", "DI", "DL", "IL", "DIL"}     # who held the maximum: alone, in pairs, all three
    # the tie family alone meets the three-way tie and every two-way tie, and at length
    fam = set()
    for c, (_, _, trace) in named:
        if c["family"] == "ties":
            fam |= trace.union("ties")
    assert {"DIL", "DI", "DL", "IL"} <= fam
    # and so does every exhaustive run by itself
    for p, (pairs, res) in exhaustive.items():
        seen, v, h = set(), set(), set()
        for _, _, trace in res:
            seen |= trace.union("ties")
            v |= trace.union("V")
            h |= trace.union("H")
        assert seen == {"D", "I", "L", "DI", "DL", "IL", "DIL"} or p[2] == 2, p
        assert (v == {-1, 0, 1, 2} and h == {-1, 0, 1, 2}) or p[2] == 2, p
    # band edges on both sides, every stop rule, alone and combined
    rules = {t["rule"] for _, (_, _, trace) in named for t in trace}
    assert {frozenset({"keep"}), frozenset({"cap"}), frozenset({"read"}), frozenset({"text"}), frozenset({"text", "keep"}),
            frozenset({"read", "text", "cap"}), frozenset({"read", "text"})} <= rules
    for W in (2, 4, 20, 32, 64, 66, 128, 256):
        lo = min(t["dmin"] for c, (_, _, trace) in named if c["W"] == W for t in trace)
        hi = max(t["dmax"] for c, (_, _, trace) in named if c["W"] == W for t in trace)
        assert (lo, hi) == (-(W // 2), W // 2 - 1), W


def test_reference_invariants(named, exhaustive):
    for c, (score, ops, _) in named:
        _check_ops(c["q"], c["d"], ops, score)
    for p, (pairs, res) in exhaustive.items():
        for (q, d), (score, ops, _) in zip(pairs, res):
            _check_ops(q, d, ops, score)
    assert gact_ref.align(b"ACGT", b"ACGT", 320, 320, 128)[:2] == (-1, b"")
    assert gact_ref.align(b"ACGT", b"ACGT", 320, -1, 128)[0] == -1 and gact_ref.align(b"ACGT", b"ACGT", 320, 120, 127)[0] == -1
    assert gact_ref.align(b"ACGT", b"ACGT", 320, 120, 0)[0] == -1
    assert gact_ref.align(b"", b"ACGT")[:2] == (0, b"") and gact_ref.align(b"ACG", b"")[:2] == (3, b"III")


def test_reference_equals_the_single_tile_restatement(exhaustive):
    """Two restatements that share nothing: where one tile without a band covers the matrix they must agree."""
    pairs = exhaustive[(320, 120, 128)][0]
    step = 7                                                    # the pure-Python one is slow: every 7th pair, all shapes
    got = gact_ref.align_many(pairs[::step], 128, 0, 512)
    for (q, d), (score, ops, trace) in zip(pairs[::step], got):
        assert ops == _single_tile_reference(q, d), (q, d)
        assert len(trace) == 1
    rng = np.random.default_rng(2)
    for n, m in ((100, 100), (100, 63), (37, 100), (64, 65)):
        d = gact_cases.rnd(m, "single", n)
        q = gact_cases._mutate(rng, gact_cases.rnd(n + 20, "single", n)[:n], 0.1, 0.05, 0.05)[:n] if n != m else \
            gact_cases._mutate(rng, d, 0.1, 0.05, 0.05)[:100]
        assert gact_ref.align(q, d, 128, 0, 512)[1] == _single_tile_reference(q, d)


def test_oracle_equals_reference_on_every_named_case(named):
    """The first time the oracle's tiling, band and walk rules meet something they share no code with."""
    for c, (score, ops, trace) in named:
        want = orc.gact(c["q"], c["d"], c["T"], c["O"], c["W"])
        assert (want[0], want[1]) == (score, ops), c["name"]
        assert want[2]["tiles"] == len(trace), c["name"]


@pytest.mark.parametrize("T,O,W", gact_cases.EXHAUSTIVE_PARAMS)
def test_oracle_equals_reference_on_the_exhaustive_sets(exhaustive, T, O, W):
    pairs, res = exhaustive[(T, O, W)]
    for (q, d), (score, ops, trace) in zip(pairs, res):
        want = orc.gact(q, d, T, O, W)
        assert (want[0], want[1]) == (score, ops) and want[2]["tiles"] == len(trace), (q, d)


def test_model_equals_reference(model, named, exhaustive):
    n = 0
    for c, (score, ops, _) in named:
        if c["W"] <= 128:
            for extra in (0, 32, 64):
                assert model(c["q"], c["d"], c["T"], c["O"], c["W"], extra) == (score, ops), (c["name"], extra)
            n += 1
    assert n > 600
    for p, (pairs, res) in exhaustive.items():
        for k, ((q, d), (score, ops, _)) in enumerate(zip(pairs, res)):
            assert model(q, d, *p, (k % 3) * 32) == (score, ops), (p, q, d)


def test_oracle_batch_equals_reference_on_the_packing_cases():
    """orc_extend_batch on keys the test wrote: strand, offset and sequence as planted, fenced windows refused."""
    pb = gact_cases.packing_batch()
    oi = orc.OracleIndex.build(pb["seqs"], o_ratio=32, hlen=4)
    assert bytes(oi.content()) == constructed.index_text(pb["seqs"])
    starts = {(n, r) for n in (200, 321, 1000) for r in range(64)}
    assert len(starts) == 192
    live = [k for k, w in enumerate(pb["windows"]) if w is not None]
    residues = {(len(pb["reads"][k]), pb["pos"][k] % 64, pb["strand"][k]) for k in live if pb["seq_id"][k] == 0}
    for n in (200, 321, 1000):
        assert {(n, r, s) for r in range(64) for s in (0, 1)} <= residues
    reads, lens = gact_cases.read_matrix(pb["reads"])
    best = np.zeros(len(lens), dtype=orc.ENTRY_DT)
    best["key"] = np.array(pb["keys"], dtype=np.uint64)
    got = oi.extend_batch(reads, lens, best, (320, 120, 128))
    want = gact_ref.align_many([(constructed.revcomp(r) if s else r, w) for r, s, w in
                                zip(pb["reads"], pb["strand"], pb["windows"]) if w is not None], 320, 120, 128)
    off = np.concatenate([[0], np.cumsum([2 * len(s) for s in pb["seqs"]])])
    it = iter(want)
    assert len(live) < len(lens)
    for k in range(len(lens)):
        if pb["windows"][k] is None:
            assert (got["meta_r"][k], got["score"][k], got["n_ops"][k], got["meta"]["seq_id"][k]) == (0, -1, 0, -1), k
            assert bytes(reads[k, :lens[k]]) == pb["reads"][k]
            continue
        score, ops, _ = next(it)
        assert got["meta_r"][k] == 1 and got["score"][k] == score and bytes(got["ops"][k, :got["n_ops"][k]]) == ops, k
        m = got["meta"][k]
        assert (m["seq_id"], m["strand"], m["off"], m["loc"]) == \
            (pb["seq_id"][k], pb["strand"][k], pb["pos"][k], off[pb["seq_id"][k]] + pb["pos"][k]), k
        assert bytes(reads[k, :lens[k]]) == (constructed.revcomp(pb["reads"][k]) if pb["strand"][k] else pb["reads"][k])


# ---------------------------------------------------------------------------------------------------------------------
# negative controls: the reference with one rule bent disagrees with the oracle on cases the set names
# ---------------------------------------------------------------------------------------------------------------------
CONTROLS = [
    ("tie order DIAG, DEL, INS", dict(tie_order="DLI"), "ties/AC-CA@64,16,32",
     lambda c: c["family"] == "ties" and c["T"] <= 64),
    ("symmetric band", dict(symmetric_band=True), "band/del16-tile0@320,120,32",
     lambda c: c["family"] == "band" and c["W"] <= 32),
    ("walk of a non-final tile while a <= T-O", dict(keep_inclusive=True), "tile/run-on-the-stop@64,16,128",
     lambda c: c["family"] == "tile" and c["T"] <= 64),
]


@pytest.mark.parametrize("what,bent,witness,subset", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_a_bent_rule_is_seen(named, what, bent, witness, subset):
    seen = []
    for c, _ in named:
        if subset(c):
            want = orc.gact(c["q"], c["d"], c["T"], c["O"], c["W"])
            if gact_ref.align(c["q"], c["d"], c["T"], c["O"], c["W"], **bent)[:2] != (want[0], want[1]):
                seen.append(c["name"])
    print("%s shows on %d cases: %s" % (what, len(seen), ", ".join(seen[:8])))
    assert witness in seen, (what, seen)


def test_a_swapped_tie_order_is_seen_by_the_exhaustive_sets(exhaustive):
    for p, (pairs, res) in exhaustive.items():
        bent = gact_ref.align_many(pairs[:21844:3], *p, tie_order="DLI")
        differ = sum(b[1] != r[1] for b, r in zip(bent, res[:21844:3]))
        assert differ > 100 or p[2] == 2, (p, differ)
