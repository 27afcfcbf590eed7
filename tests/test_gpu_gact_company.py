"""The extension kernels on the constructed alignments of tests/gact_cases.py IN COMPANY (tests/gact_company.py): a case
shares its wavefront with lanes that hold tiles of their own.  Every table goes through lrm_debug_gact_jobs -- the
product's plan and launch on a job table with target lengths -- and every job of it, case and companion, must give
tests/gact_ref.py's (score, ops) exactly.  For the bit-sliced kernel one table is one wavefront (bs_waves = 1, job k in
lane k) and the counting build's counters must equal the control-flow model's (tests/bs_flow.py): that the intended path
ran is certified, not assumed.  tests/test_gact_company_cpu.py shows that the companies force what they are for."""
import numpy as np
import pytest

import company_ref
import gact_cases
import gact_company
from longreadmapper_amd import capi, mapper

pytestmark = pytest.mark.gpu

BYTE, BYTE3, BITSLICED = 1, 3, 4                     # lrm_map_options.gact_impl
FILL = 0xAB                                          # what the op rows, n_ops and score hold before the launch
FAMILIES = ("ties", "band", "tile", "exhaustion", "blocks", "random")


def _run(co, impl, counting=False):
    arr, lens = gact_cases.read_matrix([q for q, _ in co["pairs"]])
    meta_r = [0 if k in co["fenced"] else 1 for k in range(len(lens))]
    return mapper.debug_gact_jobs(arr, lens, co["text"], co["toffs"], [len(d) for _, d in co["pairs"]], co["gact"], impl,
                                  bs_waves=1, counting=counting, meta_r=meta_r, store_stride=co["store_stride"], fill=FILL)


def _check_results(co, got, want):
    untouched = np.int32(np.uint32(FILL * 0x01010101).astype(np.int32))
    for k, (score, ops) in enumerate(want):
        if k in co["fenced"]:
            assert (int(got["score"][k]), int(got["n_ops"][k])) == (-1, 0), (co["name"], k)
            assert (got["ops"][k] == FILL).all(), (co["name"], k)
            continue
        assert got["n_ops"][k] != untouched and got["score"][k] != untouched, (co["name"], k)
        assert (int(got["score"][k]), int(got["n_ops"][k])) == (score, len(ops)), (co["name"], k, co["cases"].get(k))
        assert bytes(got["ops"][k, :len(ops)]) == ops, (co["name"], k, co["cases"].get(k))


def _check_counters(co, got, tiles, cnt):
    want = {k: cnt[k] for k in capi.BS_COUNTERS}
    # flagged reads run on the byte kernel behind the bit-sliced one, which counts their tiles too
    want["gact_tiles"] = cnt["gact_tiles"] + sum(len(tiles[k]) for k in co["flagged"] - co["fenced"])
    assert got["counters"] == want, co["name"]
    assert want["bs_blocks_full"] + want["bs_blocks_windowed"] + want["bs_blocks_skipped"] == cnt["blocks_per_tile_sum"]


def _same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("ops", "n_ops", "score"))


def _bitsliced(companies):
    """Each table on one wavefront of the counting build: answers and counters; the first again with counting off."""
    assert companies
    for at, co in enumerate(companies):
        want, tiles, cnt, _ = company_ref.model(co)
        got = _run(co, BITSLICED, counting=True)
        _check_results(co, got, want)
        _check_counters(co, got, tiles, cnt)
        if at == 0:
            off = _run(co, BITSLICED)
            assert _same_bytes(got, off) and not any(off["counters"][k] for k in capi.BS_COUNTERS)
            assert off["counters"]["gact_tiles"] == got["counters"]["gact_tiles"] > 0


def _of_family(companies, family):
    return [co for co in companies if all(name.split("/")[0] == family for name in co["cases"].values())]


@pytest.mark.parametrize("family", FAMILIES)
def test_whole_company(gpu, family):
    """The case among 63 lanes of whole tiles: the wavefront's S0, masks and block widths are a whole tile's."""
    _bitsliced([co for gact in sorted(company_ref.groups(128)) for co in _of_family(company_ref.companies("whole", gact), family)])


@pytest.mark.parametrize("family", FAMILIES)
def test_staircase_company(gpu, family):
    """W = 128: every pair of the case's wave-tiles masked, every block in full width."""
    _bitsliced([co for gact in sorted(company_ref.groups(128)) if gact[2] == 128
                for co in _of_family(company_ref.companies("staircase", gact)[0], family)])


def test_ragged_company_bitsliced(gpu):
    """Unequal tq and tt side by side in one wavefront, flagged and fenced jobs among them, both store paths."""
    _bitsliced([co for gact in sorted(company_ref.groups(128)) for co in company_ref.companies("ragged", gact)])


@pytest.mark.parametrize("impl", [0, BYTE, BYTE3])
def test_ragged_company_byte_kernels(gpu, impl):
    """The same tables, and those of the bands above 128 diagonals, on gact_wide_kernel (many jobs with m != n, rows
    addressed by job) and on what gact_impl = 0 and 3 choose for a small table."""
    n = 0
    for gact in sorted(company_ref.groups(None)):
        for co in company_ref.companies("ragged", gact):
            want = [r[:2] for r in company_ref.align(co["pairs"], gact)]
            _check_results(co, _run(co, impl), want)
            n += 1
    assert n >= 50


@pytest.mark.parametrize("partner", gact_company.PARTNERS)
def test_pair_company(gpu, partner):
    """gact3_kernel: every case in the low and in the high half of its wavefront's registers, beside a whole-tile read, a
    one-base pair, a copy of itself, another case."""
    n = 0
    for gact in sorted(company_ref.groups(128)):
        if not gact_company.packed_plan(gact):
            continue
        (co,) = [c for c in company_ref.companies("pairs", gact) if c["kind"] == "pair-" + partner]
        want = [r[:2] for r in company_ref.align(co["pairs"], gact)]
        got = _run(co, BYTE3)
        _check_results(co, got, want)
        assert got["counters"]["gact_tiles"] == sum(len(r[2]) for r in company_ref.align(co["pairs"], gact))
        n += len(co["cases"])
    assert n == 2 * sum(len(g) for gact, g in company_ref.groups(128).items() if gact_company.packed_plan(gact))
