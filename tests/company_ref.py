"""What the company tests expect, computed once per test run: tests/gact_ref.py's alignment of every job of a company
(cases and companions alike), its tiles for the control-flow model, and the companies of tests/gact_company.py built
from the lives those alignments give.  Shared by test_gact_company_cpu.py and test_gpu_gact_company.py; nothing is
changed after it is computed."""
import functools

import bs_flow
import gact_company
import gact_ref

_REF = {}                                     # (q, d, gact) -> (score, ops, tiles)


def align(pairs, gact):
    """[(score, ops, tiles)] of the pairs; the new ones of equal tile shape are filled together."""
    new = list({p for p in pairs if p + (gact,) not in _REF})
    for p, (score, ops, trace) in zip(new, gact_ref.align_many(new, *gact)):
        _REF[p + (gact,)] = (score, ops, bs_flow.tile_rows(ops, trace))
    return [_REF[p + (gact,)] for p in pairs]


@functools.lru_cache(maxsize=None)
def groups(max_w=128):
    return gact_company.groups(max_w)


@functools.lru_cache(maxsize=None)
def lives(gact):
    """{case name: tiles of its reference alignment} of the cases of one (T, O, W)."""
    cases = groups(None)[gact]
    return {c["name"]: len(r[2]) for c, r in zip(cases, align([(c["q"], c["d"]) for c in cases], gact))}


@functools.lru_cache(maxsize=None)
def companies(kind, gact):
    """The companies of one kind for the cases of one (T, O, W); staircase: (companies, names left out)."""
    cases = groups(None)[gact]
    if kind == "ragged":
        return gact_company.ragged(cases, gact)
    return getattr(gact_company, kind)(cases, gact, lives(gact))


_MODEL = {}                                   # company name -> model()


def model(company):
    """-> (expected [(score, ops)], tiles, counters of the model, its record) of a company on one wavefront."""
    if company["name"] not in _MODEL:
        ref = align(company["pairs"], company["gact"])
        tiles = [r[2] for r in ref]
        record = []
        cnt = bs_flow._model(tiles, company["fenced"] | company["flagged"], 1, company["gact"], record)
        _MODEL[company["name"]] = ([r[:2] for r in ref], tiles, cnt, record)
    return _MODEL[company["name"]]
