"""The batches of tests/seed_lines_cases.py are what they say, by brute force on the text alone (constructed.census: sorted
S-mer codes of the index text; nothing of the device, the index builder or the oracle)."""
import numpy as np
import pytest

import constructed as K
import seed_lines_cases as L

S = L.S


@pytest.fixture(scope="module")
def world():
    seq = L.forward()
    content = K.index_text([seq])
    return seq, content, K.census(content, S)


def test_text(world):
    seq, content, cen = world
    assert len(seq) == L.FWD and len(content) == 2 * L.FWD + 1
    assert int(cen.counts.max()) < L.THRES
    assert len(L.CORE) == S - 3 and set(L.CORE) <= set(b"ACGT")
    assert [bytes(seq[at + 3:at + 3 + len(L.CORE)]) for at in L.COPY_AT] == [L.CORE] * 4


def test_the_core_names_line_zero():
    # the restated hash on the core's code, for the table sizes the GPU test uses and the ends of the range
    code = sum(int(K._CODE[b]) << (2 * i) for i, b in enumerate(L.CORE))
    assert code == L.CORE_CODE
    for bits in (3, 13, 16, 17, 21, 25, 26, 31):
        assert L.line_of(code, bits) == 0, bits
    assert L.line_of(code ^ 1, 17) != 0                      # (the restatement is no constant)


def test_crowded_line(world):
    seq, content, cen = world
    pairs = L.core_pairs(content)
    assert len(pairs) >= 9, len(pairs)                       # eight slots and at least one entry beside the line
    assert len(pairs) == 16 and {r for r, _ in pairs} == {0, 1, 2, 3}
    assert all(sum(1 for r, _ in pairs if r == q) == 4 for q in range(4))
    # the reads: clean windows, every seed in the text; every pair is some read's seed at a position of its role
    reads = L.batch("crowd", seq)
    assert len(reads) == 16
    seen = set()
    for i, r in enumerate(reads):
        c = L.seed_counts(r, cen)
        assert len(c) == L.CROWD_LEN - S and (c > 0).all() and (c < L.THRES).all()
        at = r.find(L.CORE)
        assert at >= 3 and at % 4 == (3 + L.CROWD_LEAD + i % 4) % 4           # the copy at all four positions mod 4
        for p in range(at - 3, at + 1):
            if (p & 3) == p - (at - 3):                      # the seed at p has the core as ITS core: role p & 3
                seen.add((p & 3, r[p:p + S]))
    assert seen == pairs


def test_random_reads_hold_no_smer_of_the_text(world):
    seq, _, cen = world
    reads = L.batch("random", seq)
    assert {(len(r) - S) % 4 for r in reads} == {0, 1, 2, 3}
    for r in reads:
        assert not L.seed_counts(r, cen).any()


def test_ragged_lengths(world):
    seq, _, cen = world
    reads = L.batch("ragged", seq)
    assert [len(r) for r in reads] == list(L.RAGGED)
    lim = [len(r) - S for r in reads]
    assert {n % 4 for n in lim} >= {1, 2, 3}
    assert any(n % 64 == 1 and n > 64 for n in lim) and any(n % 256 == 1 and n > 256 for n in lim)
    assert any(n % 4 == 2 and n > 64 for n in lim) and any(n % 4 == 3 and n > 64 for n in lim)
    for r in reads:
        assert (L.seed_counts(r, cen) > 0).all()
