"""The batches of tests/seed_filter_cases.py are what they say, by brute force on the text alone (constructed.census: sorted
S-mer codes of the index text; nothing of the device, the index builder or the oracle)."""
import numpy as np
import pytest

import constructed as K
import seed_filter_cases as F

S = F.S


@pytest.fixture(scope="module")
def world():
    seq = F.forward()
    content = K.index_text([seq])
    return seq, content, K.census(content, S)


def test_text(world):
    seq, content, cen = world
    assert len(seq) == F.FWD and len(content) == 2 * F.FWD + 1
    assert cen.count(seq[F.REP_AT[0] + 10:][:S]) == 3           # the planted string: 1 < count < thres
    assert int(cen.counts.max()) < F.THRES


def test_tile_holds_every_smer_of_the_text(world):
    seq, content, cen = world
    reads = F.batch("tile", seq)
    seen = np.zeros(len(content) - 1 - S, dtype=bool)           # every S-mer but the one on the last base
    for i, r in enumerate(reads):
        c = F.seed_counts(r, cen)
        a = i * F.TILE
        assert bytes(content[a:a + len(r)]) == r
        assert np.array_equal(c, cen.at[a:a + len(c)]) and (c > 0).all() and (c < F.THRES).all()       # every seed survives
        seen[a:a + len(c)] = True
    assert seen.all()
    assert K.revcomp(bytes(content[:-1])) == bytes(content[:-1])          # both strands: the text is its own reverse complement


def test_random_reads_hold_no_smer_of_the_text(world):
    seq, _, cen = world
    reads = F.batch("random", seq)
    assert max(len(r) for r in reads) - S > 4096 and any((len(r) - S) % 256 == 1 for r in reads)
    for r in reads:
        assert not F.seed_counts(r, cen).any()


def test_stretch_reads(world):
    seq, _, cen = world
    reads = F.batch("stretch", seq)
    n = F.STRETCH - S + 1
    for r, at in zip(reads, F.STRETCH_AT):
        c = F.seed_counts(r, cen)
        assert np.flatnonzero(c).tolist() == list(range(at, at + n)), at
    assert sorted(at % 4 for at in F.STRETCH_AT[:4]) == [0, 1, 2, 3]
    assert all(at // 64 == (at + n - 1) // 64 for at in F.STRETCH_AT[:4])          # one wavefront, one or two quads
    assert [at // d != (at + n - 1) // d for at, d in zip(F.STRETCH_AT[4:], (64, 256, 2048))] == [True] * 3
    for r, at in zip(reads[len(F.STRETCH_AT):], F.HOLE_AT):
        c = F.seed_counts(r, cen)
        assert np.flatnonzero(c == 0).tolist() == list(range(at - S + 1, at + 1)), at
        # the wavefront(s) of the hole keep quads with seeds
        assert c[(at - S + 1) // 64 * 64:(at // 64 + 1) * 64].any()


def test_lengths(world):
    seq, _, cen = world
    reads = F.batch("lengths", seq)
    assert [len(r) for r in reads] == list(F.LENGTHS)
    its = [(max(len(r) - S, 0) + 255) // 256 for r in reads]
    assert 0 in its and {i % 2 for i in its if i} == {0, 1} and max(its) > 2048 // 256      # a second workgroup too
    for r in reads:
        assert (F.seed_counts(r, cen) == 1).all()


def test_ont_reads(world):
    seq, _, cen = world
    reads = F.batch("ont", seq)
    assert len(reads) == 64
    frac = np.mean(np.concatenate([F.seed_counts(r, cen) > 0 for r in reads]))
    assert 0.05 < frac < 0.5, frac                              # most seeds of a noisy read are absent from the text
