"""The premises of tests/test_gpu_hostile_buffers.py, on the references: whatever lies outside the reads -- zeros, the text's
own continuation, random bases of either case, 0xFF, the next read -- the CPU references of every stage return the same
results and leave those bytes alone; and the batch of tests/hostile_buffers.py reaches the edges it was made for."""
import numpy as np
import pytest

import anchored_ref
import hostile_buffers as H

OTHERS = [name for name in H.LAYOUTS if name != "plain"]


@pytest.fixture(scope="module")
def batch():
    return H.batch()


@pytest.fixture(scope="module")
def plain(batch):
    buf = H.build(batch, "plain")
    return H.references(batch, buf.rows[:batch["n"]], batch["lens"]), buf


def _outside(buf, n):
    """mask over the allocation: True for every byte that is not a base of one of the first n reads"""
    m = np.ones(len(buf.alloc), dtype=bool)
    for i in range(n):
        at = buf.shift + i * buf.stride
        m[at:at + int(buf.lens[i])] = False
    return m


@pytest.mark.parametrize("layout", H.LAYOUTS)
def test_layouts_hold_the_reads_and_no_zero_byte(batch, layout):
    n = batch["n"]
    for shift in (0, H.shift_of(layout)):
        buf = H.build(batch, layout, shift)
        stride = H.LAYOUTS[layout][0]
        assert buf.stride == stride and len(buf.alloc) == shift + (n + H.D) * stride and buf.rows.base is not None
        for row in range(n + H.D):
            i = row if row < n else row - H.D
            assert int(buf.lens[row]) == len(batch["reads"][i]) <= H.M <= stride
            assert bytes(buf.rows[row, :buf.lens[row]]) == batch["reads"][i], (layout, row)
        assert (buf.alloc == 0).any() == (layout == "plain")
    assert 1 <= H.shift_of(layout) <= 15
    if layout == "abutting":                               # the byte behind a full-length read is the next read's first base
        full = np.flatnonzero(batch["lens"] == H.M)
        assert all(buf.rows[i].ctypes.data + H.M == buf.rows[i + 1].ctypes.data for i in full)
        assert buf.lens[-1] == H.M and buf.rows[-1].ctypes.data + H.M == buf.alloc.ctypes.data + len(buf.alloc)
    if layout.startswith("text-pad"):                      # ... continues the locus: an exact read would go on matching
        i = next(k for k, (kind, _, _) in enumerate(batch["spec"]) if kind == "edge" and batch["lens"][k] == 129)
        seq, strand = batch["spec"][i][1:]
        src = bytes(batch["seqs"][seq]) if strand == 0 else bytes(anchored_ref.revcomp(batch["seqs"][seq]))
        assert bytes(buf.rows[i, :stride]) in src


@pytest.mark.parametrize("layout", OTHERS)
def test_references_see_the_reads_alone(batch, plain, layout):
    want, _ = plain
    n = batch["n"]
    for shift in (0, H.shift_of(layout)):
        buf = H.build(batch, layout, shift)
        before = buf.alloc.copy()
        got = H.references(batch, buf.rows[:n], batch["lens"], second=shift == 0)
        want_here = want if shift == 0 else {k: v for k, v in want.items() if k not in ("split", "secondary")}
        assert H.same_references(want_here, got) == [], (layout, shift)
        # the oracle's extension turned the reverse-strand reads round in place and left every other byte as it was
        out = _outside(buf, n)
        assert np.array_equal(buf.alloc[out], before[out]), (layout, shift)
        for i in range(n):
            assert np.array_equal(buf.rows[i, :buf.lens[i]], want["oriented"][i, :buf.lens[i]])


def test_the_batch_reaches_its_edges(batch, plain):
    ref, buf = plain
    n, lens, spec = batch["n"], batch["lens"], batch["spec"]
    assert 50 <= n <= 70 and int(lens.max()) == H.M
    cl, classic = ref["clipped"], ref["classic"]
    assert (classic["meta_r"] == 1).all()
    for length in H.LENGTHS:                               # every edge length on both strands, as made and as mapped
        at = [i for i in range(n) if lens[i] == length and spec[i][0] == "edge"]
        assert sorted(spec[i][2] for i in at) == [0, 1] and sorted(int(classic["strand"][i]) for i in at) == [0, 1], length
    full = np.flatnonzero(lens == H.M)
    assert len(full) >= 4 and (np.diff(full) == 1).any() and full[-1] == n - 1
    flags = cl["anchor"][:, 5]
    counts = dict(anchored=int(((flags & anchored_ref.ANCHORED) != 0).sum()),
                  clipped_200=int(((cl["clip_left"] >= 200) | (cl["clip_right"] >= 200)).sum()),
                  segments=len(ref["split"]["table"]), candidates=len(ref["secondary"]["cand"]),
                  mapq0=int((ref["mapq"]["mapq"] == 0).sum()), later_phase=int((ref["phases"] > 1).sum()),
                  reverse=int((classic["strand"] == 1).sum()),
                  seq_end=sum(int(classic["off"][i]) + int(lens[i]) + 64 >= H.mta_of(batch["hi"])[classic["seq_id"][i]][1] for i in range(n)))
    print("hostile batch: %d reads, %s" % (n, counts))
    assert counts["anchored"] >= 10 and counts["clipped_200"] >= 3 and counts["segments"] >= 3 and counts["candidates"] >= 3
    assert counts["mapq0"] >= 3 and counts["later_phase"] >= 5 and counts["seq_end"] >= 1 and 20 <= counts["reverse"] <= n - 20
    # the second passes have work of both kinds: segments with a locus, secondaries that are reported
    assert (ref["split"]["ext"]["meta_r"] != 0).any() and (ref["secondary"]["flags"] & 1).sum() >= 3
    # the flagged reads: their anchor is the exact end, which stops on the read's last base, not on a 32-base word
    flagged = [i for i in range(n) if spec[i][0] == "flagged"]
    assert len(flagged) >= 3 and all(b"N" in batch["reads"][i] for i in flagged)
    assert sum(int(cl["anchor"][i, 1] + cl["anchor"][i, 2]) == int(lens[i]) and lens[i] % 32 != 0 for i in flagged) >= 2
    # op rows end at every residue of the 4- and 16-byte groups the extents are stated in
    assert len({int(k) % 4 for k in classic["n_ops"]}) == 4 and len({int(k) % 16 for k in cl["n_ops"]}) >= 12
