"""The premises of tests/test_gpu_stage_mix.py, on the references alone: the batch of tests/stage_mix.py gives every stage work
at once, and gives it on the same reads -- reads that are a secondary candidate AND the source of segments, on both strands.
The counts are printed ("Composition of the stages", quotes them)."""
import numpy as np
import pytest

import anchored_ref
import hostile_buffers as H
import rival_ref
import split_ref
import stage_mix as S


@pytest.fixture(scope="module")
def made():
    w = S.world()
    before = w["reads"].copy()
    ref = S.references()
    assert np.array_equal(w["reads"], before)              # the references work on a copy
    return w, ref


def _counts(w, ref):
    cl, sp, sec = ref["clipped"], ref["split"], ref["secondary"]
    n = w["n"]
    seg_reads = [t[0] for t in sp["table"]]
    per_read = np.bincount(seg_reads, minlength=n)
    cand = np.zeros(n, dtype=bool)
    cand[sec["cand"]] = True
    both = cand & (per_read > 0)
    seg_aligned = (sp["ext"]["meta_r"] != 0) & ((sp["ext"]["anchor"][:, 5] & anchored_ref.ANCHORED) != 0)
    cols = ref["pileup"].columns()
    in_copy = np.zeros(len(cols), dtype=bool)
    (off0, len0), (off1, len1) = H.mta_of(w["hi"])
    assert (len0, len1) == (S.CUT, S.TEXT - S.CUT)
    in_copy[off0 + S.A0:off0 + S.A0 + S.LN] = in_copy[off1 + S.B0 - S.CUT:off1 + S.B0 - S.CUT + S.LN] = True
    x_all = cols["depth"].astype(np.int64) - cols["n_eq"] - cols["n_del"]
    return dict(reads=n, per_class={c: int((w["cls"] == c).sum()) for c in S.CLASSES},
                mapped={c: int(((cl["meta_r"] != 0) & (cl["score"] != -1) & (w["cls"] == c)).sum()) for c in S.CLASSES},
                candidates=int(cand.sum()), reported=int(((sec["flags"] & rival_ref.SEC_ALIGNED) != 0).sum()),
                duplicates=int(((sec["flags"] & rival_ref.SEC_DUPLICATE) != 0).sum()),
                segments=len(sp["table"]), segments_aligned=int(seg_aligned.sum()),
                both=int(both.sum()), both_reverse=int((both & (cl["strand"] == 1) & (cl["meta_r"] != 0)).sum()),
                both_two_segments=int((both & (per_read == 2)).sum()),
                depth_in_copy=int(cols["depth"][in_copy].max()), x=int(x_all.sum()), d=int(cols["n_del"].sum()), i=int(cols["n_ins"].sum()),
                events=len(ref["diff_events"])), cand, per_read


def test_the_batch_gives_every_stage_work_on_the_same_reads(made):
    w, ref = made
    c, cand, per_read = _counts(w, ref)
    print("stage mix: %s" % c)
    assert 180 <= c["reads"] <= 220 and int(w["lens"].max()) <= S.MAX_LEN and sorted(set(w["lens"][w["cls"] == "e"]))[:3] == [1, 19, 37]
    assert all(c["per_class"][k] > 0 for k in S.CLASSES)
    assert c["both"] >= 8 and c["both_reverse"] >= 3 and c["both_two_segments"] >= 1
    assert c["duplicates"] >= 1 and c["reported"] >= 20 and c["segments_aligned"] >= 20
    assert c["depth_in_copy"] >= 2 and c["x"] > 0 and c["d"] > 0 and c["i"] > 0 and c["events"] > 0
    # every class is what it was made to be once the references have run
    cl = ref["clipped"]
    is_ = lambda k: w["cls"] == k
    mapped = (cl["meta_r"] != 0) & (cl["score"] != -1)
    ins = np.array([p[0][0] == "unique-ins" for p in w["parts"]])
    dup = np.zeros(w["n"], dtype=bool)
    dup[ref["secondary"]["cand"][(ref["secondary"]["flags"] & rival_ref.SEC_DUPLICATE) != 0]] = True
    assert mapped[is_("a")].sum() >= 0.9 * is_("a").sum() and not cand[is_("a") & ~ins].any() and ins.sum() == 4 and dup[ins].any()
    assert cand[is_("b")].sum() >= 0.9 * is_("b").sum()
    assert (cand & (per_read >= 1))[is_("c")].sum() >= 8
    assert (per_read[is_("d")] == 2).sum() >= 3
    # (no locus: best is the zero entry, and the extension's fall-back at text position 0 is not anchored)
    assert not ref["best"]["val"][is_("e")].any() and not (cl["anchor"][is_("e"), 5] & anchored_ref.ANCHORED).any()
    assert not cand[is_("e")].any() and not per_read[is_("e")].any()
    # both sequences, both strands, and chimeras in both part orders and every strand combination
    assert set(cl["seq_id"][mapped]) == {0, 1} and set(cl["strand"][mapped]) == {0, 1}
    combos = {tuple(p) for p, k in zip(w["parts"], w["cls"]) if k == "c"}
    assert combos == {((a, s), (b, t)) for a, b in (("copy", "unique"), ("unique", "copy")) for s in (0, 1) for t in (0, 1)}


def test_the_segment_table_and_the_candidates_are_the_rules(made):
    w, ref = made
    cl = ref["clipped"]
    assert ref["split"]["table"] == split_ref.plan(w["lens"], cl["clip_left"], cl["clip_right"])
    assert np.array_equal(ref["secondary"]["cand"], rival_ref.plan(ref["mapq"]))
    off = ref["diff_off"]
    assert len(off) == w["n"] + 1 and off[-1] == len(ref["diff_events"])
    assert [int(b - a) for a, b in zip(off[:-1], off[1:])] == [s["n_x"] + s["n_del"] for s in ref["summary"]]


def test_the_second_batch_is_a_batch_of_its_own(made):
    w, ref = made
    rows, lens, pick = S.every_third()
    assert len(pick) == (w["n"] + 2) // 3 and np.array_equal(rows, w["reads"][pick])
    cls = set(w["cls"][pick])
    assert cls == set(S.CLASSES)
