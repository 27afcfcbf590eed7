"""tests/anchor_job_cases.py against tests/anchored_ref.py alone: every read anchors at exactly the planned place, and the
places cover what the list promises.  This is what keeps tests/test_gpu_anchor_job_cases.py from passing vacuously."""
import numpy as np

import anchor_job_cases as ajc
import anchored_ref


def test_every_case_anchors_where_it_was_planted():
    s = ajc.seq()
    cs = ajc.cases()
    assert len(s) == ajc.SEQ_LEN and 70 <= len(cs) <= 100
    for c in cs:
        L = c["start"]                                                 # the sequence at text offset 0, the locus at the window
        assert len(c["fwd"]) == c["n"] <= 8300
        # shortest legal anchor_min_len: nothing without the run, the run with it -- and with the default too
        assert anchored_ref.find_anchor(c["plain"], s, L, 0, len(s), 12) is None, c["name"]
        assert anchored_ref.find_anchor(c["fwd"], s, L, 0, len(s), 12) == (ajc.RUN, 0, c["j"]), c["name"]
        assert anchored_ref.find_anchor(c["fwd"], s, L, 0, len(s)) == (ajc.RUN, 0, c["j"]), c["name"]


def test_the_list_covers_the_residues_and_the_edges():
    cs = ajc.cases()
    js = {c["j"] for c in cs}
    rs = {c["n"] - c["j"] for c in cs}
    edges = {4095, 4096, 4097, 4111, 4112}
    assert {j % 16 for j in js} == set(range(16)) and {r % 16 for r in rs} == set(range(16))
    assert set(range(1, 18)) <= js and edges <= js and 0 in js
    assert set(range(ajc.RUN, ajc.RUN + 18)) <= rs and edges <= rs and min(rs) == ajc.RUN
    assert any(c["j"] in edges and c["n"] - c["j"] in edges for c in cs)          # both rows past one chunk
    # either strand meets every residue of either job, and every chunk edge
    for strand in (0, 1):
        sub = [c for c in cs if c["strand"] == strand]
        assert len(sub) >= len(cs) // 2
        assert {c["j"] % 16 for c in sub} == set(range(16)) and {(c["n"] - c["j"]) % 16 for c in sub} == set(range(16))
        assert edges <= {c["j"] for c in sub} | {c["n"] - c["j"] for c in sub}


def test_batches_at_the_three_strides():
    s = ajc.seq()
    cs = ajc.cases()
    max_len = max(c["n"] for c in cs)
    st = ajc.strides(max_len)
    assert st[0] == max_len + 1 and st[1] == max_len + 2 and st[2] % 16 == 0 and st[2] > max_len
    S, ls = 0, len(s)
    text = np.concatenate([s, anchored_ref.revcomp(s)])
    reads, lens, keys = ajc.batch(cs, S, ls, st[0])
    for i, c in enumerate(cs):
        n = c["n"]
        assert lens[i] == n and not reads[i, n:].any()
        # the read as sequenced lies at its key in the text but for its substitutions
        assert (reads[i, :n] == text[int(keys[i]):int(keys[i]) + n]).mean() > 0.9
        assert c["strand"] == (keys[i] >= S + ls)
