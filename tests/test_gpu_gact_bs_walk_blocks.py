"""gact_bs_kernel with the walk's `on` by recurrence and the full-width blocks of a tile decided once, ahead of the blocks
(a bit per block from the lanes' tq and tt): one wavefront of 64 reads of 330 .. 2000 bases, the smallest grid
(bs_waves = 1), so that lanes finish at different times, ask the queue and sit without a tile beside lanes in whole tiles
and lanes in their reads' last tiles.  Scores and op bytes against the oracle; all seven bs_* counters of the counting
build, gact_tiles and the sum of blocks per tile against tests/bs_flow.py, which decides full width per block from the
block's own stream words.  The batch is the first 64 reads of test_gpu_gact_bs_counters' unequal batch: the T = 320
reference is computed once for both modules."""
import numpy as np
import pytest

# The batch builder, the oracle reference (with its per-module cache, which is why the T = 320 reference is computed once)
# and the counter check are test_gpu_gact_bs_counters' own: this file is a second set of cases for that module's
# machinery and changes with it.
from test_gpu_gact_bs_counters import _Batch, _pairs

pytestmark = pytest.mark.gpu

W = 128


@pytest.fixture(scope="module")
def one_wave(gpu):
    lengths = [int(x) for x in np.random.default_rng(41).integers(330, 2001, size=96)]
    lengths[:3] = [330, 2000, 641]
    b = _Batch(gpu, _pairs(lengths[:64], "unequal"))
    yield b
    b.close()


@pytest.mark.parametrize("T,O", [(320, 120), (128, 32)])
def test_one_wavefront_of_unequal_reads(one_wave, T, O):
    gact = (T, O, W)
    got, st = one_wave.run(gact, True, waves=1)
    one_wave.check_results(got, gact)
    want = one_wave.check_counters(st, 1, gact)
    # the batch mixes what the change touches: both block forms, blocks left out, lanes that ask the queue again
    assert want["bs_blocks_full"] > 0 and want["bs_blocks_windowed"] > 0 and want["bs_refill_rounds"] > 3
    assert want["bs_pass1_pairs_masked"] > 0 and want["bs_pass1_pairs_plain"] > 0
    # and walks that end at the read's end (text left over) as well as at the text's (the rest of the read follows as 'I')
    ref, _ = one_wave.reference(gact)
    text_used = [sum(op != ord("I") for op in ops) for _, ops in ref]
    by_text = sum(used == len(d) and ops.endswith(b"I") for used, (_, ops), (_, d) in zip(text_used, ref, one_wave.pairs))
    by_read = sum(used < len(d) for used, (_, d) in zip(text_used, one_wave.pairs))
    print("walks ended by text end:", by_text, "by read end:", by_read)
    assert by_text > 0 and by_read > 0
    # with counting off: the same bytes, and nothing counted
    off, st_off = one_wave.run(gact, False, waves=1)
    assert all(st_off[k] == 0 for k in ("bs_blocks_full", "bs_blocks_windowed", "bs_blocks_skipped", "bs_wave_tiles"))
    for key in ("n_ops", "score", "meta_r"):
        assert got[key].tobytes() == off[key].tobytes(), key
    for k, n_ops in enumerate(got["n_ops"]):
        assert got["ops"][k, :n_ops].tobytes() == off["ops"][k, :n_ops].tobytes(), k
