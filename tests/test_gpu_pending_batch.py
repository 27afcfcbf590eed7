"""A PendingBatch that is never waited for: dropping it (or leaving its `with` block) waits for the ticket before the arrays
the host pipeline writes into may go, and the handle goes on working."""
import gc
import weakref

import numpy as np
import pytest

from longreadmapper_amd import index, mapper, synth


@pytest.mark.gpu
def test_a_dropped_pending_batch_completes_into_its_arrays(gpu):
    ref = synth.reference(100_000, seed=1)
    hi = index.HostIndex.build([ref], hlen=10)
    r = synth.reads([ref], 64, 300, synth.ONT, seed=3)
    lens, n = r["lens"], len(r["lens"])
    stride = (2 * int(lens.max()) + 15) // 16 * 16
    di = index.DeviceIndex.upload(hi, gpu)
    try:
        reads1, store1 = r["reads"].copy(), np.zeros((n, stride), dtype=np.uint8)
        want = mapper.map_batch_submit(di, reads1, lens, store=store1).wait()
        assert want["ops"] is store1 and (want["score"] >= 0).sum() > n // 2 and store1.any()
        assert not np.array_equal(reads1, r["reads"])                      # reverse-strand reads came back reverse-complemented

        reads2, store2 = r["reads"].copy(), np.zeros((n, stride), dtype=np.uint8)
        pending = mapper.map_batch_submit(di, reads2, lens.astype(np.int64), store=store2)     # (its uint32 lens are the batch's alone)
        finalizer = pending._finalizer
        assert finalizer.alive and pending.ticket is not None
        del pending
        gc.collect()
        assert not finalizer.alive
        assert store2.tobytes() == store1.tobytes() and reads2.tobytes() == reads1.tobytes()

        # a batch that alone owns what the handle's threads read and write: reads given as a temporary, lens converted for it
        store5 = np.zeros((n, stride), dtype=np.uint8)
        pending = mapper.map_batch_submit(di, r["reads"].copy(), lens.astype(np.int64), store=store5)
        own = [weakref.ref(a) for a in pending._keep]
        assert len(own) == 2 and all(w() is not None for w in own)
        got = pending.wait()
        assert all(w() is not None for w in own)                           # held through the wait, for as long as the batch lives
        assert store5.tobytes() == store1.tobytes() and np.array_equal(got["score"], want["score"])
        store5[:] = 0
        pending = mapper.map_batch_submit(di, r["reads"].copy(), lens.astype(np.int64), store=store5)
        own = [weakref.ref(a) for a in pending._keep]
        del pending, got
        gc.collect()
        assert store5.tobytes() == store1.tobytes() and all(w() is None for w in own)      # released, after the ticket was waited for

        reads3, store3 = r["reads"].copy(), np.zeros((n, stride), dtype=np.uint8)
        with mapper.map_batch_submit(di, reads3, lens, store=store3) as left:
            pass
        assert left.ticket is None and not left._finalizer.alive
        assert store3.tobytes() == store1.tobytes() and reads3.tobytes() == reads1.tobytes()
        with mapper.map_batch_submit(di, r["reads"].copy(), lens, store=store3) as waited:
            again = waited.wait()                                          # a batch waited for inside the block is left alone
        assert waited.ticket is None and np.array_equal(again["score"], want["score"])

        reads4 = r["reads"].copy()
        got = mapper.map_batch(di, reads4, lens)                           # lrm_map_batch on the same handle afterwards
        for key in ("best", "n_ops", "score", "meta", "meta_r"):
            assert np.array_equal(got[key], want[key]), key
        for i in range(n):
            assert mapper.ops_of(got, i) == mapper.ops_of(want, i), i
        assert reads4.tobytes() == reads1.tobytes()
    finally:
        di.close()
