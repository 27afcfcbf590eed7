"""Host I/O probe (CPU only): throughput of the FASTQ batch loader and of the SAM formatter on 10 kbp reads.
python tools/io_probe.py [n_reads]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longreadmapper_amd import mapper, synth, textio
from longreadmapper_amd.capi import lib

n, Lr = int(sys.argv[1]) if len(sys.argv) > 1 else 4000, 10000
ref = synth.reference(2_000_000, seed=1)
r = synth.reads([ref], n, Lr, synth.ONT, seed=3)
path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "io_probe_%d.fq" % os.getpid())
with open(path, "wb") as f:
    q = b"I" * Lr
    for i in range(n):
        f.write(b"@read%d some comment\n" % i + r["reads"][i, :Lr].tobytes() + b"\n+\n" + q + b"\n")
size = os.path.getsize(path)
rd = textio.Reader(path)
t0 = time.perf_counter()
got = rd.next(n)
t1 = time.perf_counter()
assert got == n
print("reader: %d reads, %.1f MB of FASTQ in %.3f s = %.0f MB/s = %.3f Gbp/s" % (n, size / 1e6, t1 - t0, size / 1e6 / (t1 - t0), n * Lr / (t1 - t0) / 1e9))
mta = textio.mta_table([(b"chrA", 0, len(ref))])
store = np.full((n, 2 * Lr), ord("="), dtype=np.uint8)
store[:, ::7] = ord("X"); store[:, ::31] = ord("I"); store[:, 5::43] = ord("D")
score = np.full(n, 980, dtype=np.int32)
cig = textio.cigar_table(store.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(store.shape[1]), 11000, score)
meta_r = np.ones(n, dtype=np.int32)
meta = np.zeros(n, dtype=mapper.META_DT)
meta["off"] = np.arange(n) * 13
ln = C.c_uint64()
for _ in range(2):                       # the second call has the thread team and the allocator warm; the C call alone is timed
    t0 = time.perf_counter()
    t = lib.lrm_sam_format(C.byref(rd.batch), mta, len(mta), cig.ctypes.data, score.ctypes.data, meta.ctypes.data, meta_r.ctypes.data, n, C.byref(ln))
    t1 = time.perf_counter()
    lib.lrm_free(t)
print("sam_format: %.1f MB of SAM in %.3f s = %.0f MB/s = %.3f Gbp/s (%d threads)" % (ln.value / 1e6, t1 - t0, ln.value / 1e6 / (t1 - t0), n * Lr / (t1 - t0) / 1e9, os.cpu_count()))
rd.close()
os.remove(path)
