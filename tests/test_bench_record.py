"""bench.py's host side: the stdout line stays short enough for a log tail, and --dump-outputs keeps a fixed sample of
the outputs inside its byte budget in float formats that hold every value.  tests/golden/bench_record.json is a full
record (--full --record) of the default workload, GRCh38-sized child leg included."""
import json
import os

import numpy as np

import bench

GOLD = os.path.join(os.path.dirname(__file__), "golden", "bench_record.json")


def test_stdout_line_is_short_and_keeps_the_figures():
    with open(GOLD) as f:
        full = json.load(f)
    assert len(json.dumps(full)) > 20000
    line = json.dumps(bench.compact_record(full))
    assert len(line) < 6144 and "\n" not in line
    back = json.loads(line)
    for rec, want in ((back, full), (back["grch38"], full["grch38"])):
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                  "value_hbm_resident", "value_pcie_inclusive", "config", "speedup_vs_cpu"):
            assert rec[k] == want[k], k
        for k in ("kernel", "bound", "achieved", "peak", "frac"):
            assert rec["roofline"][k] == want["roofline"][k], k
        assert rec["cpu_baseline"]["value"] == want["cpu_baseline"]["value"]
        assert rec["pcie_inclusive"]["in_flight_dense_pinned"] == want["pcie_inclusive"]["in_flight_dense_pinned"]["value"]
    assert back["kernel_avg_ms"]["gact_bs_kernel"] == full["kernels"]["gact_bs_kernel"]["avg_ms"]


def test_stdout_line_of_a_record_without_optional_legs():
    with open(GOLD) as f:
        full = json.load(f)
    for k in ("pcie_inclusive", "isolated", "roofline"):
        full[k] = None
    full["grch38"] = dict(failed="child exit code 1", stderr_tail="x" * 1500)
    back = json.loads(json.dumps(bench.compact_record(full)))
    assert back["value"] == full["value"] and back["roofline"] is None and "pcie_inclusive" not in back
    assert back["grch38"]["failed"] == "child exit code 1" and len(back["grch38"]["stderr_tail"]) == 400


def test_full_is_an_option_that_is_off_by_default():
    assert bench.parse_args([]).full is False
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    assert bench.parse_args(["--steps", "7", "--full"]).full is True


def test_stdout_line_of_a_plain_run():
    """A run without --full has the headline figure, the workload, the index build and the kernel times of the timed
    steps: the line carries those and none of the legs that --full adds."""
    with open(GOLD) as f:
        full = json.load(f)
    headline = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "value_hbm_resident", "config", "streams")
    plain = {k: full[k] for k in headline + ("index",)}
    plain["kernels"] = {k: dict(ms_total=v["ms_total"], launches=v["launches"], avg_ms=v["avg_ms"]) for k, v in full["kernels"].items()}
    back = json.loads(json.dumps(bench.compact_record(plain)))
    for k in headline:
        assert back[k] == full[k], k
    assert back["kernel_avg_ms"]["gact_bs_kernel"] == full["kernels"]["gact_bs_kernel"]["avg_ms"]
    assert back["index"]["build_s"] == full["index"]["build_s"]
    for k in ("roofline", "cpu_baseline", "isolated"):
        assert back[k] is None, k
    for k in ("value_pcie_inclusive", "pcie_inclusive", "speedup_vs_cpu", "grch38"):
        assert k not in back, k


def test_dump_plan_is_fixed_and_within_budget(tmp_path):
    n, read_len = 100_000, 10_000                      # the default workload
    stride, store_stride = read_len + 1, 2 * read_len
    sel, rows = bench.dump_plan(n, stride, store_stride)
    again = bench.dump_plan(n, stride, store_stride)
    assert np.array_equal(sel, again[0]) and np.array_equal(rows, again[1])
    assert np.array_equal(sel, np.arange(n))           # per-read fields: every read
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0) and rows[-1] < n
    rng = np.random.default_rng(1)
    arrays = dict(read_index=sel, row_index=rows, best=rng.integers(-2**40, 2**40, size=(n, 3)),
                  score=rng.integers(-1, 3000, size=n).astype(np.int32), n_ops=np.zeros(n, dtype=np.int32),
                  meta_r=np.ones(n, dtype=np.int32), meta=rng.integers(0, 2**40, size=(n, 4)),
                  ops=rng.integers(0, 256, size=(len(rows), store_stride)).astype(np.uint8),
                  reads=rng.integers(0, 256, size=(len(rows), stride)).astype(np.uint8))
    total = bench.write_outputs(str(tmp_path), arrays)
    on_disk = sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path))
    assert total <= on_disk <= 64_000_000
    for name, a in arrays.items():
        got = np.load(os.path.join(tmp_path, name + ".npy"))
        assert got.dtype in (np.float32, np.float64) and got.shape == a.shape and np.array_equal(got, a), name
    # a batch too large for the budget: both samples shrink, nothing else changes
    sel, rows = bench.dump_plan(1_000_000, 100_001, 200_000)
    assert len(sel) * 12 * 8 + len(rows) * 4 * 300_001 <= 64_000_000 and len(rows) > 0 and len(sel) < 1_000_000
