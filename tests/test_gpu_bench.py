"""bench.py end to end on a small workload: a plain run reports the headline figure and stops, --full goes on through the
replay, the PCIe-inclusive legs and the CPU oracle (whose results bench.py itself asserts equal to the GPU's), and both
kinds of run dump the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--ref-len", "500000", "--reads", "1024", "--read-len", "2000"]


def run_bench(extra, tmp_path, tag):
    record, dump = str(tmp_path / (tag + ".json")), str(tmp_path / tag)
    p = subprocess.run([sys.executable, BENCH] + SMALL + ["--record", record, "--dump-outputs", dump] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-3000:]
    with open(record) as f:
        return json.loads(lines[0]), json.load(f), p.stderr, dump


def test_plain_run_stops_at_the_headline_and_full_adds_the_other_legs(gpu, tmp_path):
    line, record, err, dump = run_bench([], tmp_path, "plain")
    assert (line["metric"], line["unit"], line["higher_is_better"], line["dtype"]) == ("aligned Gbp/sec", "Gbp/s", True, "u8/u64 integer")
    assert (line["n_gpus"], line["steps"], line["warmup"]) == (1, 3, 2)
    bases = 1024 * 2000
    assert line["value"] > 0 and line["value"] == pytest.approx(bases / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-9)
    assert line["kernel_avg_ms"]["seed_search_kernel"] > 0
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["isolated"] is None
    for k in ("pcie_inclusive", "value_pcie_inclusive", "cpu_baseline", "roofline", "isolated", "stats", "grch38"):
        assert k not in record, k
    assert "pcie leg" not in err and "sanity" not in err

    fline, frecord, ferr, fdump = run_bench(["--full", "--pcie-steps", "2", "--cpu-seconds", "0.5"], tmp_path, "full")
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "config"):
        assert fline[k] == line[k], k
    assert fline["value"] > 0 and fline["value_pcie_inclusive"] > 0 and fline["cpu_baseline"]["value"] > 0
    assert fline["roofline"]["kernel"] in frecord["isolated"]["kernels"]
    assert len(frecord["pcie_inclusive"]["checked"]) > 0
    assert frecord["algorithmic_bytes_per_base"]["device_layout"]["seeds"] > 0      # the counting build of the seed kernel ran
    assert "grch38" not in frecord                                 # that leg belongs to the default workload alone
    assert "pcie leg" in ferr and "sanity" in ferr

    names = sorted(os.listdir(dump))
    assert names == sorted(os.listdir(fdump)) and "score.npy" in names
    for name in names:
        assert np.array_equal(np.load(os.path.join(dump, name)), np.load(os.path.join(fdump, name))), name
