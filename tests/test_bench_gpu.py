"""bench.py's two kinds of run: a plain run times the steps and prints the headline line, --full adds what takes work
of its own (here: the state checks and the stream-copy rate) without changing what the timed call computes."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_line(*extra):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--workload", "ising256k", "--steps", "20",
                        "--warmup", "10"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_bench_runs(tmp_path):
    plain = bench_line("--dump-outputs", str(tmp_path / "plain"))
    assert plain["metric"] == "variable-updates/sec" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["value"] > 0 and abs(plain["value"] * plain["ms_per_step"] / 1e3 - 512 * 512) < 1.0
    assert plain["parity"] is None and "cpu_baseline" not in plain
    assert plain["roofline"]["stream_copy_GBs"] is None and plain["roofline"]["launches"] > 0

    full = bench_line("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert full["parity"]["ok"] is True and full["parity"]["statistics"] == "counted"
    assert full["parity"]["tallied_sweeps"] == 20 and full["parity"]["tally_in_bounds"] is True
    assert full["roofline"]["stream_copy_GBs"] > 0
    for name in ("var_value", "marginals"):
        assert np.array_equal(np.load(str(tmp_path / "plain" / (name + ".npy"))),
                              np.load(str(tmp_path / "full" / (name + ".npy")))), name
