"""bench.py's command line: a plain run times the steps and prints the headline line only,
--full adds the other measurements, --dump-outputs writes the scores of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "parity")
FULL_ONLY = ("roofline", "cpu_baseline", "batch_c3", "affine_step", "c5", "byte_alphabets", "scaling_note")


def test_options_and_dump_format(tmp_path, monkeypatch):
    """CPU: --full is off by default, and dump_outputs writes float64 scores in order."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path / "d")])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == str(tmp_path / "d")
    bench.dump_outputs(args.dump_outputs, np.array([7458, 0, 2**31 - 1], dtype=np.int32))
    got = np.load(tmp_path / "d" / "scores.npy")
    assert got.dtype == np.float64 and got.tolist() == [7458.0, 0.0, float(2**31 - 1)]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_score(tmp_path, golden):
    """GPU: one plain run of the C2 headline: the line holds the headline keys and none of
    the --full measurements, `steps` is the number asked for, and scores.npy is the C2 golden."""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    for k in HEADLINE:
        assert k in line, k
    for k in FULL_ONLY:
        assert k not in line, k
    assert line["host_api"] is None
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["parity"] == "ok" and line["unit"] == "GCUPS" and line["higher_is_better"] is True
    assert abs(line["value"] - 65536 * 65536 / (line["ms_per_step"] * 1e-3) / 1e9) < 1e-3 * line["value"]
    got = np.load(out / "scores.npy")
    assert got.dtype == np.float64 and got.tolist() == [float(golden("configs.json")["C2"]["score"])]
