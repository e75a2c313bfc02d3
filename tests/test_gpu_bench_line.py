"""A plain `bench.py --gpus 1 --steps K --warmup W` run: K timed steps, the headline keys and nothing that only --full measures, and
with --dump-outputs the answer of the last timed step, equal to the unmodified reference's (tests/golden/ref_full_q1_sf1.tbl)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import goldens

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_plain_run_times_its_steps_and_dumps_the_answer(tmp_path):
    out = tmp_path / "out"
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--sf", "1", "--steps", "7", "--warmup", "2",
                         "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout[-1000:]
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["unit"] == "rows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int64" and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - line["config"]["rows"]) <= 1e-6 * line["config"]["rows"]
    assert not {"cpu_baseline", "extras", "parity_checked"} & set(line)
    assert "measured_read_roofline" not in line["roofline"]
    with open(os.path.join(ROOT, "tests", "golden", "ref_full_q1_sf1.tbl")) as f:
        want = goldens.golden_columns(f.read())
    assert sorted(p.name for p in out.iterdir()) == sorted(f"{c}.npy" for c in want)
    for name, values in want.items():
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float64 and got.tolist() == values, name
