"""A plain `python bench.py` run: the timed steps and the line, no side leg, and --dump-outputs
writing what the last timed step returned (the cfg-2 search's winner, tests/golden/big_winners.json)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu


def test_plain_run_times_the_steps_and_dumps_the_last_result(tmp_path):
    out = os.path.join(str(tmp_path), "outputs")
    detail = os.path.join(str(tmp_path), "detail.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--prewarm", "0", "--dump-outputs", out, "--detail-file", detail],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(r.stdout.strip().splitlines()) == 1
    line = json.loads(r.stdout)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["metric"] == "pose-candidates x beams scored per second" and line["unit"] == "candidate-beams/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(line["config"]["units_per_step"] / (line["ms_per_step"] * 1e-3))
    with open(detail) as f:
        full = json.load(f)
    for leg in ("cpu_baseline", "host_call", "particle_filter", "cfg4_single_gpu", "default_search",
                "cfg1_search", "c_host_multi_device"):
        assert leg not in full, leg
    with open(os.path.join(HERE, "golden", "big_winners.json")) as f:
        want = json.load(f)["cfg2"]
    got = {name: np.load(os.path.join(out, name + ".npy"))
           for name in ("match_records", "score", "pose", "covariance", "best_index")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["match_records"].shape == (1, 12) and got["covariance"].shape == (3, 3)
    assert int(got["best_index"][0]) == want["best_index"] == line["match_result"]["best_index"]
    assert [float(v).hex() for v in got["pose"]] == want["pose_hex"]
    assert float(got["score"][0]) == pytest.approx(want["score"], abs=1e-12)
    assert np.allclose(got["covariance"], want["covariance"], rtol=1e-9, atol=0)
