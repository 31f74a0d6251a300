"""bench.py's one-line JSON contract on a short --full run of the headline
workload: BASELINE.json's metric and unit, a positive whole-job value, the
roofline block of the dominant kernel (frac <= 1), vs_baseline null
(BASELINE.md publishes no number), and the configuration it names; and a plain
run's leaner line with --dump-outputs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_bench_json_line_contract():
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--no-gap"], cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == base["metric"]
    assert d["unit"] == "coord updates/s" and d["value"] > 0 and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f64"
    assert d["config"]["workload"].startswith("C2") and d["config"]["eval_flow"].startswith("deferred")
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and 0 < r["frac"] <= 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert d["ms_per_step"] > 0 and abs(d["value"] - d["config"]["K_total"] * d["config"]["H"] /
                                        (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]


@pytest.mark.timeout(120)
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run (no --full) of a small C2-shaped shard: the headline keys
    only, none of the extra measurements, --steps timed steps, and
    --dump-outputs writes the last step's w, alpha, evaluation and the gap
    trajectory as float64 .npy files that agree with the result line."""
    import numpy as np
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--n", "40000", "--parts", "16", "--n-test", "4000", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "coord updates/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and abs(d["value"] - d["config"]["K_total"] * d["config"]["H"] /
                                        (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for k in ("cpu_baseline", "roofline", "roofline_eval", "kernel_ms", "time_to_gap_s", "gpu_telemetry"):
        assert k not in d, k
    assert len(d["gap_trajectory_timed"]) == 4
    a = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(a) == ["alpha", "eval", "gap_trajectory", "w"]
    assert all(x.dtype == np.float64 and np.all(np.isfinite(x)) for x in a.values())
    assert a["w"].shape == (47236,) and a["alpha"].shape == (40000,) and np.any(a["w"] != 0)
    assert a["alpha"].min() >= 0.0 and a["alpha"].max() <= 1.0  # the SDCA box constraint
    assert a["gap_trajectory"].tolist() == d["gap_trajectory_timed"]
    ev = dict(zip(d["dump_outputs"]["eval_fields"], a["eval"]))
    assert ev["gap"] == a["gap_trajectory"][-1] and ev["gap"] == ev["primal"] - ev["dual"]
    assert ev["test_rows"] == 4000 and ev["test_error"] == ev["test_err_count"] / ev["test_rows"]
