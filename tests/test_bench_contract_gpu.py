"""The driver reads ONE JSON line from `python bench.py --gpus N --steps K --warmup W`: this test runs the
N = 1 command as the driver does (a subprocess, its own process and library load) with a short K and checks
the line's keys, types and internal consistency -- the contract of the task statement, section 4."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_conforming_json_line(gpu_device):
    env = dict(os.environ)
    env.pop("RAGFIN_LIB", None)          # the product library, as the driver runs it
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5",
                        "--full", "--no-configs"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines            # exactly one line on stdout
    d = json.loads(lines[0])
    for key, typ in (("metric", str), ("value", (int, float)), ("unit", str), ("n_gpus", int), ("steps", int),
                     ("warmup", int), ("ms_per_step", (int, float)), ("higher_is_better", bool), ("scaling", str),
                     ("dtype", str), ("data", str), ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert key in d and isinstance(d[key], typ), key
    assert "vs_baseline" in d and d["vs_baseline"] is None        # BASELINE.md holds no published number for this metric
    assert d["n_gpus"] == 1 and d["steps"] >= 30 and d["warmup"] == 5 and d["higher_is_better"] is True
    assert d["scaling"] in ("weak", "strong") and "workload" in d["config"] and "model" not in d["config"]
    assert d["data"].startswith("synthetic") and d["dtype"] == "f16"
    # value = units processed / time of the timed region
    assert abs(d["value"] - 64 / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01
    rf = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in rf, key
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s")
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0.3 < rf["frac"] < 1.0
    cb = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in cb, key
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1 and cb["value"] > 0
    # the oracle check of the same run
    assert d["recall_at_10"] == 1.0 and d["ids_ranks_exact"] is True and d["checked_queries"] == 64


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(gpu_device, tmp_path):
    """Without --full the line carries the headline only; --dump-outputs writes what the last timed step
    returned, and those arrays are the C oracle's answer on the same seeded inputs."""
    import numpy as np

    from oracle import c_oracle, search as osearch
    env = dict(os.environ)
    env.pop("RAGFIN_LIB", None)
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "25", "--warmup", "3",
                        "--rows", "100000", "--dump-outputs", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for key, typ in (("metric", str), ("value", (int, float)), ("unit", str), ("higher_is_better", bool),
                     ("dtype", str), ("ms_per_step", (int, float))):
        assert key in d and isinstance(d[key], typ), key
    assert d["steps"] == 25 and d["warmup"] == 3 and d["flags_clean"] is True
    assert abs(d["value"] - 64 / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01
    for key in ("serial", "roofline", "survey_8d", "cpu_baseline", "configs", "recall_at_10"):
        assert key not in d, key                 # side measurements are --full only
    got = {n: np.load(out / (n + ".npy")) for n in ("scores", "ids", "exact_scores", "flags")}
    assert got["scores"].dtype == np.float32 and got["scores"].shape == (64, 10)
    assert got["ids"].dtype == np.float64 and got["exact_scores"].dtype == np.float64
    c16 = osearch.synth_unit_rows(100_000, 384, 1234)
    q16 = osearch.synth_unit_rows(64, 384, 5678)
    os_, oi = c_oracle.search(q16, c16, 10)
    assert np.array_equal(got["ids"], oi.astype(np.float64))
    assert np.array_equal(got["exact_scores"], os_)
    assert np.array_equal(got["scores"], os_.astype(np.float32))
    assert not got["flags"].any()


def test_dump_outputs_writes_float32_or_float64(tmp_path):
    """bench.dump_outputs keeps float32 / float64 as they are and widens integer arrays to float64 exactly."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench
    ids = torch.tensor([[0, 999_999, (1 << 40) + 3]], dtype=torch.int64)
    arrays = (torch.tensor([[0.5, -1.25]], dtype=torch.float32), ids,
              torch.tensor([[0.1, 0.2]], dtype=torch.float64), torch.tensor([0, 7], dtype=torch.int32))
    bench.dump_outputs(str(tmp_path / "d"), ("scores", "ids", "exact_scores", "flags"), arrays)
    for name, t, dtype in zip(("scores", "ids", "exact_scores", "flags"), arrays,
                              (np.float32, np.float64, np.float64, np.float64)):
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == dtype and a.shape == tuple(t.shape), name
        assert np.array_equal(a, t.numpy().astype(dtype)), name
    assert int(np.load(tmp_path / "d" / "ids.npy")[0, 2]) == (1 << 40) + 3
