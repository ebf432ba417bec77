"""bench.py's own contract on a small grid: a plain run times exactly --steps steps and skips the checks, --full adds them, and
--dump-outputs writes what the timed steps computed -- the same arrays with and without --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", "48", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)] + list(extra)
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    arrays = {n: np.load(os.path.join(out_dir, f"{n}.npy")) for n in ("x", "residual", "defect")}
    return out, arrays


def test_dump_of_a_long_vector_is_a_fixed_sample(tmp_path):
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.DUMP_SAMPLE + 12345
    x = torch.arange(n, dtype=torch.float64)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), x, -x, 0.5)
    xa, xb, ra = (np.load(tmp_path / d / f) for d, f in (("a", "x.npy"), ("b", "x.npy"), ("a", "residual.npy")))
    assert xa.dtype == np.float64 and xa.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(xa, xb) and np.array_equal(ra, -xa)                 # same positions in every run, for every vector
    assert (np.diff(xa) > 0).all() and xa[0] >= 0 and xa[-1] < n              # distinct entries, in order
    assert np.load(tmp_path / "a" / "defect.npy").tolist() == [0.5]


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain, a = _bench(tmp_path / "plain")
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["value"] > 0
    assert plain["ms_per_step"] == pytest.approx(1e3 / plain["value"], rel=1e-9)
    assert plain["solve"] is None and plain["cpu_baseline"] is None and plain["secondary"] is None
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["x"].shape == a["residual"].shape and a["x"].ndim == 1 and a["defect"].shape == (1,)
    assert np.isfinite(a["x"]).all() and np.isfinite(a["residual"]).all() and np.abs(a["x"]).max() > 0
    assert 0 < a["defect"][0] <= np.linalg.norm(a["residual"]) * (1 + 1e-12)   # ||r|| sums the owned entries only

    full, f = _bench(tmp_path / "full", "--full", "--cpu-iters", "0")
    assert full["solve"]["converged"] and full["steps"] == 3
    for n in a:
        assert np.array_equal(a[n], f[n]), n
