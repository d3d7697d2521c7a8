"""-m gpu: `bench.py --dump-outputs DIR` -- exactly K timed steps, and what the last of them computed (predictions and
weights) written as DIR/<name>.npy, the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from util import close

pytestmark = pytest.mark.gpu


def _bench_dump(out_dir, steps=3, warmup=2):
    r = subprocess.run([sys.executable, "bench.py", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
                        "--extra", "", "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == steps and rec["config"]["timing"]["repeats"] == 1
    assert rec["config"]["timing"]["steps_per_repeat"] == steps
    return {f[:-len(".npy")]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_bench_dumps_the_last_timed_step_reproducibly(tmp_path):
    a = _bench_dump(tmp_path / "a")
    b = _bench_dump(tmp_path / "b")
    assert a["preds"].shape == (512, 41)
    assert len(a) > 4 and set(a) == set(b)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.isfinite(a[k]).all(), k
        close(a[k], b[k], k, 1e-3, 1e-3)


def test_plain_run_measures_the_headline_only():
    """Without --full the run sets up, warms up, times its steps and prints the line: no in-step roofline, no other
    configurations, no CPU baseline.  Naming other configurations without --full is refused before anything runs."""
    r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "2"], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["metric"] == "seed-nodes/sec" and rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["dtype"] == "bf16"
    assert rec["roofline"] is None and rec["extra"] == {} and rec["cpu_baseline"] is None
    r = subprocess.run([sys.executable, "bench.py", "--extra", "max_pool"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]
