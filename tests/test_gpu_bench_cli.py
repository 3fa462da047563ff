"""bench.py's command line: a plain run times the headline only, --steps sets
the number of timed steps, and --dump-outputs writes what the last timed step
left -- the same arrays, bit for bit, that a caller stepping the same seeded
QP through the same path reads back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 2
N, M, P = 1024, 256, 128  # bench.py's "small" workload


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench") / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--workload", "small", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), d


def test_plain_line(plain_run):
    out, _ = plain_run
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == STEPS and out["warmup"] == WARMUP
    assert out["unit"] == "steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-12)
    # everything but the headline belongs to --full
    for k in ("cpu_baseline", "batched", "batched_shard", "configs", "phase_ms_per_step", "roofline"):
        assert k not in out, k


def test_dump_is_the_last_timed_steps_output(plain_run):
    _, d = plain_run
    names = sorted(f for f in os.listdir(d))
    assert names == ["daff.npy", "dir.npy", "residuals.npy", "scalars.npy", "vars.npy"]
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in names}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())

    ctx = I.Context(0, stream=torch.cuda.current_stream().cuda_stream, nbo=0, nbi=64)  # as bench.py
    g = I.Optimizer(N, M, P, ctx)
    g.generate(1234)
    for _ in range(WARMUP + STEPS):
        g.step(I.STEP_RESTART_IF_CONVERGED | I.STEP_GRAPH)
    torch.cuda.synchronize()
    want = {"vars": g.vars(), "daff": g.daff(), "dir": g.dir(), "residuals": g.residuals(),
            "scalars": np.array(list(g.scalars().values()))}
    g.close()
    assert np.abs(want["dir"]).max() > 0
    for k, a in want.items():
        assert np.array_equal(got[k], a), k
