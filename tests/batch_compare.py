"""The bounds of the batched-step comparisons and the helpers that apply them,
shared by tests/test_gpu_batch_large.py and tests/test_gpu_batch_forms.py.

Bounds (BASELINE.json north star, test_gpu_parity.py): f, res, mu within
1e-12 relative; alpha_aff, mu_aff, sigma, alpha and every block of both
directions within 1e-9 relative; ||dx_gpu - dx_cpu||_inf < 1e-10.
"""
import numpy as np
import pytest

I = pytest.importorskip("ipmz_amd")
DX_TOL = 1e-10
STATE_KEYS = ("f", "res", "mu")
STEP_KEYS = ("alpha_aff", "mu_aff", "sigma", "alpha")


class Worst:
    """Worst figure per bound over a case, with where it occurred."""

    BOUNDS = {"f/res/mu rel": 1e-12, "step scalars rel": 1e-9, "direction blocks rel": 1e-9, "|dx - dx_cpu|": DX_TOL}

    def __init__(self, label, bounds=None):
        self.label = label
        self.bounds = dict(self.BOUNDS, **(bounds or {}))
        self.fig = {k: (0.0, None) for k in self.bounds}

    def add(self, key, err, where):
        err = float("inf") if np.isnan(err) else float(err)
        if err > self.fig[key][0]:
            self.fig[key] = (err, where)

    def check(self):
        for k, (err, where) in self.fig.items():
            print(f"{self.label}: {k} {err:.3e} (bound {self.bounds[k]:.3e}) at {where}", flush=True)
        for k, (err, where) in self.fig.items():
            assert err < self.bounds[k], (self.label, k, err, self.bounds[k], where)


def _rel(got, ref):
    return abs(got - ref) / max(1.0, abs(ref))


def _compare_step(w, o, rec, sc, daff, dirv, where):
    """One QP's step against its oracle's (rec: the oracle's record, sc: the
    batch's scalars after the step)."""
    n = o.qp["n"]
    for k in STEP_KEYS:
        w.add("step scalars rel", _rel(sc[I.SC[k]], rec[k]), where + (k,))
    for tag, got, ref in (("daff", daff, o.daff()), ("dir", dirv, o.dir())):
        sg, sr = o.split(got), o.split(ref)
        for s in o.order:
            w.add("direction blocks rel", np.abs(sg[s] - sr[s]).max() / max(1.0, np.abs(sr[s]).max()), where + (tag, s))
        w.add("|dx - dx_cpu|", np.abs(got[:n] - ref[:n]).max(), where + (tag,))
