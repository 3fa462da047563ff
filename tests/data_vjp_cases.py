"""Cotangent rows, the independent reference and the measures of the gradient with respect to the problem data
(ipmz_batch_data_vjp: Optimizer.data_grad_tensors; ipmz_amd.layer.solve_qp), shared by
tests/test_gpu_data_vjp.py, tests/test_gpu_qp_layer.py (the device) and tests/test_oracle_data_vjp.py (what the
reference relies on, no GPU).

Shapes, batches and the residuals' numpy restatement are those of tests/newton_multi_cases.py.  The reference for
the default form (SlackedSlacks inequalities, both bounds, equalities Regularization or None) is read off
nc.residuals_numpy's expressions: every r_v is affine in the data, so g_theta = (d r / d theta)^T w.  Every other
formulation is judged by the bilinear identity <w, r(theta + D) - r(theta)> = sum <g_theta, D_theta>, which is exact
for an affine map, on the device's own residual path.
"""
import functools

import numpy as np

import newton_multi_cases as nc

# load_tensors' names -> the keys of oracle.gen_qp's dict
KEYS = dict(Q="Q", c="c", l_x="lx", u_x="ux", A_ineq="A", l_A_ineq="lA", u_A_ineq="uA", A_eq="C", b_eq="d")
NAMES = tuple(KEYS)
MATRICES = ("Q", "A_ineq", "A_eq")
KCHUNK = 64  # csrc/kernels.h IPMZ_VJP_KCHUNK: QPs per chunk of a shared matrix block's sum over the batch
# (n, m, p, batch): nc.BATCHES, every residue of the batch mod 4 (the K tail of the 16x16x4 MFMA) and the chunk
# size - 1, + 0, + 1 at the smallest shape; n = 130: partial M / N tiles and an odd tile count
BATCH_CASES = [c[:4] for c in nc.BATCHES] + [(12, 5, 3, b) for b in (1, 2, 3, 5, 9, KCHUNK - 1, KCHUNK, KCHUNK + 1)]


def present(n, m, p):
    """The blocks a solver of these dimensions has."""
    return [k for k in NAMES if not ((k in ("A_ineq", "l_A_ineq", "u_A_ineq") and m == 0) or
                                     (k in ("A_eq", "b_eq") and p == 0))]


@functools.lru_cache(maxsize=None)
def cotangents(L, B=1):
    """(B, L) standard-normal cotangent rows."""
    w = np.random.default_rng(9700 + L).standard_normal((B, L))
    w.setflags(write=False)
    return w


def reference(q, vars_, w, eq_none=False):
    """The nine gradients of the default form at the iterate vars_, w one cotangent row in the order of the
    residuals: the transposes of nc.residuals_numpy's expressions, line by line."""
    v, ws = nc.split(q, np.asarray(vars_), eq_none), nc.split(q, np.asarray(w), eq_none)
    x, wx = v["x"], ws["x"]
    g = {}
    g["c"] = wx.copy()                                  # rx = c + ...
    g["Q"] = np.outer(wx, x)                            # ... + Q @ x
    g["l_x"] = ws["lambda_y"].copy()                    # r[lambda_y] = lx + y - x
    g["u_x"] = -ws["lambda_z"]                          # r[lambda_z] = x + z - ux
    if "s" in v:
        # rx += A.T @ lambda_A;  r[lambda_A] = A @ x - s
        g["A_ineq"] = np.outer(ws["lambda_A"], x) + np.outer(v["lambda_A"], wx)
        g["l_A_ineq"] = ws["lambda_g"].copy()           # r[lambda_g] = lA + g - s
        g["u_A_ineq"] = -ws["lambda_h"]                 # r[lambda_h] = h + s - uA
    if "lambda_C" in v:
        # rx += C.T @ lambda_C;  r[lambda_C] = C @ x [+ DELTA p] - d
        g["A_eq"] = np.outer(ws["lambda_C"], x) + np.outer(v["lambda_C"], wx)
        g["b_eq"] = -ws["lambda_C"]
    return g


def perturbed(q, deltas):
    """A copy of the QP dict with deltas (load_tensors' names) added."""
    out = dict(q)
    for k, d in deltas.items():
        out[KEYS[k]] = q[KEYS[k]] + d
    return out


def random_deltas(q, seed, names=None, scale=1e-2):
    """Standard-normal perturbations of the named blocks (default: all the QP has), scaled; the generated QPs keep
    l < u under them (bound gaps of order 1)."""
    rng = np.random.default_rng(seed)
    names = present(q["n"], q["m"], q["p"]) if names is None else names
    return {k: scale * rng.standard_normal(q[KEYS[k]].shape) for k in names}


def ld(a):
    return np.asarray(a, dtype=np.longdouble)


def bilinear_gap(w, r0, r1, grads, deltas):
    """|<w, r1 - r0> - sum <grad_theta, D_theta>| in longdouble."""
    lhs = np.sum(ld(w) * (ld(r1) - ld(r0)))
    rhs = sum(np.sum(ld(grads[k]) * ld(deltas[k])) for k in deltas)
    return float(abs(lhs - rhs))


def bilinear_bound(w, r0, r1):
    """The project's bar on the identity: nc.TOL sum |w| |r1 - r0| (each term of the inner product to TOL)."""
    return nc.TOL * float(np.sum(np.abs(w) * np.abs(np.asarray(r1) - np.asarray(r0))))


def rel_err(a, ref):
    """|a - ref|inf / max(1, |ref|inf); NaN counts as inf."""
    a, ref = np.asarray(a), np.asarray(ref)
    if a.size == 0:
        return 0.0
    e = float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))
    return np.inf if np.isnan(e) else e
