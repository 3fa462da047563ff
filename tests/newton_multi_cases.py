"""Shapes, residual rows, the independent reference and the error measure of
the Newton directions for a block of residuals (Optimizer.newton_solve,
Batch.newton_solve_all), shared by tests/test_gpu_newton_multi.py (the device)
and tests/test_oracle_newton_multi.py (what the reference relies on, no GPU).

The reference does not go through the augmented system at all: it is the
dense Jacobian J of "newton system / lhs" (tests/golden/formulations.txt) at
the iterate, numpy.linalg.solve(J, -r) per row, and get_max_step_ restated in
numpy.  SlackedSlacks inequalities with both bounds, equalities Regularization
(delta = 1e-4) or None; absent slots dropped (m = 0: the box-only form).
"""
import functools

import numpy as np

import oracle

# (n, m, p): the smallest shapes at which each piece can go wrong
SHAPES = [
    (12, 5, 3),     # N = 20: below one inner block, every slot a different length
    (48, 16, 8),    # N = 72: one block plus 8 columns
    (256, 48, 17),  # N = 321: odd N; with EqualityHandling::None L = 1585 is odd too: the even stride
    (40, 0, 0),     # box-only: the explicit x bounds enter alpha
]
# (n, m, p, batch, seed0)
BATCHES = [(48, 16, 8, 3, 1000), (130, 40, 22, 3, 1100)]
# the step-length kernel takes 1024 threads per row from n + m > 2048 (csrc/newton.hip qp_ratio_multi): the last
# shape of the 256-thread kernel and the first of the other
RATIO_WIDE = 2048
RATIO_SHAPES = [(2032, 16, 0), (2040, 16, 0)]
SEED = 7
RPG = 4                      # csrc/kernels.h IPMZ_NEWTON_MULTI_RPG: rows one thread walks
RHS_COUNTS = (1, 3, 17, 6)   # 17 = 4 groups + one row; 6: not a multiple of the row group either
RHS_MAX = max(RHS_COUNTS)
TOL = 1e-10   # |d - d_ref|_inf <= TOL * max(1, |d_ref|_inf) per row (README: the Newton-direction bar)
DELTA = 1e-4


def case_id(c):
    return "n%d_m%d_p%d" % tuple(c[:3])


def even(k):
    return k + (k & 1)


@functools.lru_cache(maxsize=None)
def qp(n, m, p, seed=SEED):
    """The generated QP, made once per session and never modified."""
    return oracle.gen_qp(n, m, p, seed)


def sizes(q, eq_none):
    n, m, p = q["n"], q["m"], q["p"]
    order = oracle.newton_order(n, m, p, eq_none)
    return order, {s: oracle.slot_size(s, n, m, p, eq_none) for s in order}


def offsets(q, eq_none):
    order, sz = sizes(q, eq_none)
    off, o = {}, 0
    for s in order:
        off[s] = o
        o += sz[s]
    return order, sz, off, o


def split(q, flat, eq_none):
    order, sz, off, _ = offsets(q, eq_none)
    return {s: flat[off[s]:off[s] + sz[s]] for s in order}


@functools.lru_cache(maxsize=None)
def rows(L, B=1):
    """(B, RHS_MAX, L) standard-normal residual rows; a call with fewer rows uses the first ones."""
    r = np.random.default_rng(9000 + L).standard_normal((B, RHS_MAX, L))
    r.setflags(write=False)
    return r


def full_jacobian(q, vars_, order=None, eq_none=False):
    """The dense J of "newton system / lhs": block row v is the equation whose
    residual is r_v, block column w the Newton variable w, both in Newton order."""
    order_, sz, off, L = offsets(q, eq_none)
    order = order or order_
    assert list(order) == list(order_)
    v = split(q, np.asarray(vars_), eq_none)
    J = np.zeros((L, L))

    def put(rs, cs, M):
        if rs in off and cs in off:
            J[off[rs]:off[rs] + sz[rs], off[cs]:off[cs] + sz[cs]] = M

    def eye(s, f=1.0):
        return f * np.eye(sz[s])

    put("x", "x", q["Q"])
    put("x", "lambda_A", q["A"].T)
    put("x", "lambda_C", q["C"].T)
    put("x", "lambda_y", -np.eye(q["n"]))
    put("x", "lambda_z", np.eye(q["n"]))
    put("lambda_A", "x", q["A"])
    if "s" in off:
        put("lambda_A", "s", -eye("s"))
        put("s", "lambda_A", -eye("s"))
        put("s", "lambda_g", -eye("s"))
        put("s", "lambda_h", eye("s"))
        put("lambda_g", "s", -eye("s"))
        put("lambda_g", "g", eye("s"))
        put("lambda_h", "s", eye("s"))
        put("lambda_h", "h", eye("s"))
    put("lambda_C", "x", q["C"])
    if "p" in off:
        put("lambda_C", "p", eye("p", DELTA))
        put("p", "lambda_C", eye("p", DELTA))
        put("p", "p", eye("p"))
    put("lambda_y", "x", -np.eye(q["n"]))
    put("lambda_y", "y", np.eye(q["n"]))
    put("lambda_z", "x", np.eye(q["n"]))
    put("lambda_z", "z", np.eye(q["n"]))
    for sl, du in (("g", "lambda_g"), ("h", "lambda_h"), ("y", "lambda_y"), ("z", "lambda_z")):
        if sl in off:
            put(sl, du, np.diag(v[sl]))   # [G -> lambda_g column]
            put(sl, sl, np.diag(v[du]))   # [Lambda_g -> g column]
    return J


def residuals_numpy(q, vars_, eq_none=False):
    """The shorthand definitions r_v at mu = 0, in Newton order."""
    order, sz, off, L = offsets(q, eq_none)
    v = split(q, np.asarray(vars_), eq_none)
    x = v["x"]
    r = {}
    rx = q["c"] + v["lambda_z"] + q["Q"] @ x
    if "lambda_A" in v:
        rx = rx + q["A"].T @ v["lambda_A"]
    if "lambda_C" in v:
        rx = rx + q["C"].T @ v["lambda_C"]
    r["x"] = rx - v["lambda_y"]
    if "s" in v:
        r["lambda_A"] = q["A"] @ x - v["s"]
        r["s"] = -(v["lambda_A"] + v["lambda_g"] - v["lambda_h"])
        r["lambda_g"] = q["lA"] + v["g"] - v["s"]
        r["lambda_h"] = v["h"] + v["s"] - q["uA"]
        r["g"] = v["g"] * v["lambda_g"]
        r["h"] = v["h"] * v["lambda_h"]
    if "lambda_C" in v:
        if "p" in v:
            r["lambda_C"] = q["C"] @ x + DELTA * v["p"] - q["d"]
            r["p"] = v["p"] + DELTA * v["lambda_C"]
        else:
            r["lambda_C"] = q["C"] @ x - q["d"]
    r["lambda_y"] = q["lx"] + v["y"] - x
    r["lambda_z"] = x + v["z"] - q["ux"]
    r["y"] = v["y"] * v["lambda_y"]
    r["z"] = v["z"] * v["lambda_z"]
    return np.concatenate([r[s] for s in order])


def max_step_numpy(q, vars_, dir_, eq_none=False):
    """get_max_step_ (Optimizer.cpp:270-342) before the 0.995 factor: the
    fraction to the boundary of every non-negative Newton variable, capped at 1;
    when neither g nor h is a Newton variable (m = 0 here) also the explicit
    bounds l_x <= x <= u_x."""
    v, d = split(q, np.asarray(vars_), eq_none), split(q, np.asarray(dir_), eq_none)
    a = 1.0
    for s in v:
        if s in oracle.NONNEG:
            neg = d[s] < 0.0
            if neg.any():
                a = min(a, float(np.min(-v[s][neg] / d[s][neg])))
    if q["m"] == 0:
        x, dx = v["x"], d["x"]
        neg, pos = dx < 0.0, dx > 0.0
        if neg.any():
            a = min(a, float(np.min((q["lx"][neg] - x[neg]) / dx[neg])))
        if pos.any():
            a = min(a, float(np.min((q["ux"][pos] - x[pos]) / dx[pos])))
    return a


def reference(q, vars_, R, eq_none=False):
    """numpy.linalg.solve(J, -R^T)^T: one full Newton direction per row of R."""
    J = full_jacobian(q, vars_, eq_none=eq_none)
    return np.linalg.solve(J, -np.asarray(R).T).T


def row_err(X, X_ref):
    """max over rows of |x - x_ref|_inf / max(1, |x_ref|_inf); NaN counts as inf."""
    X, X_ref = np.asarray(X), np.asarray(X_ref)
    e = np.abs(X - X_ref).max(axis=-1) / np.maximum(1.0, np.abs(X_ref).max(axis=-1))
    e = np.where(np.isnan(e), np.inf, e)
    return float(np.max(e)) if e.size else 0.0


def ulps(a, b):
    """Distance of two doubles in units in the last place (same sign assumed)."""
    return int(abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64))))
