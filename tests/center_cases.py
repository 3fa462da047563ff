"""The numpy reference of centering on the central path (Optimizer.center, ipmz_batch_center), shared by
tests/test_gpu_center.py (the device) and tests/test_oracle_center.py (what the reference relies on, no GPU).

center() is the device's loop restated: r = dc.residuals_form(name, q, v, kappa) -- the formulation's "shorthand
definitions" at mu = kappa -- tested in the infinity norm, a dense solve with the Jacobian of those residuals, the
step's ratio test and the update v <- v + 0.995 alpha d.  Neither the augmented system nor the device enters.

The closed form: a box-constrained QP with diagonal Q separates per coordinate; with y = x - l, z = u - x,
lambda_y = kappa / y, lambda_z = kappa / z the path point is the root of q x + c - kappa / (x - l) + kappa / (u - x)
in (l, u), where that function rises from -inf to +inf: bisection.
"""
import functools

import numpy as np

import batch_form_cases as fc
import data_vjp_cases as dc
import newton_multi_cases as nc
import oracle

KAPPAS = (1e-2, 1e-4)
TOL = 1e-10        # |r(z; kappa)|inf <= TOL: the stop of the loop
MAX_ITER = 30      # the cap the GPU tests call with (tests/test_oracle_center.py guards it)
# the formulations ipmz_batch_center serves, of fc.FORMS
FORMS = tuple(f for f in fc.FORMS if f not in ("sl", "pen", "eqss", "naiveeq"))
U = 2.0 ** -52


def jacobian_form(name, q, vars_, mu=0.0):
    """d dc.residuals_form(name, q, v, mu) / d v at v = vars_: block row s the equation r_s, block column w the
    Newton variable w, both in the formulation's Newton order.  mu enters only PenaltyFunction's block."""
    f, eq = dc.FORM_TABLE[name]
    n, m, p = q["n"], q["m"], q["p"]
    order, sz, off, L = dc.form_offsets(name, n, m, p)
    v = dc.form_split(name, n, m, p, np.asarray(vars_))
    x = v["x"]
    J = np.zeros((L, L))

    def put(rs, cs, M):
        if rs in off and cs in off:
            J[off[rs]:off[rs] + sz[rs], off[cs]:off[cs] + sz[cs]] = M

    In, Im, Ip = np.eye(n), np.eye(m), np.eye(p)
    put("x", "x", q["Q"])
    put("x", "lambda_z", In)
    put("x", "lambda_y", -In)
    if m and f.naive:
        put("x", "lambda_h", q["A"].T)
        put("x", "lambda_g", -q["A"].T)
        put("lambda_g", "g", Im)
        put("lambda_g", "x", -q["A"])
        put("lambda_h", "h", Im)
        put("lambda_h", "x", q["A"])
    elif m:
        put("x", "lambda_A", q["A"].T)
        put("lambda_A", "x", q["A"])
        put("lambda_A", "s", -Im)
        put("s", "lambda_A", -Im)
        put("s", "lambda_g", -Im)
        put("s", "lambda_h", Im)
        if f.slacks:
            if "lambda_g" in v:
                put("lambda_g", "s", np.diag(v["lambda_g"]))
                put("lambda_g", "lambda_g", np.diag(v["s"] - q["lA"]))
            if "lambda_h" in v:
                put("lambda_h", "s", -np.diag(v["lambda_h"]))
                put("lambda_h", "lambda_h", np.diag(q["uA"] - v["s"]))
        else:
            put("lambda_g", "g", Im)
            put("lambda_g", "s", -Im)
            put("lambda_h", "h", Im)
            put("lambda_h", "s", Im)
    if p:
        put("x", "lambda_C", q["C"].T)
        put("lambda_C", "x", q["C"])
        if eq == "reg":
            put("lambda_C", "p", nc.DELTA * Ip)
            put("p", "p", Ip)
            put("p", "lambda_C", nc.DELTA * Ip)
        elif eq == "pen":
            put("lambda_C", "lambda_C", -mu * Ip)
    if f.slacks:
        if "lambda_y" in v:
            put("lambda_y", "x", np.diag(v["lambda_y"]))
            put("lambda_y", "lambda_y", np.diag(x - q["lx"]))
        if "lambda_z" in v:
            put("lambda_z", "x", -np.diag(v["lambda_z"]))
            put("lambda_z", "lambda_z", np.diag(q["ux"] - x))
    else:
        put("lambda_y", "y", In)
        put("lambda_y", "x", -In)
        put("lambda_z", "z", In)
        put("lambda_z", "x", In)
    for sl, du in (("g", "lambda_g"), ("h", "lambda_h"), ("y", "lambda_y"), ("z", "lambda_z")):
        if sl in off:
            put(sl, sl, np.diag(v[du]))
            put(sl, du, np.diag(v[sl]))
    return J


def max_step_form(name, q, vars_, dir_):
    """get_max_step_ before the 0.995 factor (csrc/newton.hip ratio_elem): the fraction to the boundary of every
    non-negative Newton variable the formulation has, capped at 1; where neither g nor h is a Newton variable
    (InequalityHandling::Slacks, or m == 0) also the explicit bounds on x and s, both sides always."""
    f = dc.FORM_TABLE[name][0]
    n, m, p = q["n"], q["m"], q["p"]
    v, d = dc.form_split(name, n, m, p, np.asarray(vars_)), dc.form_split(name, n, m, p, np.asarray(dir_))
    a = 1.0
    for s in v:
        if s in oracle.NONNEG:
            neg = d[s] < 0.0
            if neg.any():
                a = min(a, float(np.min(-v[s][neg] / d[s][neg])))
    if f.slacks or m == 0:
        pairs = [(v["x"], d["x"], q["lx"], q["ux"])] + ([(v["s"], d["s"], q["lA"], q["uA"])] if m else [])
        for val, dv, lo, up in pairs:
            neg, pos = dv < 0.0, dv > 0.0
            if neg.any():
                a = min(a, float(np.min((lo[neg] - val[neg]) / dv[neg])))
            if pos.any():
                a = min(a, float(np.min((up[pos] - val[pos]) / dv[pos])))
    return a


def resid_norm(name, q, v, kappa):
    e = float(np.abs(dc.residuals_form(name, q, v, kappa)).max())
    return np.inf if np.isnan(e) else e


def center(q, v, kappa, tol=TOL, max_iter=MAX_ITER, form="box"):
    """(z, updates applied, centered, |r(z; kappa)|inf): damped Newton from v toward r(z; mu = kappa) = 0, the
    test first and after every update, at most max_iter updates."""
    v = np.array(v, dtype=np.float64)
    it = 0
    while True:
        r = dc.residuals_form(form, q, v, kappa)
        e = float(np.abs(r).max())
        if e <= tol or it >= max_iter:
            return v, it, bool(e <= tol), e
        d = np.linalg.solve(jacobian_form(form, q, v, kappa), -r)
        v = v + 0.995 * max_step_form(form, q, v, d) * d
        it += 1


def jinv_norm(name, q, v, kappa=0.0):
    """|J^{-1}|inf at v: two points whose residuals at the same kappa are below tol each lie within
    |J^{-1}|inf * 2 tol of each other, to first order (r(a) - r(b) = J (a - b))."""
    return float(np.abs(np.linalg.inv(jacobian_form(name, q, v, kappa))).sum(axis=1).max())


def residual_bound(q, z, tol=TOL):
    """The bar on numpy's residual of a device iterate that met tol on the device: tol plus the other summation
    order of the matrix-vector products, 8 n 2^-52 max(1, |z|inf) max(1, |data|inf)."""
    data = max(float(np.abs(q[k]).max()) for k in ("Q", "c", "A", "lA", "uA", "C", "d", "lx", "ux") if np.size(q[k]))
    return tol + 8 * q["n"] * U * max(1.0, float(np.abs(z).max())) * max(1.0, data)


@functools.lru_cache(maxsize=None)
def solved(form, shape, seed):
    """The oracle's converged iterate of the generated QP (made once, read-only)."""
    o = fc.FORMS[form].oracle(fc.qp(shape, seed))
    for _ in range(100):
        conv, rec = o.iterate()
        if rec["converged"]:
            break
    assert rec["converged"], (form, shape, seed)
    v = o.vars()
    v.setflags(write=False)
    return v


# ---------------------------------------------------------------------------
# the diagonal box QP: n = 12, bounds [-1, 1], unconstrained minimisers t up to 2.5 outside them, coordinates 4 and
# 8 with t exactly on a bound (the degenerate ones: active with a zero multiplier at the solution)
BOX_N = 12
BOX_T = np.array([0.3, -0.4, 1.7, -1.6, 1.0, 2.5, -2.0, 0.5, -1.0, 1.5, -1.5, 0.1])
BOX_DEGENERATE = (4, 8)
BOX_KAPPAS = (1e-2, 1e-3)


@functools.lru_cache(maxsize=None)
def box_case():
    """(QP dict, diag(Q), the cotangent g of x the gradient tests use)."""
    n = BOX_N
    rng = np.random.default_rng(5)
    g = rng.standard_normal(n)
    dq = rng.uniform(1.0, 4.0, n)
    q = dict(n=n, m=0, p=0, Q=np.diag(dq), c=-dq * BOX_T, A=np.zeros((0, n)), lA=np.zeros(0), uA=np.zeros(0),
             C=np.zeros((0, n)), d=np.zeros(0), lx=np.full(n, -1.0), ux=np.full(n, 1.0))
    assert all(-q["c"][i] / dq[i] in (-1.0, 1.0) for i in BOX_DEGENERATE)
    for a in list(q.values()) + [dq, g]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return q, dq, g


def box_root(dq, c, l, u, kappa):
    """Per coordinate the root of q x + c - kappa / (x - l) + kappa / (u - x) in (l, u), by bisection down to
    adjacent doubles."""
    x = np.empty(len(dq))
    for i in range(len(dq)):
        lo, hi = float(l[i]), float(u[i])
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if dq[i] * mid + c[i] - kappa / (mid - l[i]) + kappa / (u[i] - mid) > 0.0:
                hi = mid
            else:
                lo = mid
        x[i] = 0.5 * (lo + hi)
    return x


def box_state(x, l, u, kappa):
    """The whole path point in the box-only Newton order x, lambda_y, lambda_z, y, z."""
    return np.concatenate([x, kappa / (x - l), kappa / (u - x), x - l, u - x])


def box_derivatives(dq, x, l, u, kappa):
    """dx/dc, dx/dQ_ii, dx/dl, dx/du per coordinate, with D = q + kappa / (x - l)^2 + kappa / (u - x)^2."""
    D = dq + kappa / (x - l) ** 2 + kappa / (u - x) ** 2
    return dict(c=-1.0 / D, Q=-x / D, l_x=kappa / ((x - l) ** 2 * D), u_x=kappa / ((u - x) ** 2 * D)), D


def box_implicit(q, v, g):
    """numpy implicit differentiation at the iterate v (J^T w = -g on x, then the numpy contraction of
    tests/data_vjp_cases.py): the gradients of <g, x> with respect to c, diag(Q), l_x, u_x."""
    J = nc.full_jacobian(q, v)
    gz = np.zeros(J.shape[0])
    gz[:q["n"]] = g
    ref = dc.reference(q, v, np.linalg.solve(J.T, -gz))
    return dict(c=ref["c"], Q=np.diag(ref["Q"]).copy(), l_x=ref["l_x"], u_x=ref["u_x"])
