"""Cotangent rows, the independent reference and the measures of the gradient with respect to the problem data
(ipmz_batch_data_vjp: Optimizer.data_grad_tensors; ipmz_amd.layer.solve_qp), shared by
tests/test_gpu_data_vjp.py, tests/test_gpu_qp_layer.py (the device) and tests/test_oracle_data_vjp.py (what the
reference relies on, no GPU).

Shapes, batches and the residuals' numpy restatement are those of tests/newton_multi_cases.py.  The reference for
the default form (SlackedSlacks inequalities, both bounds, equalities Regularization or None) is read off
nc.residuals_numpy's expressions: every r_v is affine in the data, so g_theta = (d r / d theta)^T w.  Every other
formulation is judged by the bilinear identity <w, r(theta + D) - r(theta)> = sum <g_theta, D_theta>, which is exact
for an affine map, on the device's own residual path -- and, elementwise, by reference_form: the transposes of the
formulation's own "shorthand definitions" (tests/golden/formulations.txt), which needs the iterate and the cotangent
only (tests/test_gpu_data_vjp_batch.py: every formulation and every loop of the batched kernels).
"""
import collections
import functools

import numpy as np

import ipmz_amd as I
import oracle

import batch_form_cases as fc
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


# ---------------------------------------------------------------------------
# Every served formulation: name -> (oracle.Form, equality handling "reg" / "none" / "pen").  The names are fc.FORMS'
# without eqss and naiveeq (refused) plus pen_sl, PenaltyFunction with Slacks; form_kw gives the solver's keywords.
FORM_TABLE = collections.OrderedDict([
    ("box", (oracle.Form(), "reg")), ("vlo", (oracle.Form(False, 3, 1), "reg")), ("vup", (oracle.Form(False, 3, 2), "reg")),
    ("vnone", (oracle.Form(False, 3, 0), "reg")), ("alo", (oracle.Form(False, 1, 3), "reg")),
    ("aup", (oracle.Form(False, 2, 3), "reg")), ("sl", (oracle.Form(True, 3, 3), "reg")),
    ("naive", (oracle.Form(naive=True), "reg")), ("pen", (oracle.Form(), "pen")), ("none", (oracle.Form(), "none")),
    ("pen_sl", (oracle.Form(True, 3, 3), "pen")),
])
FORM_NAMES = tuple(FORM_TABLE)
M0_FORMS = tuple(k for k in FORM_NAMES if k in fc.S0_FORMS or k == "pen_sl")  # (the others need m > 0)
# The loops of grad.hip at the smallest batch that reaches them, default form: (n, m, p, B).  257: a range of
# k_grad_vectors_shared holds 5 QPs (one full group of four plus a tail), the last non-empty range 2 of 5, ranges
# 52..63 none; 4097: past gridDim.y of k_grad_matrix (4096 // ceil(rows / 4)) and of k_grad_vectors (4096), 65
# chunks of the shared matrix sum, 65 QPs per range.  Two loops are out of reach of any shape a solver here is built
# for and have no case: the row loop of k_grad_matrix (rows > 8192) and the element loop of k_grad_vectors
# (max(n, m, p) > 524288).
LOOP_SHAPE = (12, 5, 3)
LOOP_BATCHES = (257, 4097)
GRID_Y = 4096   # csrc/grad.hip grad_grid: gridDim.x * gridDim.y <= this
SUM_GX = 2048   # ... and gridDim.x <= this, 256 threads each: k_grad_shared_sum loops from rows * n > 524288
BIG_N = 768     # n^2 = 589824 > SUM_GX * 256


def form_kw(name):
    """The keywords of I.Optimizer / I.Batch for a served formulation."""
    if name == "pen_sl":
        return dict(equality_handling=I.EQ_PENALTY, inequality_handling=I.INEQ_SLACKS)
    return dict(fc.FORMS[name].kw)


def form_absent(name):
    """The bound blocks the formulation lacks: their gradient is 0."""
    f = FORM_TABLE[name][0]
    return tuple(k for k, bit, b in (("l_x", 1, f.var_bounds), ("u_x", 2, f.var_bounds), ("l_A_ineq", 1, f.ineq_bounds),
                                     ("u_A_ineq", 2, f.ineq_bounds)) if not b & bit)


def form_offsets(name, n, m, p):
    """(order, sizes, offsets, length) of the formulation's Newton order."""
    f, eq = FORM_TABLE[name]
    order = oracle.newton_order(n, m, p, eq != "reg", f)
    sz = {s: oracle.slot_size(s, n, m, p, eq != "reg", f) for s in order}
    off, o = {}, 0
    for s in order:
        off[s] = o
        o += sz[s]
    return order, sz, off, o


def form_split(name, n, m, p, flat):
    order, sz, off, _ = form_offsets(name, n, m, p)
    return {s: flat[off[s]:off[s] + sz[s]] for s in order}


def reference_form(name, n, m, p, vars_, w):
    """The nine gradients (blocks of dimension 0 omitted) of a served formulation at the iterate vars_, w one
    cotangent row in the order of the residuals: the transposes of the "shorthand definitions" of the formulation's
    section of tests/golden/formulations.txt, line by line (residuals_form below restates them), mu held fixed.
    Neither the data nor the device enters."""
    f, eq = FORM_TABLE[name]
    v, ws = form_split(name, n, m, p, np.asarray(vars_)), form_split(name, n, m, p, np.asarray(w))
    x, wx = v["x"], ws["x"]
    g = {}
    g["c"] = wx.copy()                                      # r_x := (c + ...
    g["Q"] = np.outer(wx, x)                                # ... + (Q * x) ...
    g["l_x"], g["u_x"] = np.zeros(n), np.zeros(n)           # (a bound the formulation lacks)
    if f.slacks:
        if "lambda_y" in v:
            g["l_x"] = -(v["lambda_y"] * ws["lambda_y"])    # r_ly := (((X - L_x) * lambda_y) - (mu * e_x))
        if "lambda_z" in v:
            g["u_x"] = v["lambda_z"] * ws["lambda_z"]       # r_lz := (((U_x - X) * lambda_z) - (mu * e_x))
    else:
        if "lambda_y" in v:
            g["l_x"] = ws["lambda_y"].copy()                # r_ly := (l_x + y - x)
        if "lambda_z" in v:
            g["u_x"] = -ws["lambda_z"]                      # r_lz := (x + z - u_x)
    if m:
        g["l_A_ineq"], g["u_A_ineq"] = np.zeros(m), np.zeros(m)
        if f.naive:
            # r_x has (A^T * (lambda_h - lambda_g));  r_lg := (l_A + g - (A * x));  r_lh := (h + (A * x) - u_A)
            g["A_ineq"] = np.outer(ws["lambda_h"] - ws["lambda_g"], x) + np.outer(v["lambda_h"] - v["lambda_g"], wx)
            g["l_A_ineq"] = ws["lambda_g"].copy()
            g["u_A_ineq"] = -ws["lambda_h"]
        else:
            # r_x has (A^T * lambda_A);  r_lA := ((A * x) - s)
            g["A_ineq"] = np.outer(ws["lambda_A"], x) + np.outer(v["lambda_A"], wx)
            if f.slacks:
                if "lambda_g" in v:
                    g["l_A_ineq"] = -(v["lambda_g"] * ws["lambda_g"])   # r_lg := (((S - L_A) * lambda_g) - ...)
                if "lambda_h" in v:
                    g["u_A_ineq"] = v["lambda_h"] * ws["lambda_h"]      # r_lh := (((U_A - S) * lambda_h) - ...)
            else:
                if "lambda_g" in v:
                    g["l_A_ineq"] = ws["lambda_g"].copy()               # r_lg := (l_A + g - s)
                if "lambda_h" in v:
                    g["u_A_ineq"] = -ws["lambda_h"]                     # r_lh := (h + s - u_A)
    if p:
        # r_x has (C^T * lambda_C);  r_lC := ((C * x) [+ (delta * p)] - d), or -(d + (mu * lambda_C) - (C * x))
        g["A_eq"] = np.outer(ws["lambda_C"], x) + np.outer(v["lambda_C"], wx)
        g["b_eq"] = -ws["lambda_C"]
    return g


def residuals_form(name, q, vars_, mu):
    """The "shorthand definitions" r_v of the formulation's section of tests/golden/formulations.txt at the QP dict
    q (oracle.gen_qp's keys), the iterate vars_ and the barrier parameter mu, in Newton order."""
    f, eq = FORM_TABLE[name]
    n, m, p = q["n"], q["m"], q["p"]
    order = form_offsets(name, n, m, p)[0]
    v = form_split(name, n, m, p, np.asarray(vars_))
    x = v["x"]
    r = {}
    rx = q["c"]
    if "lambda_z" in v:
        rx = rx + v["lambda_z"]
    rx = rx + q["Q"] @ x
    if m:
        rx = rx + q["A"].T @ ((v["lambda_h"] - v["lambda_g"]) if f.naive else v["lambda_A"])
    if p:
        rx = rx + q["C"].T @ v["lambda_C"]
    if "lambda_y" in v:
        rx = rx - v["lambda_y"]
    r["x"] = rx
    if m and f.naive:
        ax = q["A"] @ x
        r["lambda_g"] = q["lA"] + v["g"] - ax
        r["lambda_h"] = v["h"] + ax - q["uA"]
        r["g"] = v["g"] * v["lambda_g"] - mu
        r["h"] = v["h"] * v["lambda_h"] - mu
    elif m:
        r["lambda_A"] = q["A"] @ x - v["s"]
        if "lambda_g" in v and "lambda_h" in v:
            r["s"] = -(v["lambda_A"] + v["lambda_g"] - v["lambda_h"])
        elif "lambda_g" in v:
            r["s"] = -(v["lambda_A"] + v["lambda_g"])
        else:
            r["s"] = v["lambda_h"] - v["lambda_A"]
        if f.slacks:
            if "lambda_g" in v:
                r["lambda_g"] = (v["s"] - q["lA"]) * v["lambda_g"] - mu
            if "lambda_h" in v:
                r["lambda_h"] = (q["uA"] - v["s"]) * v["lambda_h"] - mu
        else:
            if "lambda_g" in v:
                r["lambda_g"] = q["lA"] + v["g"] - v["s"]
                r["g"] = v["g"] * v["lambda_g"] - mu
            if "lambda_h" in v:
                r["lambda_h"] = v["h"] + v["s"] - q["uA"]
                r["h"] = v["h"] * v["lambda_h"] - mu
    if p:
        if eq == "reg":
            r["lambda_C"] = q["C"] @ x + nc.DELTA * v["p"] - q["d"]
            r["p"] = v["p"] + nc.DELTA * v["lambda_C"]
        elif eq == "none":
            r["lambda_C"] = q["C"] @ x - q["d"]
        else:
            r["lambda_C"] = -(q["d"] + mu * v["lambda_C"] - q["C"] @ x)
    if f.slacks:
        if "lambda_y" in v:
            r["lambda_y"] = (x - q["lx"]) * v["lambda_y"] - mu
        if "lambda_z" in v:
            r["lambda_z"] = (q["ux"] - x) * v["lambda_z"] - mu
    else:
        if "lambda_y" in v:
            r["lambda_y"] = q["lx"] + v["y"] - x
            r["y"] = v["y"] * v["lambda_y"] - mu
        if "lambda_z" in v:
            r["lambda_z"] = x + v["z"] - q["ux"]
            r["z"] = v["z"] * v["lambda_z"] - mu
    assert set(r) == set(order), (name, sorted(r), order)
    return np.concatenate([r[s] for s in order])


def shared_reference(refs):
    """The shared block of per-QP references (B, ...): (their longdouble sum over the QPs as float64, the error
    bound nc.TOL max(1, max_elem sum_z |g_z|)).  Any summation order of B doubles is within (B - 1) 2^-53 sum |g_z|
    of the exact sum -- 4.5e-13 sum |g_z| at B = 4097 -- so the bound holds for every order."""
    a = ld(refs)
    return np.asarray(a.sum(axis=0), dtype=np.float64), nc.TOL * max(1.0, float(np.abs(a).sum(axis=0).max()))


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
