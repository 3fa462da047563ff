"""Inputs, measures and tables for the factors and KKT solves on graded pivots,
shared by tests/test_gpu_graded_pivots.py (the device) and
tests/test_oracle_graded_cases.py (the reference alone, no GPU).  numpy only.

Two kinds of input put pivots of very different magnitude into a factor:

  graded(K0, span, seed) = S K0 S with S = diag(2^e_i), e_i integers uniform in
      [-span, span].  The scaling is by powers of two, so every operation of an
      unpivoted LDL^T commutes with it (multiply, fma, MFMA, the hardware
      reciprocal and a Newton step on it) as long as nothing over- or
      underflows and no pivot is exactly zero: the factor of S K0 S is exactly
      (S L0 S^-1, S D0 S), the solution of (S K0 S) x = S b0 is S^-1 x0.
  plant(oracle_qp, seed)  the oracle's initial iterate with every slack / dual
      pair overwritten by slack = u1 2^e, dual = u2 2^(lo - e): a late iterate's
      magnitudes (mu about 2e-9, KKT diagonals from about 6e-10 to 2e9) as an
      input to the linear algebra, not a point on a central path.

The measures are componentwise backward errors in np.longdouble, so an error
on a pivot of size 1e-20 counts as much as one on a pivot of size 1e20:

  omega_factor(K, L, D) = max_{i>=j} |K - L D L^T|_ij / (|L||D||L^T|)_ij
  omega_solve(K, L, D, b, x) = max_i |b - K x|_i / (|L||D||L^T||x|)_i
  omega_rows(J, d, r, rows) = max_{i in rows} |J d + r|_i / (|J||d| + |r|)_i

with the bounds (u = 2^-53, or 2^-24 for the fp32 factor)

  omega_factor <= 2 (N + 1) u   Higham's gamma_{N+1} for an unpivoted LDL^T with
                                exact division, doubled: l = a * rcp(d) is two
                                more roundings than a / d
  omega_solve  <= (3 N + 1) u   the factor plus the two sweeps
  omega_rows   <= 16 u          no slot's back-substitution formula has more
                                than eight rounded operations; doubled
"""
import functools

import numpy as np

import batch_kkt_cases as kc
import newton_multi_cases as nc
import oracle
import pivot_cases as pc

LD = np.longdouble
U = 2.0 ** -53
U32 = 2.0 ** -24
SPAN64 = 33    # pivots from about 1e-20 to 1e20
SPAN32 = 20    # everything that goes through fp32: nothing comes near its range
QD_SEED = 11   # pc.qd / pc.aug
SCALE_SEED = 12
PLANT_SEED = 3  # QP i of a batch: PLANT_SEED + i
FULL_ROWS_MAX = 1100  # omega_factor over every row up to this order, sampled rows above
ROWS_BOUND = 16 * U

# (N, (nbo, nbi)) of the fp64 factor: every blocking; the two large orders
FACTOR_CONFIGS = pc.ORACLE_CONFIGS
LARGE_OMEGA = (2560, (0, 64))   # equivariance + omega_factor on the sampled rows
LARGE_EQUIV = (4100, (0, 64))   # equivariance only
SOLVE_NRHS = (1, 3, 17)
NORMAL_CASES = [(150, 50), (450, 250)]
MIXED_ORDERS = (300, 700)
# (n, m, p, batch) of the assembly test, gen_qp seeds 1000 + i; and the box-only shape
ASSEMBLY_CASES = [(48, 16, 8, 3), (256, 48, 17, 3), (800, 200, 40, 2), (40, 0, 0, 1)]
QP_SEED = 1000
NEWTON_CASES = [(48, 16, 8, 3), (256, 48, 17, 3)]
SINGLE_KKT_ORDERS = (72, 321)  # Optimizer.kkt_solve: the panel path fed by the step's own assembly
REDUCED_SLOTS = ("x", "lambda_A", "lambda_C")  # the unknowns of the augmented system
# The slots eliminated by back-substitution are s, p, the duals and the slacks.  The block row s is what the
# elimination turned into the (lambda_A, lambda_A) row of K: with x and lambda_A it is one of the three block rows on
# which no componentwise bound holds (tests/test_oracle_graded_cases.py).  The others are bounded; the block rows
# named after a slack (and p) and those named after a dual are listed apart because the reference's order of a
# slack / dual pair meets the second kind only for the iterate's own residual (csrc/newton.hip backsub_elem).
UNBOUNDED_ROWS = ("x", "lambda_A", "s")
SLACK_ROWS = ("p", "g", "h", "y", "z")
DUAL_ROWS = ("lambda_g", "lambda_h", "lambda_y", "lambda_z")
BACKSUB_ROWS = SLACK_ROWS + DUAL_ROWS
PAIRS = (("g", "lambda_g"), ("h", "lambda_h"), ("y", "lambda_y"), ("z", "lambda_z"))


def factor_bound(N, u=U):
    return 2 * (N + 1) * u


def solve_bound(N, u=U):
    return (3 * N + 1) * u


# ---------------------------------------------------------------------------
# inputs
def scales(N, span, seed=SCALE_SEED):
    """diag(S): 2^e_i, e_i integers uniform in [-span, span]."""
    e = np.random.default_rng(seed).integers(-span, span, N, endpoint=True)
    return np.ldexp(1.0, e)


def graded(K0, span, seed=SCALE_SEED):
    """S K0 S (exact: powers of two, nothing leaves the range)."""
    s = scales(K0.shape[0], span, seed)
    return s[:, None] * K0 * s[None, :]


@functools.lru_cache(maxsize=None)
def qd_pair(N, span=SPAN64):
    """(K0, K, s, B0): pc.qd(N, QD_SEED), its graded form, diag(S) and 17 right-hand sides b0 (the graded ones are
    s * b0).  Made once and never modified."""
    K0 = pc.qd(N, QD_SEED)
    s = scales(N, span)
    K = s[:, None] * K0 * s[None, :]
    B0 = np.random.default_rng(100 + N).uniform(-1.0, 1.0, (max(SOLVE_NRHS), N))
    for a in (K0, K, s, B0):
        a.setflags(write=False)
    return K0, K, s, B0


@functools.lru_cache(maxsize=None)
def aug_pair(n, mp, span=SPAN64):
    K0 = pc.aug(n, mp, QD_SEED)
    N = n + mp
    s = scales(N, span)
    K = s[:, None] * K0 * s[None, :]
    B0 = np.random.default_rng(200 + N).uniform(-1.0, 1.0, (max(SOLVE_NRHS), N))
    for a in (K0, K, s, B0):
        a.setflags(write=False)
    return K0, K, s, B0


def plant(o, seed, lo=-30):
    """The iterate of OracleQP o with every slack / dual pair present overwritten: slack = u1 2^e, dual =
    u2 2^(lo - e), e an integer uniform in [lo, 0], u1 and u2 uniform in [1, 2).  Returns the state vector."""
    v = o.vars()
    parts = o.split(v)  # views
    rng = np.random.default_rng(seed)
    for sl, du in PAIRS:
        if sl in parts and du in parts:
            k = parts[sl].size
            e = rng.integers(lo, 0, k, endpoint=True)
            u1, u2 = rng.uniform(1.0, 2.0, k), rng.uniform(1.0, 2.0, k)
            parts[sl][:] = np.ldexp(u1, e)
            parts[du][:] = np.ldexp(u2, lo - e)
    return v


@functools.lru_cache(maxsize=None)
def planted(n, m, p, seed, plant_seed):
    """(oracle at the planted iterate, the iterate, sym KKT, oracle L, oracle D): once per QP, never modified."""
    o = oracle.OracleQP(kc.qp(n, m, p, seed))
    v = plant(o, plant_seed)
    o.set_vars(v)
    K = o.kkt()
    L, D = oracle.ldlt(K)
    for a in (v, K, L, D):
        a.setflags(write=False)
    return o, v, K, L, D


def planted_batch(n, m, p, B, seed0):
    return [planted(n, m, p, seed0 + i, PLANT_SEED + i) for i in range(B)]


# ---------------------------------------------------------------------------
# measures (np.longdouble)
def _unit_lower(L):
    N = L.shape[0]
    Lq = np.tril(np.asarray(L), -1).astype(LD)
    Lq[np.arange(N), np.arange(N)] = 1.0
    return Lq


def _ratio(num, den):
    """max num / den with 0 / 0 = 0 and a non-finite entry = inf."""
    if not (np.isfinite(num).all() and np.isfinite(den).all()):
        return float("inf")
    bad = (den == 0) & (num != 0)
    if bad.any():
        return float("inf")
    ok = den != 0
    return float((num[ok] / den[ok]).max()) if ok.any() else 0.0


def sample_rows(N, D, nbo, nbi):
    """Every row up to FULL_ROWS_MAX; above it the edge positions of the blocking, the 16 rows of smallest and of
    largest |D| and 16 drawn with a fixed seed."""
    if N <= FULL_ROWS_MAX:
        return np.arange(N)
    o = np.argsort(np.abs(D), kind="stable")
    r = np.random.default_rng(N).choice(N, 16, replace=False)
    return np.unique(np.concatenate([np.array(pc.positions(N, nbo, nbi)), o[:16], o[-16:], r]))


def omega_factor(K, L, D, rows=None):
    """max over rows i (default all) and j <= i of |K - L D L^T|_ij / (|L||D||L^T|)_ij, row by row.  L: the strict
    lower triangle is read, the unit diagonal implied.  K in any float type (float32 for the fp32 factor)."""
    N = len(D)
    if not (np.isfinite(np.asarray(L, dtype=np.float64)).all() and np.isfinite(np.asarray(D, dtype=np.float64)).all()):
        return float("inf")
    Lq, Dq = _unit_lower(L), np.asarray(D).astype(LD)
    aL, aD = np.abs(Lq), np.abs(Dq)
    worst = 0.0
    for i in (range(N) if rows is None else rows):
        Lt = Lq[:i + 1, :i + 1]
        num = np.abs(np.asarray(K[i, :i + 1]).astype(LD) - Lt @ (Lq[i, :i + 1] * Dq[:i + 1]))
        den = aL[:i + 1, :i + 1] @ (aL[i, :i + 1] * aD[:i + 1])
        worst = max(worst, _ratio(num, den))
    return worst


class SolveMeasure:
    """omega_solve for many (b, x) on one (K, L, D): the conversions are made once."""

    def __init__(self, K, L, D):
        self.K = np.asarray(K).astype(LD)
        self.aL = np.abs(_unit_lower(L))
        self.aD = np.abs(np.asarray(D).astype(LD))

    def __call__(self, b, x):
        b, x = np.atleast_2d(b), np.atleast_2d(x)
        worst = 0.0
        for br, xr in zip(b, x):
            if not np.isfinite(xr).all():
                return float("inf")
            xq = xr.astype(LD)
            num = np.abs(br.astype(LD) - self.K @ xq)
            den = self.aL @ (self.aD * (self.aL.T @ np.abs(xq)))
            worst = max(worst, _ratio(num, den))
        return worst


def omega_solve(K, L, D, b, x):
    return SolveMeasure(K, L, D)(b, x)


def newton_rows(q, slots=BACKSUB_ROWS, eq_none=False):
    """Indices (Newton order) of the block rows `slots` of nc.full_jacobian (absent slots dropped)."""
    order, sz, off, L = nc.offsets(q, eq_none)
    return np.concatenate([np.arange(off[s], off[s] + sz[s]) for s in order if s in slots])


def omega_rows(J, d, r, rows):
    """max over the rows `rows` of |J d + r|_i / (|J||d| + |r|)_i."""
    if not np.isfinite(d).all():
        return float("inf")
    Jq, dq, rq = np.asarray(J[rows]).astype(LD), np.asarray(d).astype(LD), np.asarray(r)[rows].astype(LD)
    return _ratio(np.abs(Jq @ dq + rq), np.abs(Jq) @ np.abs(dq) + np.abs(rq))


def reduced(q, d, eq_none=False):
    """(dx, dlambda_A, dlambda_C) of a full direction: the unknowns of the augmented system, in its order."""
    parts = nc.split(q, np.asarray(d), eq_none)
    return np.concatenate([parts[s] for s in REDUCED_SLOTS if s in parts])


def newton_restated(q, v, r, L, D, rowwise=False):
    """The Newton direction of one residual row by the reference's own formulas in numpy (augmented rhs and
    delta_definitions in the order of csrc/newton.hip rhs_elem / backsub_elem; SlackedSlacks, both bounds,
    Regularization), the augmented system solved by oracle.solve_ldlt with the factor (L, D).  rowwise=True: a
    slack / dual pair slack first, each from its own row (dg = ds - r_lg, dl_g = -(G^-1 (r_g + L_g dg))), as
    backsub_elem takes a caller's residual rows; False: the reference's order, dual first, as the step does."""
    V, R = nc.split(q, np.asarray(v), False), nc.split(q, np.asarray(r), False)
    g, h, y, z = V["g"], V["h"], V["y"], V["z"]
    lg, lh, ly, lz = V["lambda_g"], V["lambda_h"], V["lambda_y"], V["lambda_z"]
    tz = 1.0 / z * (R["z"] + (-(lz * R["lambda_z"])))
    ty = 1.0 / y * (R["y"] + (-(ly * R["lambda_y"])))
    th = 1.0 / h * (R["h"] + (-(lh * R["lambda_h"])))
    tg = 1.0 / g * (R["g"] + (-(lg * R["lambda_g"])))
    dsi = 1.0 / (1.0 / g * lg + 1.0 / h * lh)
    b = np.concatenate([(tz + (-R["x"])) + (-ty), dsi * ((th + (-R["s"])) + (-tg)) + (-R["lambda_A"]),
                        nc.DELTA * R["p"] + (-R["lambda_C"])])
    x = oracle.solve_ldlt(L, D, b)
    n, m = q["n"], q["m"]
    d = dict(x=x[:n], lambda_A=x[n:n + m], lambda_C=x[n + m:])
    d["lambda_y"] = -((1.0 / y * ly) * ((d["x"] + 1.0 / ly * R["y"]) + (-R["lambda_y"])))
    d["y"] = -(1.0 / ly * (R["y"] + y * d["lambda_y"]))
    d["lambda_z"] = -((1.0 / z * lz) * ((1.0 / lz * R["z"] + (-R["lambda_z"])) + (-d["x"])))
    d["z"] = -(1.0 / lz * (R["z"] + z * d["lambda_z"]))
    d["s"] = dsi * (((d["lambda_A"] + th) + (-R["s"])) + (-tg))
    d["lambda_g"] = -((1.0 / g * lg) * ((d["s"] + 1.0 / lg * R["g"]) + (-R["lambda_g"])))
    d["g"] = -(1.0 / lg * (R["g"] + g * d["lambda_g"]))
    d["lambda_h"] = -((1.0 / h * lh) * ((1.0 / lh * R["h"] + (-R["lambda_h"])) + (-d["s"])))
    d["h"] = -(1.0 / lh * (R["h"] + h * d["lambda_h"]))
    d["p"] = -(R["p"] + nc.DELTA * d["lambda_C"])
    if rowwise:
        d["y"] = d["x"] + (-R["lambda_y"])
        d["lambda_y"] = -(1.0 / y * (R["y"] + ly * d["y"]))
        d["z"] = -(d["x"] + R["lambda_z"])
        d["lambda_z"] = -(1.0 / z * (R["z"] + lz * d["z"]))
        d["g"] = d["s"] + (-R["lambda_g"])
        d["lambda_g"] = -(1.0 / g * (R["g"] + lg * d["g"]))
        d["h"] = -(d["s"] + R["lambda_h"])
        d["lambda_h"] = -(1.0 / h * (R["h"] + lh * d["h"]))
    return np.concatenate([d[s] for s in nc.offsets(q, False)[0]])


# ---------------------------------------------------------------------------
# the fp32 factor + fp64 refinement, restated
def ldlt32(K32):
    """Right-looking unpivoted LDL^T in float32 (zero-pivot rule as the reference's): (unit lower L, D)."""
    A = np.array(K32, dtype=np.float32)
    N = A.shape[0]
    D = np.zeros(N, dtype=np.float32)
    for k in range(N):
        d = A[k, k] if A[k, k] != 0 else np.float32(1e-8)
        D[k] = d
        w = A[k + 1:, k].copy()
        l = w * (np.float32(1.0) / d)
        A[k + 1:, k] = l
        A[k + 1:, k + 1:] -= np.outer(l, w)
    L = np.tril(A, -1)
    L[np.arange(N), np.arange(N)] = 1.0
    return L, D


def refine32(K, b, tol=1e-12, max_refine=10):
    """x from the float32 factor of float32(K) with fp64 residuals and corrections: (x, |r|_inf / |b|_inf reached,
    corrections applied).  Substitution in float32, plain loops over numpy rows."""
    L, D = ldlt32(K.astype(np.float32))
    N = len(D)

    def solve(r):
        y = r.astype(np.float32)
        for i in range(1, N):
            y[i] -= L[i, :i] @ y[:i]
        y /= D
        for i in range(N - 2, -1, -1):
            y[i] -= L[i + 1:, i] @ y[i + 1:]
        return y.astype(np.float64)

    x = solve(b)
    for it in range(max_refine + 1):
        r = b - K @ x
        ratio = np.abs(r).max() / np.abs(b).max()
        if ratio <= tol or it == max_refine:
            return x, ratio, it
        x = x + solve(r)
