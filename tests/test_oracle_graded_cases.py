"""What tests/test_gpu_graded_pivots.py relies on, on the CPU: the reference
alone (oracle.ldlt / oracle.solve_ldlt, OracleQP) stays within HALF of every
bound of tests/graded_cases.py on every input the GPU file uses, with no zero
or non-finite pivot; the reference's factor and solve are bitwise equivariant
under the power-of-two scaling; the planted iterates have the magnitudes they
are meant to have; and the reduced part of the oracle's own affine direction
is bitwise its LDL^T solve of rhs(0), which is what the GPU file's check of
row 0 of a Newton solve assumes.

It also records a negative result, so that nobody adds the missing check
later: on the block rows x, lambda_A and s of the full Newton system the
reference's own componentwise residual is 1e5 u and more at a planted iterate
(test_reduced_rows_have_no_componentwise_bound) -- the augmented solve is
backward stable with respect to K, not with respect to those rows of J, whose
entries the elimination multiplied by 1e9 -- so no forward or componentwise
bound exists there and the GPU file asserts none.

Every test prints its figures in units of u = 2^-53 before asserting.
"""
import numpy as np
import pytest

import batch_kkt_cases as kc
import graded_cases as gc
import newton_multi_cases as nc
import oracle
import pivot_cases as pc

U = gc.U


def _factor(K):
    L, D = oracle.ldlt(K)
    assert np.isfinite(L).all() and np.isfinite(D).all()
    assert (D != 0).all() and not (D == 1e-8).any()  # no pivot fell under the zero rule
    return L, D


# 1, 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("N", sorted({c[0] for c in gc.FACTOR_CONFIGS}))
def test_graded_qd_reference_within_half_the_bounds(N):
    """Graded pc.qd, span 33: omega_factor and omega_solve of the reference are the unscaled matrix's own figures
    (the reference is bitwise equivariant) and at most half the bounds.  Recorded: 16.9 u / 22.9 u / 34.2 u at
    N = 200 / 300 / 700 (at most 15 % of (N + 1) u), omega_solve 5.7 u / 6.3 u / 11.3 u over 17 right-hand sides."""
    K0, K, s, B0 = gc.qd_pair(N)
    assert np.array_equal(K / s[:, None] / s[None, :], K0)  # the scaling is exact
    d = np.abs(np.diag(K))
    assert d.min() < 1e-17 and d.max() > 1e17, (d.min(), d.max())
    L0, D0 = _factor(K0)
    L, D = _factor(K)
    assert np.array_equal(L, s[:, None] * L0 / s[None, :]) and np.array_equal(D, s * D0 * s)
    w0, w = gc.omega_factor(K0, L0, D0), gc.omega_factor(K, L, D)
    sm0, sm = gc.SolveMeasure(K0, L0, D0), gc.SolveMeasure(K, L, D)
    ws0 = ws = 0.0
    for b0 in B0:
        x0, x = oracle.solve_ldlt(L0, D0, b0), oracle.solve_ldlt(L, D, s * b0)
        assert np.array_equal(x, x0 / s)
        ws0, ws = max(ws0, sm0(b0, x0)), max(ws, sm(s * b0, x))
    print(f"N {N}: omega_factor {w / U:.1f} u (unscaled {w0 / U:.1f} u, bound {gc.factor_bound(N) / U:.0f} u), "
          f"omega_solve {ws / U:.1f} u (unscaled {ws0 / U:.1f} u, bound {gc.solve_bound(N) / U:.0f} u)", flush=True)
    assert w == w0 and ws == ws0
    assert w <= gc.factor_bound(N) / 2 and ws <= gc.solve_bound(N) / 2
    assert w <= 0.15 * (N + 1) * U


def test_large_orders_reference():
    """N = 2560: the sampled rows hold the edge positions and both ends of |D|, and the reference's omega_factor
    on them is within half the bound.  (N = 4100 is compared for equivariance only.)"""
    N, blocking = gc.LARGE_OMEGA
    K0, K, s, _ = gc.qd_pair(N)
    L0, D0 = _factor(K0)
    D = s * D0 * s
    nbo, nbi = pc.resolve_blocking(N, blocking)
    rows = gc.sample_rows(N, D, nbo, nbi)
    o = np.argsort(np.abs(D), kind="stable")
    assert set(pc.positions(N, nbo, nbi)) <= set(rows) and set(o[:16]) <= set(rows) and set(o[-16:]) <= set(rows)
    assert len(rows) <= 11 + 48
    w = gc.omega_factor(K, s[:, None] * L0 / s[None, :], D, rows)
    print(f"N {N}: omega_factor on {len(rows)} rows {w / U:.1f} u (bound {gc.factor_bound(N) / U:.0f} u)", flush=True)
    assert w <= gc.factor_bound(N) / 2


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,mp", gc.NORMAL_CASES)
def test_graded_aug_reference(n, mp):
    """Graded pc.aug: the (2,2) block stays diagonal, and the reference's factor and solve are equivariant."""
    K0, K, s, B0 = gc.aug_pair(n, mp)
    blk = K[n:, n:]
    assert np.array_equal(blk, np.diag(np.diag(blk))) and (np.diag(blk) < 0).all()
    L0, D0 = _factor(K0)
    L, D = _factor(K)
    assert np.array_equal(D, s * D0 * s)
    assert (D[:n] > 0).all() and (D[n:] < 0).all()
    for b0 in B0[:3]:
        assert np.array_equal(oracle.solve_ldlt(L, D, s * b0), oracle.solve_ldlt(L0, D0, b0) / s)


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", gc.MIXED_ORDERS)
def test_fp32_restatement_at_span_20(N):
    """A float32 right-looking LDL^T of float32(K) with fp64 residuals and corrections reaches 1e-12 within 10
    corrections at span 20, nothing in it leaves fp32's range, and its factor is within half of 2 (N + 1) u32.
    Recorded: 28.9 u32 and 35.2 u32 (bounds 602 and 1402 u32); ratio 1.2e-13 and 7.3e-13 after 1 correction each."""
    K0, K, s, B0 = gc.qd_pair(N, gc.SPAN32)
    K32 = K.astype(np.float32)
    assert np.isfinite(K32).all() and np.array_equal(K32 != 0, K != 0)  # no overflow, no flush to zero
    L32, D32 = gc.ldlt32(K32)
    assert np.isfinite(L32).all() and np.isfinite(D32).all() and (D32 != 0).all()
    assert np.abs(D32).min() > 1e-30 and np.abs(D32).max() < 1e30
    w = gc.omega_factor(K32, L32, D32)
    x, ratio, iters = gc.refine32(K, s * B0[0])
    print(f"N {N}: float32 omega_factor {w / gc.U32:.1f} u32 (bound {gc.factor_bound(N, gc.U32) / gc.U32:.0f} u32); "
          f"ratio {ratio:.2e} after {iters} corrections", flush=True)
    assert w <= gc.factor_bound(N, gc.U32) / 2
    assert ratio <= 1e-12 and iters <= 10


# 5, 6, 7 ---------------------------------------------------------------------
PLANTED = sorted({c[:3] + (c[4],) for c in kc.SHAPES} | {c[:3] + (gc.QP_SEED,) for c in gc.ASSEMBLY_CASES})


@pytest.mark.parametrize("n,m,p,seed0", PLANTED, ids=lambda v: str(v))
def test_planted_iterates_reference(n, m, p, seed0):
    """The planted iterate of the first QP of every batch the GPU file uses: mu about 2e-9, KKT diagonals spread
    over 1e-9 .. 1e9, no zero-rule pivot, omega_factor and omega_solve of K d = rhs(0) within half the bounds.
    Recorded (plant seed 3): (48,16,8) 7.8 u / 4.0 u; (256,48,17) seed 1000 29.1 u / 21.2 u; (640,160,32) 48.4 u /
    31.5 u; (800,200,40) 52.1 u / 41.6 u at the most, against bounds of 2082 u / 3121 u."""
    o, v, K, L, D = gc.planted(n, m, p, seed0, gc.PLANT_SEED)
    N = n + m + p
    assert 5e-10 < o.mu() < 1e-8, o.mu()
    d = np.abs(np.diag(K)[:n + m])
    assert d.max() > 1e7 and (m == 0 or d.min() < 1e-7), (d.min(), d.max())  # (the small ones: the lambda_A rows)
    assert np.isfinite(D).all() and (D != 0).all() and not (D == 1e-8).any()
    w = gc.omega_factor(K, L, D)
    b = o.rhs(0.0)
    x = oracle.solve_ldlt(L, D, b)
    ws = gc.omega_solve(K, L, D, b, x)
    print(f"({n},{m},{p}) N {N}: mu {o.mu():.2e}, |K_ii| in [{d.min():.1e}, {d.max():.1e}], omega_factor {w / U:.1f} u "
          f"(bound {gc.factor_bound(N) / U:.0f} u), omega_solve {ws / U:.1f} u (bound {gc.solve_bound(N) / U:.0f} u)",
          flush=True)
    assert w <= gc.factor_bound(N) / 2 and ws <= gc.solve_bound(N) / 2


@pytest.mark.parametrize("c", gc.NEWTON_CASES, ids=nc.case_id)
@pytest.mark.parametrize("plant_seed", (3, 4))
def test_affine_direction_is_the_solve_of_rhs0(c, plant_seed):
    """The sign and the bitwise assumption of the GPU file's row-0 check: the reduced part (dx, dlambda_A,
    dlambda_C) of the oracle's own daff() at a planted iterate IS oracle.solve_ldlt of rhs(0) with the factor of
    kkt(), bit for bit; and omega_rows of daff() on the back-substituted block rows is within half of 16 u.
    Recorded: omega_rows <= 2.1 u over plant seeds 3 and 4."""
    n, m, p = c[:3]
    q = kc.qp(n, m, p, gc.QP_SEED)
    o = oracle.OracleQP(q)
    v = gc.plant(o, plant_seed)
    o.set_vars(v)
    K, b = o.kkt(), o.rhs(0.0)
    L, D = oracle.ldlt(K)
    x = oracle.solve_ldlt(L, D, b)
    J = nc.full_jacobian(q, v)
    r = nc.residuals_numpy(q, v)
    o.iterate()
    d = o.daff()
    assert np.array_equal(gc.reduced(q, d), x)
    w = gc.omega_rows(J, d, r, gc.newton_rows(q))
    print(f"{nc.case_id(c)} plant seed {plant_seed}: omega_rows of the oracle's daff {w / U:.1f} u (bound 16 u)",
          flush=True)
    assert w <= gc.ROWS_BOUND / 2


@pytest.mark.parametrize("c", gc.NEWTON_CASES, ids=nc.case_id)
def test_random_residual_rows_by_the_reference_formulas(c):
    """Rows 1 and 2 of the GPU file's Newton solve are random (nc.rows), and the oracle only steps with its own
    residuals, so the formulas are restated in numpy (gc.newton_restated; on the residual row the restatement
    agrees with the oracle's daff() to rounding).  In the reference's order of a slack / dual pair, dual first,
    the rows p, g, h, y, z are within half of 16 u on every row, but the rows lambda_g, lambda_h, lambda_y,
    lambda_z are NOT for a random row (asserted > 1000 u, so that the order is not taken back by mistake):
    dlambda_g = -(G^-1 Lambda_g)((ds + Lambda_g^-1 r_g) - r_lg) adds Lambda_g^-1 r_g, about 1e9 |r_g| where the
    dual is 1e-9, to ds and r_lg of order one, and dg comes out of the cancellation r_g + G dlambda_g, so row
    lambda_g (dg - ds + r_lg) is left with 1e9 u of its own terms.  With the iterate's own residual r_g = g
    lambda_g that term is g, and the row holds (the test above).  Slack first, each of the pair from its own row
    (rowwise=True: what the device does with a caller's rows), every back-substituted row is within half of 16 u
    on every row, and the direction is the same to the forward accuracy the old order has.
    Recorded: reference's order: slack rows <= 1.2 u, dual rows 3.1e8 u .. 1.3e9 u on rows 1 and 2; row by row:
    every back-substituted row <= 1.2 u, and 8.2e-15 at the most from the reference's order."""
    n, m, p = c[:3]
    q = kc.qp(n, m, p, gc.QP_SEED)
    o, v, K, L, D = gc.planted(n, m, p, gc.QP_SEED, gc.PLANT_SEED)
    J, r0 = nc.full_jacobian(q, v), nc.residuals_numpy(q, v)
    fresh = oracle.OracleQP(q)
    fresh.set_vars(v)
    fresh.iterate()
    d0 = gc.newton_restated(q, v, r0, L, D)
    e = nc.row_err(d0[None], fresh.daff()[None])
    print(f"{nc.case_id(c)}: restated daff vs the oracle's {e:.2e}", flush=True)
    assert e <= 1e-10
    slack, dual = gc.newton_rows(q, gc.SLACK_ROWS), gc.newton_rows(q, gc.DUAL_ROWS)
    for k in (1, 2):
        r = np.array(nc.rows(len(v))[0, k - 1])
        d = gc.newton_restated(q, v, r, L, D)
        ws, wd = gc.omega_rows(J, d, r, slack), gc.omega_rows(J, d, r, dual)
        print(f"{nc.case_id(c)} row {k}: slack rows {ws / U:.2f} u (bound 16 u), dual rows {wd / U:.3g} u", flush=True)
        assert ws <= gc.ROWS_BOUND / 2
        assert wd > 1000 * U
    both = gc.newton_rows(q)
    for k in (0, 1, 2):
        r = r0 if k == 0 else np.array(nc.rows(len(v))[0, k - 1])
        d, dw = gc.newton_restated(q, v, r, L, D), gc.newton_restated(q, v, r, L, D, rowwise=True)
        w, e = gc.omega_rows(J, dw, r, both), nc.row_err(dw[None], d[None])
        print(f"{nc.case_id(c)} row {k}, slack first: back-substituted rows {w / U:.2f} u (bound 16 u); against the "
              f"reference's order {e:.2e}", flush=True)
        assert w <= gc.ROWS_BOUND / 2
        assert e <= 1e-10


@pytest.mark.parametrize("c", gc.NEWTON_CASES, ids=nc.case_id)
def test_reduced_rows_have_no_componentwise_bound(c):
    """The negative result: on the block rows x, lambda_A, s the oracle's own daff() leaves a componentwise
    residual of 1e5 u and more.  Asserted as such (> 1000 u), so that a check of those rows is not added by
    mistake.  Recorded: 3.0e5 u and 1.1e8 u."""
    n, m, p = c[:3]
    q = kc.qp(n, m, p, gc.QP_SEED)
    o = oracle.OracleQP(q)
    v = gc.plant(o, gc.PLANT_SEED)
    o.set_vars(v)
    J, r = nc.full_jacobian(q, v), nc.residuals_numpy(q, v)
    o.iterate()
    w = gc.omega_rows(J, o.daff(), r, gc.newton_rows(q, gc.UNBOUNDED_ROWS))
    print(f"{nc.case_id(c)}: omega_rows of the oracle's daff on the rows x, lambda_A, s: {w / U:.3g} u", flush=True)
    assert w > 1000 * U
