"""What tests/test_gpu_center.py relies on, checked without a GPU (tests/center_cases.py): the numpy centering
loop reaches the central path from the oracle's converged iterate within the cap of 30 iterations the GPU tests
call with, two starts reach one point, its Jacobian is the derivative of the residuals it is solved against, and
the closed form of the diagonal box QP and its gradients agree with numpy implicit differentiation there."""
import numpy as np
import pytest

import batch_form_cases as fc
import center_cases as cc
import data_vjp_cases as dc
import newton_multi_cases as nc
import oracle

# (shape, seed0, batch) of the GPU tests' reference runs
SHAPES = [(fc.S1, fc.SEED0[fc.S1], 3), (fc.S0, fc.SEED0[fc.S0], 3), (nc.SHAPES[0], nc.SEED, 1),
          ((130, 40, 22), 1100, 3)]


def _forms(shape):
    return [f for f in cc.FORMS if f in fc.SHAPE_FORMS.get(shape, cc.FORMS)]


def test_served_forms_are_the_table_without_the_refused():
    assert cc.FORMS == ("box", "vlo", "vup", "vnone", "alo", "aup", "naive", "none")
    assert all(f in dc.FORM_TABLE for f in cc.FORMS)
    assert cc.MAX_ITER == 30 and cc.TOL == 1e-10


@pytest.mark.parametrize("form", cc.FORMS)
def test_jacobian_is_the_derivative_of_the_residuals(form):
    shape = fc.S1
    q = fc.qp(shape, 7)
    v = np.array(cc.solved(form, shape, 7))
    J = cc.jacobian_form(form, q, v, 1e-2)
    # the residuals are quadratic in v: a complex step differentiates them exactly, column by column
    h = 1e-30
    worst = 0.0
    for k in range(len(v)):
        vc = v.astype(np.complex128)
        vc[k] += 1j * h
        col = np.imag(dc.residuals_form(form, q, vc, 1e-2)) / h
        worst = max(worst, float(np.abs(col - J[:, k]).max()))
    print(f"{form}: |J - complex-step derivative|max {worst:.3e}", flush=True)
    assert worst <= 1e-12 * max(1.0, float(np.abs(J).max()))
    if form in ("box", "none"):
        assert np.array_equal(J, nc.full_jacobian(q, v, eq_none=form == "none"))


@pytest.mark.parametrize("kappa", cc.KAPPAS + (1e-6,))
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "n%d_m%d_p%d" % c[0])
def test_reference_centers_within_the_cap(case, kappa):
    shape, seed0, B = case
    counts = []
    for form in _forms(shape):
        for i in range(B):
            q = fc.qp(shape, seed0 + i)
            z, it, ok, e = cc.center(q, cc.solved(form, shape, seed0 + i), kappa, form=form)
            assert ok and e <= cc.TOL and it <= cc.MAX_ITER - 2, (form, i, it, e)  # (the GPU tests allow count + 2)
            v = dc.form_split(form, *shape, z)
            assert all(np.all(v[s] > 0.0) for s in v if s in oracle.NONNEG), (form, i)
            counts.append(it)
    print(f"{shape} kappa {kappa:g}: iterations {min(counts)}..{max(counts)}", flush=True)


@pytest.mark.parametrize("kappa", cc.KAPPAS)
def test_two_starts_reach_the_same_point(kappa):
    shape, form = fc.S1, "box"
    worst = 0.0
    for seed in (7, 1000, 1001):
        q = fc.qp(shape, seed)
        a, _, ok_a, _ = cc.center(q, cc.solved(form, shape, seed), kappa, form=form)
        # the other start: the first Mehrotra iterate of the oracle with mu <= kappa
        o = fc.FORMS[form].oracle(q)
        for _ in range(100):
            o.iterate()
            if o.mu() <= kappa:
                break
        b, _, ok_b, _ = cc.center(q, o.vars(), kappa, form=form)
        assert ok_a and ok_b
        bound = cc.jinv_norm(form, q, a, kappa) * 2 * cc.TOL
        err = float(np.abs(a - b).max())
        worst = max(worst, err / bound)
        print(f"seed {seed} kappa {kappa:g}: |a - b|inf {err:.3e}, bound {bound:.3e}", flush=True)
    assert worst <= 1.0


@pytest.mark.parametrize("kappa", cc.BOX_KAPPAS + (1e-5,))
def test_box_closed_form_and_its_gradients(kappa):
    q, dq, g = cc.box_case()
    o = oracle.OracleQP(q)
    for _ in range(100):
        conv, rec = o.iterate()
        if rec["converged"]:
            break
    assert rec["converged"]
    z, it, ok, e = cc.center(q, o.vars(), kappa)
    assert ok and it <= cc.MAX_ITER - 2, (it, e)
    x = cc.box_root(dq, q["c"], q["lx"], q["ux"], kappa)
    closed = cc.box_state(x, q["lx"], q["ux"], kappa)
    deriv, D = cc.box_derivatives(dq, x, q["lx"], q["ux"], kappa)
    # bisection leaves x within an ulp of the root, and the function's slope there is D
    assert cc.resid_norm("box", q, closed, kappa) <= 4 * cc.U * float(D.max()) + 64 * cc.U * float(np.abs(closed).max())
    bound = cc.jinv_norm("box", q, z, kappa) * 2 * cc.TOL
    err = float(np.abs(z[:cc.BOX_N] - x).max())
    print(f"box kappa {kappa:g}: {it} iterations, |x - closed form|inf {err:.3e} (bound {bound:.3e})", flush=True)
    assert err <= bound
    got = cc.box_implicit(q, z, g)
    for k in ("c", "Q", "l_x", "u_x"):
        ref = g * deriv[k]
        rel = float(np.abs(got[k] - ref).max()) / max(1.0, float(np.abs(ref).max()))
        print(f"  d/d{k}: numpy implicit vs closed form {rel:.3e}", flush=True)
        # the gradient moves with the point, |dx| <= bound (about 1e-9), by the slope of the closed form in x:
        # d(1 / D) / dx = (2 kappa / gap^3) / D^2 with D >= kappa / gap^2, so at most 2 gap / kappa <= 2 / lambda,
        # of order 1 to 10 for the multipliers of this case
        assert rel <= 1e-8
    for i in cc.BOX_DEGENERATE:
        assert 0.0 < -deriv["c"][i] < 1.0 / dq[i]
