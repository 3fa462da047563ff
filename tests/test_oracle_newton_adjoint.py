"""What tests/test_gpu_newton_adjoint.py relies on, checked without a GPU: the
reference of tests/newton_adjoint_cases.py, numpy.linalg.solve(J^T, -G^T)^T
with the dense Jacobian J of tests/newton_multi_cases.py.  For every shape,
Regularization and None equalities, at the oracle's iterates 0-2:

  * W = reference_adjoint(G) solves its own system: |W J + G|_inf <= 1e-13,
    evaluated in numpy.longdouble (measured <= 1.6e-14);
  * it is the transpose of the forward reference D = nc.reference(R):
    |G D^T - W R^T|_max / |G D^T|_max <= 1e-13 (measured <= 4.6e-15; cond(J)
    <= 120 on all of them; the device bound is 1e-10);

and the header declares both new entry points and ipmz_amd.EXPORTS lists them.
"""
import os
import re

import numpy as np
import pytest

import newton_adjoint_cases as ac
import newton_multi_cases as nc
import oracle

REF_TOL = 1e-13
SHAPES = nc.SHAPES + [nc.BATCHES[1][:3]]
CASES = [(c, e) for c in SHAPES for e in (False, True)]
NAMES = ("ipmz_qp_newton_adjoint_multi", "ipmz_batch_newton_adjoint_multi")


@pytest.mark.parametrize("c,eq_none", CASES, ids=[nc.case_id(c) + ("_none" if e else "_reg") for c, e in CASES])
def test_reference_solves_the_transposed_system(c, eq_none):
    n, m, p = c
    q = nc.qp(n, m, p)
    o = oracle.OracleQP(q, eq_none=eq_none)
    L = nc.offsets(q, eq_none)[3]
    assert L == o.L
    G, R = ac.rows(L)[0], nc.rows(L)[0]
    worst_res = worst_dot = worst_cond = 0.0
    for it in range(3):
        v = o.vars()
        J = nc.full_jacobian(q, v, o.order, eq_none)
        W = ac.reference_adjoint(q, v, G, eq_none)
        D = nc.reference(q, v, R, eq_none)
        res = float(np.abs(ac.ld(W) @ ac.ld(J) + ac.ld(G)).max())
        gd = ac.ld(G) @ ac.ld(D).T
        dot = float(np.abs(gd - ac.ld(W) @ ac.ld(R).T).max() / np.abs(gd).max())
        worst_res, worst_dot = max(worst_res, res), max(worst_dot, dot)
        worst_cond = max(worst_cond, np.linalg.cond(J))
        done, _ = o.iterate()
        assert not done, it
    print(f"{nc.case_id(c)} eq_none={eq_none}: |W J + G|inf {worst_res:.3e}, |G D^T - W R^T| / |G D^T| "
          f"{worst_dot:.3e} (bounds {REF_TOL:.1e}), cond(J) <= {worst_cond:.1f}", flush=True)
    assert worst_res <= REF_TOL and worst_dot <= REF_TOL


def test_cotangent_rows_differ_from_the_residual_rows():
    L = nc.offsets(nc.qp(*nc.SHAPES[1]), False)[3]
    G, R = ac.rows(L, 3), nc.rows(L, 3)
    assert G.shape == R.shape == (3, nc.RHS_MAX, L) and not np.array_equal(G, R)
    assert not G.flags.writeable


def test_bounds_scale_with_what_they_name():
    rng = np.random.default_rng(1)
    D_I, G = rng.standard_normal((5, 5)), rng.standard_normal((3, 5))
    ref = ac.identity_reference(D_I, G)
    assert np.allclose(np.asarray(ref, dtype=np.float64), G @ D_I.T)
    b = ac.identity_bound(D_I, G, ref)
    assert b.shape == (3, 5) and (b >= 2 * nc.TOL * min(1.0, np.abs(G).sum(axis=1).min())).all()
    gap, bound = ac.dot_gap(G, D_I[:4], ref, rng.standard_normal((4, 5)))
    assert gap.shape == bound.shape == (3, 4) and (bound > 0).all()


def test_header_and_binding_name_the_new_calls():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "ipmz.h")) as f:
        txt = f.read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in txt.split("Conventions")[0], "the list at the top of the header"
    import ipmz_amd
    for name in NAMES:
        assert name in ipmz_amd.EXPORTS
    assert hasattr(ipmz_amd.Optimizer, "newton_adjoint") and hasattr(ipmz_amd.Batch, "newton_adjoint_all")
