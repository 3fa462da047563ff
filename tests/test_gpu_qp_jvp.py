"""ipmz_amd.layer.solution_jvp and solve_qp under torch.autograd.forward_ad: data tangents -> R
(ipmz_batch_data_jvp) -> the Newton solve of all rows (ipmz_*_newton_solve_multi) -> the tangent of the solution.

References: numpy.linalg.solve on nc.full_jacobian at the device's own iterate with the device's own R (no
convergence error, no conditioning term); the reverse-mode chain of solve_qp on the same device; and the closed form
of an interior box QP, where the distance is the IPM's stopping error and the CPU oracle's converged iterate sets the
scale.  Every test prints its worst figure before it asserts.
"""
import types

import numpy as np
import pytest

import data_jvp_cases as jc
import data_vjp_cases as dc
import newton_multi_cases as nc
import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")
layer = pytest.importorskip("ipmz_amd.layer")

SEED0 = 1000


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _dev(a, grad=False):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda().requires_grad_(grad)
    torch.cuda.synchronize()
    return t


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _stack(qs):
    return {k: np.stack([q[dc.KEYS[k]] for q in qs]) for k in dc.present(qs[0]["n"], qs[0]["m"], qs[0]["p"])}


def _kw(eq_none):
    return dict(equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION)


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
@pytest.mark.parametrize("c", nc.SHAPES[:2], ids=nc.case_id)
def test_solution_jvp_at_the_converged_iterate(ctx, c, eq_none):
    n, m, p = c
    B, ntan = 3, 3
    qs = [nc.qp(n, m, p, SEED0 + i) for i in range(B)]
    bt = I.Batch(n, m, p, B, ctx, **_kw(eq_none))
    bt.generate(SEED0)
    its, converged = bt.solve_all(100)
    assert converged == B
    gen = bt._generation
    L = bt.state_len
    worst = 0.0
    for shared in (False, True):
        D = {k: _dev(a) for k, a in jc.tangents(n, m, p, ntan, None if shared else B).items()}
        R = _host(bt.data_jvp_tensors(D))[:, :, :L]
        before = [bt.state(i) for i in range(B)]
        dx, dz = layer.solution_jvp(bt, **D)
        assert dx.shape == (B, ntan, n) and dz.shape == (B, ntan, L) and dx.data_ptr() == dz.data_ptr()
        dzh = _host(dz)
        for i in range(B):
            assert np.array_equal(bt.state(i), before[i]), "the iterate does not move"
            ref = nc.reference(qs[i], before[i], R[i], eq_none)
            worst = max(worst, nc.row_err(dzh[i], ref))
    assert bt._generation == gen, "the generation counter does not move"
    print(f"{nc.case_id(c)} eq_none={eq_none}: worst |dz - numpy solve| per row {worst:.3e} (bound {nc.TOL:.1e})", flush=True)
    assert worst <= nc.TOL


# 9 ---------------------------------------------------------------------------
def _implicit(q, v, g_x, eq_none=False):
    """numpy implicit differentiation at the iterate v (tests/test_gpu_qp_layer.py): J^T w = -g, then the numpy
    reference's contraction."""
    J = nc.full_jacobian(q, v, eq_none=eq_none)
    g = np.zeros(J.shape[0])
    g[:q["n"]] = g_x
    w = np.linalg.solve(J.T, -g)
    return dc.reference(q, v, w, eq_none), w


@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
@pytest.mark.parametrize("c", nc.SHAPES[:2], ids=nc.case_id)
def test_forward_against_reverse_on_the_device(ctx, c, eq_none):
    """<G, dx> of solution_jvp = sum <.grad of solve_qp(...).backward, D>, per QP and tangent.  The bound is assembled
    from the existing bars: nc.TOL |G|_1 max(1, |dx|inf) for the forward side (each dx element to the Newton-direction
    bar) plus sum_k |D_k|_1 times the per-element bound of test_backward_vs_numpy_implicit_differentiation."""
    n, m, p = c
    B, ntan = 3, 3
    qs = [nc.qp(n, m, p, SEED0 + i) for i in range(B)]
    bt = I.Batch(n, m, p, B, ctx, **_kw(eq_none))
    leaves = {k: _dev(a, True) for k, a in _stack(qs).items()}
    x = layer.solve_qp(bt, **leaves)
    G = np.random.default_rng(79).standard_normal((B, n))
    (torch.from_numpy(G).cuda() * x).sum().backward()
    torch.cuda.synchronize()
    Dh = jc.tangents(n, m, p, ntan, B)
    dx = _host(layer.solution_jvp(bt, **{k: _dev(a) for k, a in Dh.items()})[0])
    worst = 0.0
    for i in range(B):
        v = bt.state(i)
        ref, w = _implicit(qs[i], v, G[i], eq_none)
        carried = 2 * nc.TOL * max(1.0, np.abs(w).max()) * max(1.0, np.abs(v).max())
        for t in range(ntan):
            lhs = np.sum(dc.ld(G[i]) * dc.ld(dx[i, t]))
            rhs = sum(np.sum(dc.ld(leaves[k].grad[i].cpu().numpy()) * dc.ld(Dh[k][i, t])) for k in Dh)
            bound = nc.TOL * np.abs(G[i]).sum() * max(1.0, np.abs(dx[i, t]).max()) + \
                sum(np.abs(Dh[k][i, t]).sum() * (nc.TOL * max(1.0, np.abs(ref[k]).max()) + carried) for k in Dh)
            worst = max(worst, float(abs(lhs - rhs)) / bound)
    print(f"{nc.case_id(c)} eq_none={eq_none}: worst |<G, dx> - sum <grad, D>| / bound {worst:.3e}", flush=True)
    assert worst <= 1.0


# 10 --------------------------------------------------------------------------
def _interior_box_qp():
    """The "interior" box QP of tests/test_gpu_qp_layer.py: Q SPD with condition <= 10, the minimiser -Q^{-1} c inside
    the box by at least 9."""
    n = 12
    rng = np.random.default_rng(5)
    rng.standard_normal(n)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q = (U * np.linspace(1.0, 10.0, n)) @ U.T
    Q = 0.5 * (Q + Q.T)
    xs = rng.uniform(-1.0, 1.0, n)
    q = dict(n=n, m=0, p=0, Q=Q, c=-Q @ xs, A=np.zeros((0, n)), lA=np.zeros(0), uA=np.zeros(0), C=np.zeros((0, n)),
             d=np.zeros(0), lx=np.full(n, -10.0), ux=np.full(n, 10.0))
    return q, xs


def test_closed_form(ctx):
    q, xs = _interior_box_qp()
    n, ntan = q["n"], 2
    rng = np.random.default_rng(6)
    D = dict(Q=rng.standard_normal((1, ntan, n, n)), c=rng.standard_normal((1, ntan, n)))
    cf = np.stack([-np.linalg.solve(q["Q"], D["c"][0, t] + D["Q"][0, t] @ xs) for t in range(ntan)])
    o = oracle.OracleQP(q)
    for _ in range(100):
        conv, rec = o.iterate()
        if rec["converged"]:
            break
    assert rec["converged"]
    v = o.vars()
    Rc = np.stack([jc.jvp_reference("box", q, v, jc.one(D, t, 0)) for t in range(ntan)])
    e_cpu = float(np.abs(nc.reference(q, v, Rc)[:, :n] - cf).max())
    s = I.Optimizer(n, 0, 0, ctx)
    x = layer.solve_qp(s, **{k: _dev(q[dc.KEYS[k]]) for k in ("Q", "c", "l_x", "u_x")})
    dx = _host(layer.solution_jvp(s, **{k: _dev(a) for k, a in D.items()})[0])[0]
    e_gpu = float(np.abs(dx - cf).max())
    allowed = 10.0 * e_cpu + nc.TOL * max(1.0, float(np.abs(cf).max()))
    print(f"interior dx: GPU vs closed form {e_gpu:.3e}, CPU oracle vs closed form {e_cpu:.3e}, allowed {allowed:.3e}",
          flush=True)
    assert e_gpu <= allowed


# 11 --------------------------------------------------------------------------
def test_forward_ad(ctx):
    import torch.autograd.forward_ad as fwAD
    n, m, p = nc.SHAPES[1]
    B = 3
    qs = [nc.qp(n, m, p, SEED0 + i) for i in range(B)]
    data = _stack(qs)
    data["Q"] = qs[0]["Q"]  # one Q for every QP: its tangent is a shared tangent
    prim = {k: _dev(a) for k, a in data.items()}
    rng = np.random.default_rng(80)
    tang = {k: _dev(rng.standard_normal(a.shape)) for k, a in data.items() if k in ("Q", "c", "A_ineq", "b_eq")}
    bt = I.Batch(n, m, p, B, ctx)
    with fwAD.dual_level():
        duals = {k: (fwAD.make_dual(t, tang[k]) if k in tang else t) for k, t in prim.items()}
        x = layer.solve_qp(bt, **duals)
        xp, xt = fwAD.unpack_dual(x)
        assert xt is not None and xt.shape == (B, n)
        xt = _host(xt)
    assert np.array_equal(_host(xp), np.stack([bt.state(i)[:n] for i in range(B)]))
    D = {k: (t.unsqueeze(0) if k == "Q" else t.unsqueeze(1)) for k, t in tang.items()}
    dx = _host(layer.solution_jvp(bt, **D)[0])[:, 0]
    assert np.array_equal(xt, dx), "the dual's tangent is solution_jvp's dx"
    print("forward_ad: the dual's tangent is bitwise solution_jvp's, Q's tangent taken as shared", flush=True)
    # a load between forward and jvp: the generation check of backward
    fake = types.SimpleNamespace(solver=bt, generation=bt._generation, shapes={k: tuple(t.shape) for k, t in prim.items()},
                                 shared=("Q",))
    args = [tang.get(k) for k in layer._NAMES]
    assert np.array_equal(_host(layer._SolveQP.jvp(fake, None, None, None, None, *args)), dx)
    bt.load_tensors(c=prim["c"])
    with pytest.raises(I.IpmzError, match="changed between forward and jvp"):
        layer._SolveQP.jvp(fake, None, None, None, None, *args)
