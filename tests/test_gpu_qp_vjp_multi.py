"""ipmz_amd.layer.solution_vjp and solution_jacobian: cotangents of the solution (or of the whole Newton state), ncot
rows per QP -> the adjoint Newton solve of all rows from one factor (ipmz_*_newton_adjoint_multi) -> their
contraction with d r / d data (ipmz_batch_data_vjp_multi).

References: numpy implicit differentiation at the device's own converged iterate (numpy.linalg.solve(J^T, -g) on
nc.full_jacobian, pushed through dc.reference) under the per-element bound of
tests/test_gpu_qp_layer.py::test_backward_vs_numpy_implicit_differentiation; the forward-mode chain solution_jvp on
the same device under the bound of tests/test_gpu_qp_jvp.py::test_forward_against_reverse_on_the_device; and the
closed form d x* / d c = -Q^{-1} of an interior box QP, where the distance is the IPM's stopping error and the CPU
oracle's converged iterate sets the scale (tests/test_gpu_qp_jvp.py::test_closed_form).  Every test prints its worst
figure before it asserts.
"""
import numpy as np
import pytest

import data_jvp_cases as jc
import data_vjp_cases as dc
import newton_multi_cases as nc
import oracle
from test_gpu_qp_jvp import _interior_box_qp

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")
layer = pytest.importorskip("ipmz_amd.layer")

SEED0 = 1000
B, NCOT = 3, 3
CASES = [(c, e) for c in nc.SHAPES[:2] for e in (False, True)]
IDS = [f"{nc.case_id(c)}-{'none' if e else 'reg'}" for c, e in CASES]


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _dev(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _solved(c, eq_none, ctx):
    """The converged batch of nc.qp(n, m, p, SEED0 + i), its QPs and its iterates."""
    n, m, p = c
    qs = [nc.qp(n, m, p, SEED0 + i) for i in range(B)]
    bt = I.Batch(n, m, p, B, ctx, equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION)
    bt.generate(SEED0)
    its, converged = bt.solve_all(100)
    assert converged == B
    return bt, qs, [bt.state(i) for i in range(B)]


def _implicit(q, v, g, eq_none):
    """numpy implicit differentiation at the iterate v for a cotangent g of the solution (n entries) or of the whole
    Newton state: J^T w = -g, then the numpy reference's contraction."""
    J = nc.full_jacobian(q, v, eq_none=eq_none)
    full = np.zeros(J.shape[0])
    full[:len(g)] = g
    w = np.linalg.solve(J.T, -full)
    return dc.reference(q, v, w, eq_none), w


def _carried(w, v):
    """test_backward_vs_numpy_implicit_differentiation's term: the adjoint solve to the bar, carried through the
    products with the iterate."""
    return 2 * nc.TOL * max(1.0, np.abs(w).max()) * max(1.0, np.abs(v).max())


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("c,eq_none", CASES, ids=IDS)
def test_solution_vjp_vs_numpy_implicit_differentiation(ctx, c, eq_none):
    n, m, p = c
    bt, qs, V = _solved(c, eq_none, ctx)
    L = bt.state_len
    rng = np.random.default_rng(177)
    worst = {}
    for width in (n, L):  # cotangents of x*, and of the whole Newton state (non-zero in the dual slots)
        G = rng.standard_normal((B, NCOT, width))
        grads, W = layer.solution_vjp(bt, _dev(G))
        assert W.shape == (B, NCOT, L)
        got = {k: _host(t) for k, t in grads.items()}
        assert set(got) == set(dc.present(n, m, p))
        w_ = 0.0
        for q in range(B):
            for r in range(NCOT):
                ref, w = _implicit(qs[q], V[q], G[q, r], eq_none)
                carried = _carried(w, V[q])
                for k, rk in ref.items():
                    bound = nc.TOL * max(1.0, np.abs(rk).max()) + carried
                    err = np.abs(got[k][q, r] - rk).max()
                    w_ = max(w_, (np.inf if np.isnan(err) else err) / bound)
        worst[width] = w_
    print(f"{nc.case_id(c)} eq_none={eq_none}: worst |grad - numpy implicit| / bound, G of width n {worst[n]:.3e}, "
          f"of width state_len {worst[L]:.3e}", flush=True)
    assert max(worst.values()) <= 1.0


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("c,eq_none", CASES, ids=IDS)
def test_forward_against_reverse(ctx, c, eq_none):
    """<G[q, r], dx[q, t]> of solution_jvp = sum_k <grads[k][q, r], D_k[q, t]> for all (r, t), under the bound of
    test_forward_against_reverse_on_the_device: nc.TOL |G|_1 max(1, |dx|inf) for the forward side plus sum_k |D_k|_1
    times the per-element bound of test 7."""
    n, m, p = c
    ntan = 3
    bt, qs, V = _solved(c, eq_none, ctx)
    G = np.random.default_rng(179).standard_normal((B, NCOT, n))
    grads = {k: _host(t) for k, t in layer.solution_vjp(bt, _dev(G))[0].items()}
    Dh = jc.tangents(n, m, p, ntan, B)
    dx = _host(layer.solution_jvp(bt, **{k: _dev(a) for k, a in Dh.items()})[0])
    worst = 0.0
    for q in range(B):
        for r in range(NCOT):
            ref, w = _implicit(qs[q], V[q], G[q, r], eq_none)
            carried = _carried(w, V[q])
            for t in range(ntan):
                lhs = np.sum(dc.ld(G[q, r]) * dc.ld(dx[q, t]))
                rhs = sum(np.sum(dc.ld(grads[k][q, r]) * dc.ld(Dh[k][q, t])) for k in Dh)
                bound = nc.TOL * np.abs(G[q, r]).sum() * max(1.0, np.abs(dx[q, t]).max()) + \
                    sum(np.abs(Dh[k][q, t]).sum() * (nc.TOL * max(1.0, np.abs(ref[k]).max()) + carried) for k in Dh)
                worst = max(worst, float(abs(lhs - rhs)) / bound)
    print(f"{nc.case_id(c)} eq_none={eq_none}: worst |<G, dx> - sum <grad, D>| / bound over (QP, r, t) {worst:.3e}",
          flush=True)
    assert worst <= 1.0


# 9 ---------------------------------------------------------------------------
@pytest.mark.parametrize("c,eq_none", CASES, ids=IDS)
def test_solution_jacobian_against_solution_jvp(ctx, c, eq_none):
    """Along the n unit tangents of c: J["c"][q, i, j] = dx[q, t = j, i], within nc.TOL max(1, |J|inf) plus the
    carried term of test 8 (w: numpy's adjoint rows of the n unit cotangents)."""
    n, m, p = c
    bt, qs, V = _solved(c, eq_none, ctx)
    grads, W = layer.solution_jacobian(bt)
    J = _host(grads["c"])
    assert J.shape == (B, n, n) and W.shape == (B, n, bt.state_len)
    dx = _host(layer.solution_jvp(bt, c=_dev(np.tile(np.eye(n), (B, 1, 1))))[0])
    worst = 0.0
    for q in range(B):
        Jn = nc.full_jacobian(qs[q], V[q], eq_none=eq_none)
        E = np.zeros((Jn.shape[0], n))
        E[:n] = np.eye(n)
        w = np.linalg.solve(Jn.T, -E)
        bound = nc.TOL * max(1.0, np.abs(J[q]).max()) + _carried(w, V[q])
        worst = max(worst, float(np.abs(J[q] - dx[q].T).max()) / bound)
    print(f"{nc.case_id(c)} eq_none={eq_none}: worst |J[c][q, i, j] - dx[q, j, i]| / bound {worst:.3e}", flush=True)
    assert worst <= 1.0


def test_solution_jacobian_closed_form(ctx):
    """The interior box QP: d x* / d c = -Q^{-1}.  The distance is the IPM's stopping error: the same Jacobian from
    the CPU oracle's converged iterate sets the scale, as in test_gpu_qp_jvp.py::test_closed_form."""
    q, xs = _interior_box_qp()
    n = q["n"]
    cf = -np.linalg.inv(q["Q"])  # [i, j] = d x_i / d c_j; row t = j of the tangents' dx is column j
    o = oracle.OracleQP(q)
    for _ in range(100):
        conv, rec = o.iterate()
        if rec["converged"]:
            break
    assert rec["converged"]
    v = o.vars()
    D = dict(c=np.eye(n)[None])
    Rc = np.stack([jc.jvp_reference("box", q, v, jc.one(D, t, 0)) for t in range(n)])
    e_cpu = float(np.abs(nc.reference(q, v, Rc)[:, :n].T - cf).max())
    s = I.Optimizer(n, 0, 0, ctx)
    layer.solve_qp(s, **{k: _dev(q[dc.KEYS[k]]) for k in ("Q", "c", "l_x", "u_x")})
    grads, W = layer.solution_jacobian(s)
    J = _host(grads["c"])[0]
    dx = _host(layer.solution_jvp(s, c=_dev(np.eye(n)[None]))[0])[0]
    e_gpu = float(np.abs(J - cf).max())
    e_fr = float(np.abs(J - dx.T).max())
    allowed = 10.0 * e_cpu + nc.TOL * max(1.0, float(np.abs(cf).max()))
    Jn = nc.full_jacobian(q, s.vars())
    E = np.zeros((Jn.shape[0], n))
    E[:n] = np.eye(n)
    bound_fr = nc.TOL * max(1.0, np.abs(J).max()) + _carried(np.linalg.solve(Jn.T, -E), s.vars())
    print(f"interior d x* / d c: GPU Jacobian vs -Q^-1 {e_gpu:.3e}, CPU oracle vs -Q^-1 {e_cpu:.3e}, allowed "
          f"{allowed:.3e}; vs solution_jvp {e_fr:.3e} (bound {bound_fr:.3e})", flush=True)
    assert e_gpu <= allowed
    assert e_fr <= bound_fr


# 10 --------------------------------------------------------------------------
def test_guards(ctx):
    c, eq_none = nc.SHAPES[1], False
    n, m, p = c
    bt, qs, V = _solved(c, eq_none, ctx)
    L = bt.state_len
    gen = bt._generation
    G = _dev(np.random.default_rng(181).standard_normal((B, NCOT, n)))
    names = dc.present(n, m, p)
    per = {k: _host(t) for k, t in layer.solution_vjp(bt, G)[0].items()}
    sh = {k: _host(t) for k, t in layer.solution_vjp(bt, G, shared=names)[0].items()}
    some = layer.solution_vjp(bt, G, only=["c", "A_eq"], shared=["A_eq"])[0]
    assert set(some) == {"c", "A_eq"} and some["c"].shape == (B, NCOT, n) and some["A_eq"].shape == (NCOT, p, n)
    assert bt._generation == gen, "the generation counter does not move"
    for i in range(B):
        assert np.array_equal(bt.state(i), V[i]), "the iterate does not move"
    worst = 0.0
    for k in names:
        assert sh[k].shape == per[k].shape[1:], k
        for r in range(NCOT):
            want, bound = dc.shared_reference(per[k][:, r])
            worst = max(worst, float(np.abs(sh[k][r] - want).max()) / bound)
    print(f"shared names: worst |shared - sum over the batch of per-QP| / bound {worst:.3e}", flush=True)
    assert worst <= 1.0
    sym = _host(layer.solution_vjp(bt, G, only=["Q"], symmetrize=True)[0]["Q"])
    assert np.array_equal(sym, 0.5 * (per["Q"] + per["Q"].transpose(0, 1, 3, 2)))
    for bad in (G[:, 0], G[:, :, :n - 1], G[:1], G.float(), _dev(np.zeros((B, NCOT, L + 1))), _host(G)):
        with pytest.raises(ValueError):
            layer.solution_vjp(bt, bad)
    with pytest.raises(ValueError):
        layer.solution_vjp(bt, G, shared=["nope"])
    empty, W0 = layer.solution_vjp(bt, G[:, :0])
    assert W0.shape == (B, 0, L) and empty["c"].shape == (B, 0, n)
    assert bt._generation == gen
