"""ipmz_amd.layer.solve_qp: a batch of QPs as a torch.autograd.Function (forward: load, solve, x; backward: the
adjoint Newton solve and ipmz_batch_data_vjp).

References: numpy implicit differentiation at the device's own converged iterate (numpy.linalg.solve(J^T, -g) with
nc.full_jacobian, pushed through the numpy reference of tests/data_vjp_cases.py) -- no convergence error, both sides
use the same iterate; and closed forms of box-constrained QPs, where the distance is the IPM's stopping error and the
CPU oracle's converged iterate sets the scale.  Every test prints its worst figure before it asserts.
"""
import json
import os

import numpy as np
import pytest

import data_vjp_cases as dc
import newton_multi_cases as nc
import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")
layer = pytest.importorskip("ipmz_amd.layer")

SEED0 = 1000
# when set, test_closed_forms writes its two figures per gradient there (profiles/data_vjp/layer_accuracy.json is
# such a run's file)
ACCURACY_JSON = os.environ.get("IPMZ_LAYER_ACCURACY_JSON")
_accuracy = {}


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _leaf(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda().requires_grad_(True)
    torch.cuda.synchronize()
    return t


def _stack(qs):
    return {k: np.stack([q[dc.KEYS[k]] for q in qs]) for k in dc.present(qs[0]["n"], qs[0]["m"], qs[0]["p"])}


def _implicit(q, v, g_x, eq_none=False):
    """numpy implicit differentiation at the iterate v: J^T w = -g, then the numpy reference's contraction."""
    J = nc.full_jacobian(q, v, eq_none=eq_none)
    g = np.zeros(J.shape[0])
    g[:q["n"]] = g_x
    w = np.linalg.solve(J.T, -g)
    return dc.reference(q, v, w, eq_none), w


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
@pytest.mark.parametrize("c", nc.SHAPES[:2], ids=nc.case_id)
def test_backward_vs_numpy_implicit_differentiation(ctx, c, eq_none):
    n, m, p = c
    B = 3
    qs = [nc.qp(n, m, p, SEED0 + i) for i in range(B)]
    bt = I.Batch(n, m, p, B, ctx, equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION)
    leaves = {k: _leaf(a) for k, a in _stack(qs).items()}
    x = layer.solve_qp(bt, **leaves)
    assert x.shape == (B, n)
    G = np.random.default_rng(77).standard_normal((B, n))
    (torch.from_numpy(G).cuda() * x).sum().backward()
    torch.cuda.synchronize()
    worst = 0.0
    for i in range(B):
        v = bt.state(i)
        assert np.array_equal(x[i].detach().cpu().numpy(), v[:n])
        ref, w = _implicit(qs[i], v, G[i], eq_none)
        # the adjoint solve to the bar (nc.TOL max(1, |w|inf) per element of w), carried through products with the
        # iterate (two per element of gA, gC), plus the bar on the gradient itself
        carried = 2 * nc.TOL * max(1.0, np.abs(w).max()) * max(1.0, np.abs(v).max())
        for k, r in ref.items():
            got = leaves[k].grad[i].cpu().numpy()
            bound = nc.TOL * max(1.0, np.abs(r).max()) + carried
            err = np.abs(got - r).max()
            err = np.inf if np.isnan(err) else err
            worst = max(worst, err / bound)
    print(f"{nc.case_id(c)} eq_none={eq_none}: worst |grad - numpy implicit| / bound {worst:.3e}", flush=True)
    assert worst <= 1.0


# 8 ---------------------------------------------------------------------------
def _box_qp(n, Q, c, lo, hi):
    return dict(n=n, m=0, p=0, Q=Q, c=c, A=np.zeros((0, n)), lA=np.zeros(0), uA=np.zeros(0), C=np.zeros((0, n)),
                d=np.zeros(0), lx=np.full(n, lo), ux=np.full(n, hi))


def _oracle_grads(q, g_x):
    o = oracle.OracleQP(q)
    for _ in range(100):
        conv, rec = o.iterate()
        if rec["converged"]:
            break
    assert rec["converged"]
    return _implicit(q, o.vars(), g_x)[0]


def _closed_form_case(kind):
    n = 12
    rng = np.random.default_rng(5)
    g = rng.standard_normal(n)
    if kind == "interior":  # Q SPD with condition <= 10, the minimiser -Q^{-1} c inside the box by at least 9
        U, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Q = (U * np.linspace(1.0, 10.0, n)) @ U.T
        Q = 0.5 * (Q + Q.T)
        xs = rng.uniform(-1.0, 1.0, n)
        q = _box_qp(n, Q, -Q @ xs, -10.0, 10.0)
        y = np.linalg.solve(Q, g)
        closed = dict(c=-y, Q=-np.outer(y, xs), l_x=np.zeros(n), u_x=np.zeros(n))
    else:  # diagonal Q, every -c_i / Q_ii at least 0.5 inside or outside [-1, 1]
        dq = rng.uniform(1.0, 4.0, n)
        t = np.array([0.3, -0.4, 1.7, -1.6, 0.0, 2.5, -2.0, 0.5, -0.5, 1.5, -1.5, 0.1])
        q = _box_qp(n, np.diag(dq), -dq * t, -1.0, 1.0)
        low, up = t < -1.0, t > 1.0
        free = ~(low | up)
        closed = dict(c=np.where(free, -g / dq, 0.0), l_x=np.where(low, g, 0.0), u_x=np.where(up, g, 0.0))
    return q, g, closed


@pytest.mark.parametrize("kind", ("interior", "active"))
def test_closed_forms(ctx, kind):
    q, g, closed = _closed_form_case(kind)
    n = q["n"]
    cpu = _oracle_grads(q, g)
    s = I.Optimizer(n, 0, 0, ctx)
    leaves = {k: _leaf(q[dc.KEYS[k]]) for k in ("Q", "c", "l_x", "u_x")}
    x = layer.solve_qp(s, **leaves)
    assert x.shape == (1, n)
    (torch.from_numpy(g).cuda() * x[0]).sum().backward()
    torch.cuda.synchronize()
    ok = True
    for k, cf in closed.items():
        e_gpu = float(np.abs(leaves[k].grad.cpu().numpy() - cf).max())
        e_cpu = float(np.abs(cpu[k] - cf).max())
        allowed = 10.0 * e_cpu + nc.TOL * max(1.0, float(np.abs(cf).max()))
        _accuracy[f"{kind}/{k}"] = dict(gpu_vs_closed_form=e_gpu, cpu_oracle_vs_closed_form=e_cpu, allowed=allowed)
        print(f"{kind} d/d{k}: GPU vs closed form {e_gpu:.3e}, CPU oracle vs closed form {e_cpu:.3e}, allowed "
              f"{allowed:.3e}", flush=True)
        ok = ok and e_gpu <= allowed
    if ACCURACY_JSON:
        with open(ACCURACY_JSON, "w") as f:
            json.dump(_accuracy, f, indent=1, sort_keys=True)
    assert ok


# 9 ---------------------------------------------------------------------------
def test_shared_inputs_get_the_sum_over_the_batch(ctx):
    n, m, p = nc.SHAPES[1]
    B = 3
    qs = [nc.qp(n, m, p, SEED0 + i) for i in range(B)]
    data = _stack(qs)
    data["Q"], data["A_ineq"] = qs[0]["Q"], qs[0]["A"]  # one Q and one A for every QP
    G = torch.from_numpy(np.random.default_rng(78).standard_normal((B, n))).cuda()
    bt = I.Batch(n, m, p, B, ctx)
    shared = {k: _leaf(a) for k, a in data.items()}
    x1 = layer.solve_qp(bt, **shared)
    (G * x1).sum().backward()
    full = {k: _leaf(a) for k, a in data.items()}
    for k in ("Q", "A_ineq"):
        full[k] = shared[k].detach().expand(B, *shared[k].shape).clone().requires_grad_(True)
    x2 = layer.solve_qp(bt, **full)
    (G * x2).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(x1, x2)
    worst = 0.0
    for k in data:
        a, b = shared[k].grad.cpu().numpy(), full[k].grad.cpu().numpy()
        assert a.shape == data[k].shape
        if k in ("Q", "A_ineq"):
            worst = max(worst, dc.rel_err(a, b.sum(axis=0)))
        else:
            assert np.array_equal(a, b), k
    print(f"shared Q and A_ineq: .grad vs the sum of the per-QP gradients {worst:.3e} (bound {nc.TOL:.1e})", flush=True)
    assert worst <= nc.TOL


# 10 --------------------------------------------------------------------------
def test_guards(ctx):
    n, m, p = nc.SHAPES[0]
    B = 2
    qs = [nc.qp(n, m, p, SEED0 + i) for i in range(B)]
    data = _stack(qs)
    bt = I.Batch(n, m, p, B, ctx)
    leaves = {k: _leaf(a) for k, a in data.items()}
    x = layer.solve_qp(bt, **leaves)
    bt.step()
    with pytest.raises(I.IpmzError, match="changed between forward and backward"):
        x.sum().backward()
    with pytest.raises(I.IpmzError, match="did not converge"):
        layer.solve_qp(bt, max_iter=1, **leaves)
    x = layer.solve_qp(bt, max_iter=1, strict=False, **leaves)
    assert x.shape == (B, n)
    # inputs that do not require grad get None; symmetrize returns the symmetric part of gQ
    some = {k: (_leaf(a) if k in ("Q", "b_eq") else torch.from_numpy(np.array(a)).cuda()) for k, a in data.items()}
    x = layer.solve_qp(bt, **some)
    x.sum().backward()
    gq = some["Q"].grad.clone()
    assert all((t.grad is None) == (k not in ("Q", "b_eq")) for k, t in some.items())
    sym = {k: _leaf(a) for k, a in data.items()}
    layer.solve_qp(bt, symmetrize=True, **sym).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(sym["Q"].grad, 0.5 * (gq + gq.transpose(1, 2)))
    assert not torch.equal(gq, gq.transpose(1, 2))
    print("guards: stale backward and strict refuse; requires_grad=False gets None; symmetrize", flush=True)
