"""Centering on the central path: ipmz_batch_center (Optimizer.center) and ipmz_amd.layer.solve_qp(barrier=).

The reference is the same loop in numpy (tests/center_cases.py: the formulation's residuals at mu = kappa, a dense
Jacobian solve, the ratio test, the 0.995 alpha update), started from the device's own solved iterate; the closed
form of the diagonal box QP for the layer.  kappa in {1e-2, 1e-4} (the box QP: {1e-2, 1e-3}), tol 1e-10, at most
30 iterations (tests/test_oracle_center.py guards that cap on the CPU).  Every test prints its worst figure before
it asserts.
"""
import ctypes
import functools

import numpy as np
import pytest

import batch_form_cases as fc
import center_cases as cc
import data_vjp_cases as dc
import newton_multi_cases as nc
import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")
layer = pytest.importorskip("ipmz_amd.layer")

TOL, CAP = cc.TOL, cc.MAX_ITER
EVALUATED = [I.SC[k] for k in ("f", "res", "mu", "converged")]


@functools.lru_cache(maxsize=None)
def shared_ctx(nbi=64):
    return I.Context(0) if nbi == 64 else I.Context(0, nbi=nbi)


def batch_of(s):
    return I.lib.ipmz_batch_size(s.h)


def make(form, shape, B, seed, nbi=64, solve=True):
    """A solver of B QPs (B == 1: an Optimizer), QP i = fc.qp(shape, seed + i), solved."""
    n, m, p = shape
    kw = dc.form_kw(form)
    s = I.Batch(n, m, p, B, shared_ctx(nbi), **kw) if B > 1 else I.Optimizer(n, m, p, shared_ctx(nbi), **kw)
    s.generate(seed)
    if solve:
        solve_all(s)
    return s


def solve_all(s):
    B = batch_of(s)
    if B > 1:
        _, nconv = s.solve_all(100)
        assert nconv == B
    else:
        s.solve(100)
        assert s.scalars()["converged"] == 1.0


def state(s, which=0):
    return s.state_tensor(which).cpu().numpy().copy()


def scalars(s):
    out = np.zeros(batch_of(s) * I.SC_COUNT)
    assert I.lib.ipmz_batch_scalars(s.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    return out.reshape(-1, I.SC_COUNT)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(a):
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


def positive(form, shape, z):
    v = dc.form_split(form, *shape, z)
    return all(np.all(v[k] > 0.0) for k in v if k in oracle.NONNEG)


def run(form, shape, B, seed, kappa, nbi=64, max_iter=CAP):
    """solve, center: (the solved iterates, the centered ones, iterations, centered count)."""
    s = make(form, shape, B, seed, nbi)
    try:
        z0 = state(s)
        its, centered = s.center(kappa, TOL, max_iter)
        return z0, state(s), its.copy(), centered
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def cached_run(form, shape, B, seed, kappa, nbi=64):
    out = run(form, shape, B, seed, kappa, nbi)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def path_conditions(form, shape, B, seed, kappa, out, what):
    """centered == batch; numpy's residual at mu = kappa of every device iterate within the bar; the interior."""
    z0, z, its, centered = out
    worst = 0.0
    for i in range(B):
        q = fc.qp(shape, seed + i)
        e = cc.resid_norm(form, q, z[i], kappa)
        worst = max(worst, e / cc.residual_bound(q, z[i], TOL))
        assert positive(form, shape, z[i]), f"{what}: QP {i} left the interior"
    print(f"{what} kappa {kappa:g}: centered {centered}/{B}, iterations {its.tolist()}, worst |r(z; kappa)|inf / "
          f"bound {worst:.3e}", flush=True)
    assert centered == B, f"{what}: {centered} of {B} centered"
    assert worst <= 1.0
    assert np.all(its <= CAP)


def against_reference(form, shape, B, seed, kappa, out, what):
    """|z_dev - z_ref|inf <= |J^-1|inf 2 tol with J at z_ref (both meet the same residual bound, and the path point
    is unique); the device's count at most the reference's + 2."""
    z0, z, its, centered = out
    worst = 0.0
    for i in range(B):
        q = fc.qp(shape, seed + i)
        zr, itr, ok, e = cc.center(q, z0[i], kappa, TOL, CAP, form)
        assert ok, (what, i, itr, e)
        bound = cc.jinv_norm(form, q, zr, kappa) * 2 * TOL
        err = float(np.abs(z[i] - zr).max())
        err = np.inf if np.isnan(err) else err
        worst = max(worst, err / bound)
        print(f"{what} kappa {kappa:g} QP {i}: |z - z_ref|inf {err:.3e} (bound {bound:.3e}), iterations {its[i]} "
              f"(reference {itr})", flush=True)
        assert its[i] <= itr + 2
    assert worst <= 1.0


# 1, 2 ------------------------------------------------------------------------
FORM_CASES = [(f, fc.S1, B) for f in cc.FORMS for B in (1, 3)] + \
             [(f, fc.S0, B) for f in cc.FORMS if f in fc.S0_FORMS for B in (1, 3)]
FORM_IDS = [f"{f}-{fc.SHAPE_NAMES[s]}-B{B}" for f, s, B in FORM_CASES]


@pytest.mark.parametrize("case", FORM_CASES, ids=FORM_IDS)
def test_path_conditions_per_form(case):
    form, shape, B = case
    for kappa in cc.KAPPAS:
        path_conditions(form, shape, B, fc.SEED0[shape], kappa, cached_run(form, shape, B, fc.SEED0[shape], kappa),
                        f"{form} {fc.SHAPE_NAMES[shape]} B={B}")


@pytest.mark.parametrize("case", FORM_CASES, ids=FORM_IDS)
def test_against_the_numpy_reference(case):
    form, shape, B = case
    for kappa in cc.KAPPAS:
        against_reference(form, shape, B, fc.SEED0[shape], kappa, cached_run(form, shape, B, fc.SEED0[shape], kappa),
                          f"{form} {fc.SHAPE_NAMES[shape]} B={B}")


# 3 ---------------------------------------------------------------------------
def test_composition_from_existing_calls():
    """The same loop from state_tensor(RES) minus kappa on the complementarity entries, newton_solve_all and
    set_state_tensor."""
    form, shape, B, seed = "box", fc.S1, 3, fc.SEED0[fc.S1]
    order, sz, off, L = dc.form_offsets(form, *shape)
    comp = np.zeros(L)  # (float64: kappa times a bool tensor would round kappa to float32)
    for k in ("g", "h", "y", "z"):
        comp[off[k]:off[k] + sz[k]] = 1.0
    comp_t = dev(comp)
    ld = nc.even(L)
    for kappa in cc.KAPPAS:
        z0, z, its, centered = cached_run(form, shape, B, seed, kappa)
        bt = make(form, shape, B, seed)
        count = np.zeros(B, dtype=int)
        for it in range(CAP + 1):
            R = torch.zeros((B, ld), dtype=torch.float64, device="cuda")
            R[:, :L] = bt.state_tensor(3)
            R[:, :L] -= kappa * comp_t
            open_ = R.abs().amax(dim=1) > TOL
            if not bool(open_.any()) or it == CAP:
                break
            D = torch.zeros((B, ld), dtype=torch.float64, device="cuda")
            alpha = torch.zeros(B, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            bt.newton_solve_all(R.data_ptr(), D.data_ptr(), 1, ld, ld, ld, ld, alpha.data_ptr())
            V = bt.state_tensor(0) + 0.995 * alpha[:, None] * D[:, :L]
            bt.set_state_tensor(V.contiguous(), take=open_)
            count += open_.cpu().numpy()
        zc = state(bt)
        bt.close()
        err = max(float(np.abs(zc[i] - z[i]).max()) / max(1.0, float(np.abs(z[i]).max())) for i in range(B))
        print(f"composition kappa {kappa:g}: |z_center - z_composed|inf / max(1, |z|inf) {err:.3e} (bound "
              f"{nc.TOL:.1e}), iterations {its.tolist()} vs {count.tolist()}", flush=True)
        assert not bool(open_.any())
        assert err <= nc.TOL


# 4 ---------------------------------------------------------------------------
# (form, shape, B, seed, nbi, compare with the numpy reference): the reference's dense solves stay small
SHAPE_CASES = [
    ("box", nc.SHAPES[0], 1, nc.SEED, 64, True),      # N below one block, slots of different lengths
    ("box", (256, 48, 17), 1, nc.SEED, 64, True),     # odd N, L past one workgroup of the norm
    ("none", (256, 48, 17), 1, nc.SEED, 64, True),    # ... and an odd L: the tail element of the norm's pairs
    ("box", fc.SL, 2, fc.SEED0[fc.SL], 64, False),    # the non-fused batch path, N > 1024
    ("box", fc.S128, 3, fc.SEED0[fc.S128], 128, True),  # inner block 128
    ("none", fc.S1, 1, fc.SEED0[fc.S1], 64, True),    # Bunch-Kaufman, one workgroup
    ("none", fc.S1, 3, fc.SEED0[fc.S1], 64, True),    # ... per QP of a batch
    ("box", (130, 40, 22), 3, 1100, 64, True),
    ("box", fc.S2, 1, fc.SEED0[fc.S2], 64, False),    # a single QP whose factor forks onto the look-ahead streams
]


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[f"{c[0]}-n{c[1][0]}_m{c[1][1]}_p{c[1][2]}-B{c[2]}-nbi{c[4]}"
                                                   for c in SHAPE_CASES])
def test_shapes_where_a_kernel_can_go_wrong(case):
    form, shape, B, seed, nbi, ref = case
    what = f"{form} {shape} B={B} nbi={nbi}"
    for kappa in cc.KAPPAS:
        out = run(form, shape, B, seed, kappa, nbi)
        path_conditions(form, shape, B, seed, kappa, out, what)
        if ref:
            against_reference(form, shape, B, seed, kappa, out, what)


# 5 ---------------------------------------------------------------------------
def test_second_call_applies_nothing_and_runs_repeat():
    form, shape, B, seed, kappa = "box", fc.S1, 3, fc.SEED0[fc.S1], cc.KAPPAS[0]
    bt = make(form, shape, B, seed)
    its, centered = bt.center(kappa, TOL, CAP)
    snap = [state(bt, 0), state(bt, 3), scalars(bt)]
    its2, centered2 = bt.center(kappa, TOL, CAP)
    print(f"second call: iterations {its.tolist()} then {its2.tolist()}, centered {centered} then {centered2}",
          flush=True)
    assert centered == B and centered2 == B and np.all(its > 0) and np.all(its2 == 0)
    for a, b in zip(snap, [state(bt, 0), state(bt, 3), scalars(bt)]):
        assert same(a, b)
    bt.close()
    # two runs give equal bits
    a, b = cached_run(form, shape, B, seed, kappa), run(form, shape, B, seed, kappa)
    assert same(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_centered_qp_keeps_its_bits_beside_working_ones():
    form, shape, B, seed, kappa = "box", fc.S1, 3, fc.SEED0[fc.S1], cc.KAPPAS[0]
    bt = make(form, shape, B, seed)
    z0 = state(bt)
    bt.center(kappa, TOL, CAP)
    z = state(bt)
    # QP 0 stays centered; the others are warm-started away, back to their solved iterates
    bt.set_state_tensor(dev(z0), take=dev(np.array([0, 1, 1])))
    its, centered = bt.center(kappa, TOL, CAP)
    z2 = state(bt)
    print(f"one centered QP beside two working ones: iterations {its.tolist()}, centered {centered}", flush=True)
    assert centered == B and its[0] == 0 and np.all(its[1:] > 0)
    assert same(z2[0], z[0])
    # ... and the two get what they got the first time: a QP's result does not depend on its neighbours' state
    assert same(z2[1:], z[1:])
    bt.close()


def _stack(qs):
    return {k: dev(np.stack([q[dc.KEYS[k]] for q in qs])) for k in dc.present(qs[0]["n"], qs[0]["m"], qs[0]["p"])}


def test_permuting_the_batch_permutes_the_results():
    shape, B, seed, kappa = fc.S1, 3, fc.SEED0[fc.S1], cc.KAPPAS[0]
    n, m, p = shape
    qs = [fc.qp(shape, seed + i) for i in range(B)]
    perm = [2, 0, 1]
    res = []
    for order in (list(range(B)), perm):
        bt = I.Batch(n, m, p, B, shared_ctx())
        bt.load_tensors(**_stack([qs[i] for i in order]))
        solve_all(bt)
        its, centered = bt.center(kappa, TOL, CAP)
        assert centered == B
        res.append((state(bt), its.copy(), scalars(bt)))
        bt.close()
    (z, its, sc), (zp, itsp, scp) = res
    print(f"permutation {perm}: iterations {its.tolist()} and {itsp.tolist()}", flush=True)
    for k, i in enumerate(perm):
        assert same(zp[k], z[i]) and itsp[k] == its[i] and same(scp[k][EVALUATED], sc[i][EVALUATED])


def test_one_iteration_leaves_the_batch_uncentered():
    form, shape, B, seed, kappa = "box", fc.S1, 3, fc.SEED0[fc.S1], cc.KAPPAS[0]
    z0, z, its, centered = run(form, shape, B, seed, kappa, max_iter=1)
    print(f"max_iter 1: iterations {its.tolist()}, centered {centered}", flush=True)
    assert centered < B and np.all(its == 1)
    assert not same(z0, z)
    # max_iter 0 tests, evaluates and reports, and moves nothing
    z0, z, its, centered = run(form, shape, B, seed, kappa, max_iter=0)
    assert centered == 0 and np.all(its == 0) and same(z0, z)


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 3))
def test_state_afterwards(B):
    form, shape, seed, kappa = "box", fc.S1, fc.SEED0[fc.S1], cc.KAPPAS[0]
    s = make(form, shape, B, seed)
    steps_before = scalars(s)[:, I.SC["steps"]].copy()
    its, centered = s.center(kappa, TOL, CAP)
    assert centered == B
    z, res, sc = state(s), state(s, 3), scalars(s)
    print(f"B={B}: mu after centering {sc[:, I.SC['mu']].tolist()} (kappa {kappa:g}), converged "
          f"{sc[:, I.SC['converged']].tolist()}", flush=True)
    assert np.all(np.abs(sc[:, I.SC["mu"]] - kappa) <= 1e-3 * kappa) and np.all(sc[:, I.SC["converged"]] == 0.0)
    assert same(sc[:, I.SC["steps"]], steps_before)
    # the same solver given its own iterate: the whole scalar block and the residual slots keep their bits
    s.set_state_tensor(dev(z))
    assert same(state(s), z) and same(state(s, 3), res) and same(scalars(s), sc)
    # a fresh solver given that iterate: the evaluated entries and the residual slots
    f = make(form, shape, B, seed, solve=False)
    f.set_state_tensor(dev(z))
    assert same(state(f, 3), res) and same(scalars(f)[:, EVALUATED], sc[:, EVALUATED])
    # one step of each (the fused path's kept KKT matrix included)
    s.step()
    f.step()
    for which in range(4):
        assert same(state(s, which), state(f, which)), which
    assert same(scalars(s), scalars(f))
    f.close()
    solve_all(s)
    s.close()


# 7 ---------------------------------------------------------------------------
def _leaf(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda().requires_grad_(True)
    torch.cuda.synchronize()
    return t


def _oracle_converged(q):
    o = oracle.OracleQP(q)
    for _ in range(100):
        conv, rec = o.iterate()
        if rec["converged"]:
            break
    assert rec["converged"]
    return o.vars()


@pytest.mark.parametrize("kappa", cc.BOX_KAPPAS)
def test_layer_box_closed_form(kappa):
    import torch.autograd.forward_ad as fwAD
    q, dq, g = cc.box_case()
    n = cc.BOX_N
    x_cf = cc.box_root(dq, q["c"], q["lx"], q["ux"], kappa)
    deriv, D = cc.box_derivatives(dq, x_cf, q["lx"], q["ux"], kappa)
    closed = {k: g * deriv[k] for k in deriv}
    # the numpy reference run with the same tol: its point, its gradients and its tangent, against the closed form
    zr, itr, ok, _ = cc.center(q, _oracle_converged(q), kappa, TOL, CAP)
    assert ok
    cpu = cc.box_implicit(q, zr, g)
    tc = np.random.default_rng(6).standard_normal(n)
    rt = np.zeros(len(zr))
    rt[:n] = tc
    dx_cpu = np.linalg.solve(nc.full_jacobian(q, zr), -rt)[:n]
    dx_cf = -tc / D
    s = I.Optimizer(n, 0, 0, shared_ctx())
    leaves = {k: _leaf(q[dc.KEYS[k]]) for k in ("Q", "c", "l_x", "u_x")}
    x = layer.solve_qp(s, barrier=kappa, barrier_tol=TOL, barrier_max_iter=CAP, **leaves)
    assert x.shape == (1, n)
    (dev(g) * x[0]).sum().backward()
    torch.cuda.synchronize()
    xd = x[0].detach().cpu().numpy()
    bound = cc.jinv_norm("box", q, zr, kappa) * 2 * TOL
    err = float(np.abs(xd - x_cf).max())
    print(f"box kappa {kappa:g}: |x - bisection root|inf {err:.3e} (bound {bound:.3e}); numpy reference "
          f"{float(np.abs(zr[:n] - x_cf).max()):.3e} in {itr} iterations", flush=True)
    ok = err <= bound
    got = dict(c=leaves["c"].grad.cpu().numpy(), Q=np.diag(leaves["Q"].grad.cpu().numpy()).copy(),
               l_x=leaves["l_x"].grad.cpu().numpy(), u_x=leaves["u_x"].grad.cpu().numpy())
    for k, cf in closed.items():
        e_gpu, e_cpu = float(np.abs(got[k] - cf).max()), float(np.abs(cpu[k] - cf).max())
        allowed = max(10.0 * e_cpu, nc.TOL)
        print(f"  d/d{k}: GPU vs closed form {e_gpu:.3e}, numpy reference vs closed form {e_cpu:.3e}, allowed "
              f"{allowed:.3e}", flush=True)
        ok = ok and e_gpu <= allowed
    # forward mode: the tangent of x along a tangent of c
    prim = {k: t.detach() for k, t in leaves.items()}
    with fwAD.dual_level():
        duals = dict(prim, c=fwAD.make_dual(prim["c"], dev(tc)))
        xt = fwAD.unpack_dual(layer.solve_qp(s, barrier=kappa, barrier_tol=TOL, barrier_max_iter=CAP, **duals)).tangent
        xt = xt[0].cpu().numpy()
    e_gpu, e_cpu = float(np.abs(xt - dx_cf).max()), float(np.abs(dx_cpu - dx_cf).max())
    allowed = max(10.0 * e_cpu, nc.TOL)
    print(f"  forward_ad tangent of c: GPU vs closed form {e_gpu:.3e}, numpy reference vs closed form {e_cpu:.3e}, "
          f"allowed {allowed:.3e}", flush=True)
    ok = ok and e_gpu <= allowed
    # the degenerate coordinates: a gradient strictly between that of an inactive and of an active bound
    jac = layer.solution_jacobian(s, only=["c"])[0]["c"][0].cpu().numpy()
    for i in cc.BOX_DEGENERATE:
        print(f"  coordinate {i} (minimiser on its bound): -dx/dc {-jac[i, i]:.4f}, 1/q {1.0 / dq[i]:.4f}", flush=True)
        ok = ok and 0.0 < -jac[i, i] < 1.0 / dq[i]
    s.close()
    assert ok


def test_layer_backward_vs_numpy_implicit_differentiation():
    n, m, p = shape = fc.S1
    B, seed, kappa = 3, 1000, cc.KAPPAS[0]
    qs = [nc.qp(n, m, p, seed + i) for i in range(B)]
    bt = I.Batch(n, m, p, B, shared_ctx())
    leaves = {k: _leaf(np.stack([q[dc.KEYS[k]] for q in qs])) for k in dc.present(n, m, p)}
    x = layer.solve_qp(bt, barrier=kappa, **leaves)
    G = np.random.default_rng(77).standard_normal((B, n))
    (torch.from_numpy(G).cuda() * x).sum().backward()
    torch.cuda.synchronize()
    worst = 0.0
    for i in range(B):
        v = bt.state(i)
        assert np.array_equal(x[i].detach().cpu().numpy(), v[:n])
        assert cc.resid_norm("box", qs[i], v, kappa) <= cc.residual_bound(qs[i], v, TOL)
        J = nc.full_jacobian(qs[i], v)
        g = np.zeros(J.shape[0])
        g[:n] = G[i]
        w = np.linalg.solve(J.T, -g)
        ref = dc.reference(qs[i], v, w)
        # (the bar of tests/test_gpu_qp_layer.py: the adjoint solve to nc.TOL max(1, |w|inf) per element, carried
        # through products with the iterate, plus the bar on the gradient itself)
        carried = 2 * nc.TOL * max(1.0, np.abs(w).max()) * max(1.0, np.abs(v).max())
        for k, r in ref.items():
            err = np.abs(leaves[k].grad[i].cpu().numpy() - r).max()
            err = np.inf if np.isnan(err) else err
            worst = max(worst, err / (nc.TOL * max(1.0, np.abs(r).max()) + carried))
    bt.close()
    print(f"barrier {kappa:g}: worst |grad - numpy implicit| / bound {worst:.3e}", flush=True)
    assert worst <= 1.0


def test_layer_without_barrier_keeps_its_bits():
    n, m, p = shape = fc.S1
    B, seed = 3, 1000
    qs = [nc.qp(n, m, p, seed + i) for i in range(B)]
    G = torch.from_numpy(np.random.default_rng(77).standard_normal((B, n))).cuda()
    out = []
    for kw in (dict(), dict(barrier=None)):
        bt = I.Batch(n, m, p, B, shared_ctx())
        leaves = {k: _leaf(np.stack([q[dc.KEYS[k]] for q in qs])) for k in dc.present(n, m, p)}
        x = layer.solve_qp(bt, **kw, **leaves)
        (G * x).sum().backward()
        torch.cuda.synchronize()
        out.append((x.detach().cpu().numpy(), {k: t.grad.cpu().numpy() for k, t in leaves.items()}))
        bt.close()
    assert same(out[0][0], out[1][0])
    assert all(same(out[0][1][k], out[1][1][k]) for k in out[0][1])
    # strict: a QP that is not centered raises, strict=False returns
    bt = I.Batch(n, m, p, B, shared_ctx())
    data = {k: t.detach() for k, t in leaves.items()}
    with pytest.raises(I.IpmzError, match="not centered"):
        layer.solve_qp(bt, barrier=1e-2, barrier_max_iter=1, **data)
    assert layer.solve_qp(bt, barrier=1e-2, barrier_max_iter=1, strict=False, **data).shape == (B, n)
    bt.close()


# 8 ---------------------------------------------------------------------------
def test_refusals():
    n, m, p = shape = fc.S1
    ctx = shared_ctx()
    s = make("box", shape, 1, 7)
    z = state(s)
    nan, inf = float("nan"), float("inf")
    for bad in (0.0, -1e-2, nan, inf):
        with pytest.raises(I.IpmzError, match="invalid argument.*kappa"):
            s.center(bad)
        with pytest.raises(I.IpmzError, match="invalid argument.*tol"):
            s.center(1e-2, tol=bad)
    with pytest.raises(I.IpmzError, match="invalid argument.*max_iter"):
        s.center(1e-2, max_iter=-1)
    s.set_reduction(I.REDUCTION_NORMAL)
    with pytest.raises(I.IpmzError, match="invalid argument.*normal-equations"):
        s.center(1e-2)
    s.set_reduction(I.REDUCTION_AUGMENTED)
    s.set_mixed_precision(True)
    with pytest.raises(I.IpmzError, match="invalid argument.*mixed precision"):
        s.center(1e-2)
    s.set_mixed_precision(False)
    assert same(state(s), z), "a refused call moved the iterate"
    its, centered = s.center(1e-2)
    assert centered == 1
    s.close()
    for form, text in (("eqss", "SlackedSlacks / NaiveSlacks"), ("naiveeq", "SlackedSlacks / NaiveSlacks"),
                       ("pen", "PenaltyFunction"), ("sl", "InequalityHandling::Slacks")):
        for B in (1, 3):
            r = make(form, shape, B, 7, solve=False)
            with pytest.raises(I.IpmzError, match="invalid argument.*" + text):
                r.center(1e-2)
            r.close()
    r = I.Optimizer(n, m, p, ctx, equality_handling=I.EQ_PENALTY_EXTRA_DUAL)
    with pytest.raises(I.IpmzError, match="invalid argument.*PenaltyFunction"):  # (before the check for a load)
        r.center(1e-2)
    r.close()
    # (IPMZ_EQ_NONE batches with N > 4096 cannot be created: ipmz_batch_create refuses them)
    with pytest.raises(I.IpmzError, match="4096"):
        I.Batch(4097, 0, 0, 2, ctx, equality_handling=I.EQ_NONE)
    # before a load, and between a load and initialize
    fresh = I.Batch(n, m, p, 3, ctx)
    with pytest.raises(I.IpmzError, match="bad state.*load"):
        fresh.center(1e-2)
    fresh.generate(7)
    q = fc.qp(shape, 7)
    fresh.load_one(0, I.Data(**{k: q[dc.KEYS[k]] for k in dc.NAMES}))
    with pytest.raises(I.IpmzError, match="bad state.*load"):
        fresh.center(1e-2)
    fresh.close()
    print("refusals: kappa, tol, max_iter, reduction, mixed precision, four formulations, the load states", flush=True)


def test_refused_in_a_graph_capture():
    st = torch.cuda.Stream()
    c = I.Context(0, stream=st.cuda_stream)
    try:
        n, m, p = fc.S1
        bt = I.Batch(n, m, p, 3, c)
        bt.generate(7)
        solve_all(bt)
        z = state(bt)
        t = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st, capture_error_mode="thread_local"):
            t.add_(1.0)
            with pytest.raises(I.IpmzError, match="bad state.*capturing"):
                bt.center(1e-2)
        torch.cuda.synchronize()
        assert same(state(bt), z)
        its, centered = bt.center(1e-2)
        assert centered == 3
        bt.close()
    finally:
        c.close()
