"""The batched kernels of the gradient with respect to the problem data (csrc/grad.hip) on every served formulation
and through every loop a solver's shapes can reach.

Reference (tests/data_vjp_cases.py): reference_form, the numpy transposes of the formulation's "shorthand
definitions" (tests/golden/formulations.txt; tests/test_oracle_data_vjp.py shows it to be the transpose for every
form without a GPU), from the device's iterate and the cotangent alone -- elementwise, for every QP of the batch.
residuals_form, the restatement it is pinned against, is tied to the device's residual path here.

Bounds.  Per-QP blocks that are a copy, a negation or one product: bitwise.  A_ineq and A_eq (two products and a sum):
nc.TOL relative to max(1, |ref|inf) per QP.  Shared blocks, against the longdouble sum over the QPs of the reference:
nc.TOL max(1, max_elem sum_z |g_z|) -- any summation order of B doubles stays within (B - 1) 2^-53 sum_z |g_z| of the
exact sum, 4.5e-13 sum |g_z| at B = 4097, so the project's bar holds whatever order the kernels choose; two runs give
equal bits.  Every test prints its worst figure before it asserts.
"""
import time

import numpy as np
import pytest

import batch_form_cases as fc
import data_vjp_cases as dc
import newton_multi_cases as nc

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

VECTORS = tuple(k for k in dc.NAMES if k not in dc.MATRICES)
TWO_PRODUCTS = ("A_ineq", "A_eq")


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _dev(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return t


def _host(grads):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in grads.items()}


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                                 np.ascontiguousarray(b).view(np.int64))


def _stepped(name, shape, B, seed0, ctx, steps=2):
    """The batch after `steps` steps, its iterates (B, L) on the host and its cotangents on both sides."""
    bt = I.Batch(*shape, B, ctx, **dc.form_kw(name))
    bt.generate(seed0)
    for _ in range(steps):
        bt.step()
    L = bt.state_len
    assert L == dc.form_offsets(name, *shape)[3]
    V = bt.state_tensor(0).cpu().numpy()
    assert V.shape == (B, L) and np.isfinite(V).all()
    W = np.array(dc.cotangents(L, B))
    return bt, V, W, _dev(W)


def _references(fn, V, W):
    """{name: (B, ...)}: fn(iterate, cotangent) for every QP."""
    each = [fn(V[i], W[i]) for i in range(V.shape[0])]
    return {k: np.stack([g[k] for g in each]) for k in each[0]}


def _check_per_qp(got, refs):
    """Every QP's block against its reference; returns the worst relative error of the two-product blocks."""
    assert set(got) == set(refs)
    worst = 0.0
    for k, ref in refs.items():
        assert got[k].shape == ref.shape, k
        if k in TWO_PRODUCTS:
            axes = tuple(range(1, ref.ndim))
            err = np.abs(got[k] - ref).max(axis=axes) / np.maximum(1.0, np.abs(ref).max(axis=axes))
            err = np.where(np.isnan(err), np.inf, err)
            worst = max(worst, float(err.max()))
        else:
            bad = np.argwhere(got[k].view(np.int64) != ref.view(np.int64))
            assert bad.size == 0, (k, "first differing [QP, ...]", bad[0].tolist(), len(bad))
    return worst


def _check_shared(got, refs):
    """Every shared block against the longdouble sum of the references; returns the worst error / bound."""
    assert set(got) == set(refs)
    worst = 0.0
    for k, ref in refs.items():
        want, bound = dc.shared_reference(ref)
        assert got[k].shape == want.shape, k
        err = float(np.abs(got[k] - want).max())
        worst = max(worst, np.inf if np.isnan(err) else err / bound)
    return worst


# 1 ---------------------------------------------------------------------------
# No formulation's residual state carries a mu of its own: the evaluation that ends a step (and set_vars) writes every
# r_v at mu = 0 (the corrector's mu-carrying rows are overwritten by it), so every slot is compared.  Were one to
# carry it, its slots would be listed here and left out.
MU_SLOTS = {name: () for name in dc.FORM_NAMES}


@pytest.mark.parametrize("name", dc.FORM_NAMES)
def test_residuals_form_is_the_device_residual_path(ctx, name):
    shape = fc.S1
    seed = fc.seed0(shape, name)
    q = nc.qp(*shape, seed)
    g = I.Optimizer(*shape, ctx, **dc.form_kw(name))
    g.generate(seed)
    g.step()
    v, r = g.vars(), g.residuals()
    order, sz, off, L = dc.form_offsets(name, *shape)
    assert L == g.state_len
    ref = dc.residuals_form(name, q, v, 0.0)
    keep = np.ones(L, bool)
    for s in MU_SLOTS[name]:
        keep[off[s]:off[s] + sz[s]] = False
    err = dc.rel_err(r[keep], ref[keep])
    print(f"{name} L={L}: device residuals vs residuals_form(mu=0) {err:.3e} (bound {nc.TOL:.1e}; "
          f"slots left out: {MU_SLOTS[name] or 'none'})", flush=True)
    assert err <= nc.TOL


# 2 ---------------------------------------------------------------------------
FORM_B = 5  # one full K step of the 16x16x4 MFMA plus a tail of one
FORM_CASES = [(name, fc.S1) for name in dc.FORM_NAMES] + [("vnone", fc.S0)]  # S0: m = 0 meets a shared launch


@pytest.mark.parametrize("name,shape", FORM_CASES, ids=[f"{n}-{fc.SHAPE_NAMES[s]}" for n, s in FORM_CASES])
def test_every_formulation_through_the_batched_kernels(ctx, name, shape):
    n, m, p = shape
    B = FORM_B
    bt, V, W, Wt = _stepped(name, shape, B, fc.seed0(shape, name), ctx)
    names = dc.present(n, m, p)
    refs = _references(lambda v, w: dc.reference_form(name, n, m, p, v, w), V, W)
    assert set(refs) == set(names)
    per = _host(bt.data_grad_tensors(Wt))
    sh = _host(bt.data_grad_tensors(Wt, shared=names))
    worst_per = _check_per_qp(per, refs)
    worst_sh = _check_shared(sh, refs)
    print(f"{name} {fc.SHAPE_NAMES[shape]} B={B}: per-QP A_ineq / A_eq vs numpy {worst_per:.3e} (bound {nc.TOL:.1e}), "
          f"the other blocks bitwise; shared vs the longdouble sum, error / bound {worst_sh:.3e}", flush=True)
    assert worst_per <= nc.TOL
    assert worst_sh <= 1.0
    for k in dc.form_absent(name):
        if k in names:  # a bound the formulation lacks: exactly zero in both layouts
            assert not per[k].any() and not sh[k].any(), k
    again = _host(bt.data_grad_tensors(Wt, shared=names))
    again_per = _host(bt.data_grad_tensors(Wt))
    for k in names:
        assert _same(again[k], sh[k]) and _same(again_per[k], per[k]), ("two runs", k)


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", dc.LOOP_BATCHES)
def test_default_form_loops(ctx, B):
    """dc.LOOP_BATCHES (the table's comment says which loop each batch reaches): every per-QP block of every QP
    against numpy, every shared block against the longdouble sum."""
    n, m, p = shape = dc.LOOP_SHAPE
    if B == max(dc.LOOP_BATCHES):
        # grad_grid: k_grad_matrix has ceil(rows / 4) workgroups per QP and 4096 // that many QPs in flight,
        # k_grad_vectors one workgroup per QP and 4096 in flight: past both, a workgroup handles a second QP
        assert B > dc.GRID_Y // -(-n // 4), "k_grad_matrix<G_Q> no longer loops over the QPs at this batch"
        assert B > dc.GRID_Y, "k_grad_vectors no longer loops over the QPs at this batch"
    t0 = time.perf_counter()
    bt, V, W, Wt = _stepped("box", shape, B, 1000, ctx)
    names = dc.present(n, m, p)
    dims = dict(n=n, m=m, p=p)
    refs = _references(lambda v, w: dc.reference(dims, v, w), V, W)
    per = _host(bt.data_grad_tensors(Wt))
    sh = _host(bt.data_grad_tensors(Wt, shared=names))
    worst_per = _check_per_qp(per, refs)
    worst_sh = _check_shared(sh, refs)
    print(f"default form n{n} m{m} p{p} B={B}: per-QP A_ineq / A_eq vs numpy {worst_per:.3e} (bound {nc.TOL:.1e}), "
          f"the other blocks bitwise for every QP; shared vs the longdouble sum, error / bound {worst_sh:.3e}; "
          f"{time.perf_counter() - t0:.2f} s", flush=True)
    assert worst_per <= nc.TOL
    assert worst_sh <= 1.0
    again = _host(bt.data_grad_tensors(Wt, shared=names))
    for k in names:
        assert _same(again[k], sh[k]), ("two runs", k)


def test_slacks_shared_vectors_over_several_qps_per_range(ctx):
    """The iterate-dependent branch of k_grad_vectors_shared with 5 QPs per range (B = 257)."""
    n, m, p = shape = dc.LOOP_SHAPE
    B = dc.LOOP_BATCHES[0]
    bt, V, W, Wt = _stepped("sl", shape, B, 1000, ctx)
    refs = _references(lambda v, w: dc.reference_form("sl", n, m, p, v, w), V, W)
    refs = {k: refs[k] for k in VECTORS}
    sh = _host(bt.data_grad_tensors(Wt, shared=VECTORS, only=VECTORS))
    worst = _check_shared(sh, refs)
    print(f"Slacks n{n} m{m} p{p} B={B}: shared vectors vs the longdouble sum, error / bound {worst:.3e}", flush=True)
    assert worst <= 1.0
    assert any(refs[k].any() for k in ("l_x", "u_x", "l_A_ineq", "u_A_ineq"))
    again = _host(bt.data_grad_tensors(Wt, shared=VECTORS, only=VECTORS))
    for k in VECTORS:
        assert _same(again[k], sh[k]), ("two runs", k)


def test_shared_sum_second_pass(ctx):
    """n = dc.BIG_N, m = p = 0, B = 2, Q alone: rows * n exceeds k_grad_shared_sum's 2048 x 256 threads, so its
    grid-stride loop makes a second pass.  gQ = w_x x^T: one product per element."""
    n, B = dc.BIG_N, 2
    assert n * n > dc.SUM_GX * 256
    t0 = time.perf_counter()
    bt, V, W, Wt = _stepped("box", (n, 0, 0), B, 1000, ctx)
    refs = {"Q": np.stack([np.outer(W[i, :n], V[i, :n]) for i in range(B)])}
    per = _host(bt.data_grad_tensors(Wt, only=["Q"]))
    sh = _host(bt.data_grad_tensors(Wt, shared=["Q"], only=["Q"]))
    _check_per_qp(per, refs)
    worst = _check_shared(sh, refs)
    print(f"n={n} B={B}: per-QP Q bitwise w_x x^T; shared Q vs the longdouble sum, error / bound {worst:.3e}; "
          f"{time.perf_counter() - t0:.2f} s", flush=True)
    assert worst <= 1.0
    assert _same(_host(bt.data_grad_tensors(Wt, shared=["Q"], only=["Q"]))["Q"], sh["Q"]), "two runs"
