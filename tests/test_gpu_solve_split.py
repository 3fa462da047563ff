"""The persistent triangular solve with its 128-row blocks split over H = 2
and H = 4 workgroups (debug bits SOLVE_H2 / SOLVE_H4), and with the H the
library picks by itself, against the unsplit solve (H = 1, both bits) and the
CPU oracle.  Run on an MI355X: pytest -m gpu.

A split solve runs every element through the same operations in the same
order as the unsplit one, so its result is bitwise the H = 1 result
(np.array_equal); against the oracle the bound is the one of
test_gpu_parity.py::test_ldlt_ragged_vs_oracle, |x - x_ref|_inf < 1e-10.

Shapes (blocking (256, 64)): 100 = one ragged block; 129 = two blocks with a
1-row tail (parts 1 .. H-1 of the last block own no rows); 513, 710 = J >= 4,
so the pair loop, the lone tile and M_J / Q_J all run, 710 with a 70-row tail
(parts of 32, 32, 6 and 0 rows at H = 4); 1000, 1349 = even / odd counts of
bulk tiles behind them.
"""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

SOLVE_H2, SOLVE_H4 = 524288, 1048576  # kernels.h IPMZ_DEBUG_SOLVE_H2 / _H4
# forced H; both bits force the unsplit solve; "table" = what the library picks by itself
MASK = {1: SOLVE_H2 | SOLVE_H4, 2: SOLVE_H2, 4: SOLVE_H4, "table": 0}
SPLITS = (2, 4, "table")
TOL = 1e-10  # test_ldlt_ragged_vs_oracle


@pytest.fixture(scope="module")
def ctx():
    c = I.Context(0)
    c.set_blocking(256, 64)
    return c


@pytest.fixture(autouse=True)
def _mask_off():
    yield
    I.debug_inject(0)


def _qd(N, seed, scaled=False):
    """Quasi-definite symmetric matrix (test_gpu_parity.py; scaled: the badly
    scaled rows / columns of test_gpu_mixed.py)."""
    rng = np.random.default_rng(seed)
    n1 = (3 * N + 3) // 4
    K = rng.uniform(-1, 1, (N, N))
    K[:n1, :n1] /= n1
    K[n1:, :n1] /= np.sqrt(n1)
    K[n1:, n1:] = 0
    K = np.tril(K) + np.tril(K, -1).T
    d = rng.uniform(0.5, 1.5, N)
    K[np.arange(n1), np.arange(n1)] = 1 + d[:n1]
    K[np.arange(n1, N), np.arange(n1, N)] = -d[n1:]
    if scaled:
        sc = np.exp(rng.uniform(-1.5, 1.5, N))
        K = K * sc[:, None] * sc[None, :]
    return K


@functools.lru_cache(maxsize=None)
def _reference(N):
    K = _qd(N, N)
    L_o, D_o = oracle.ldlt(K)
    b = np.random.default_rng(1).uniform(-1, 1, N)
    x_o = oracle.solve_ldlt(L_o, D_o, b)
    for a in (K, b, x_o):
        a.setflags(write=False)
    return K, b, x_o


@pytest.mark.parametrize("N", [100, 129, 513, 710, 1000, 1349])
def test_split_solve_vs_oracle_and_unsplit(ctx, N):
    K, b, x_o = _reference(N)
    L, D, info = I.LinearSolvers.ldlt_decomposition(K, ctx)
    assert info == 0
    x = {}
    for H in (1,) + SPLITS:
        I.debug_inject(MASK[H])
        x[H] = I.LinearSolvers.overwriting_solve_ldlt(L, D, b.copy(), ctx)
        I.debug_inject(0)
        err = np.abs(x[H] - x_o).max()
        print(f"N={N} H={H}: |x - x_oracle|_inf = {err:.3e}")
        assert err < TOL, (N, H, err)
    for H in SPLITS:
        assert np.array_equal(x[H], x[1]), (N, H, np.abs(x[H] - x[1]).max())


def _solve_sequence(ctx, K, rhs, H):
    """factor; three solves; factor again; one solve -- all in one workspace"""
    N = K.shape[0]
    wsb = ctx.workspace_bytes(N)
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda")
    D = torch.zeros(N, dtype=torch.float64, device="cuda")
    out = []
    I.debug_inject(MASK[H])
    try:
        for group in (rhs[:3], rhs[3:]):
            Kd = torch.from_numpy(np.tril(K)).cuda()
            torch.cuda.synchronize()  # torch's stream filled ws, D and Kd; the context runs on its own
            assert ctx.ldlt_factor(N, Kd.data_ptr(), N, D.data_ptr(), ws.data_ptr(), wsb) == 0
            for b in group:
                x = torch.from_numpy(b.copy()).cuda()
                torch.cuda.synchronize()
                ctx.ldlt_solve(N, Kd.data_ptr(), N, D.data_ptr(), ws.data_ptr(), x.data_ptr())
                ctx.sync()
                out.append(x.cpu().numpy())
    finally:
        I.debug_inject(0)
    return out


def test_consecutive_solves_and_refactor_reset_the_exchange(ctx):
    N = 710
    K = _qd(N, N)
    rhs = np.random.default_rng(2).uniform(-1, 1, (4, N))
    ref = _solve_sequence(ctx, K, rhs, 1)
    assert not np.array_equal(ref[0], ref[1])
    for H in SPLITS:
        got = _solve_sequence(ctx, K, rhs, H)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert np.all(np.isfinite(g)), (H, i)
            assert np.array_equal(g, r), (H, i, np.abs(g - r).max())


def _mixed(ctx, K, b, H):
    N = K.shape[0]
    Kd = torch.from_numpy(np.tril(K)).cuda()
    wsb = ctx.mixed_workspace_bytes(N)
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda")
    I.debug_inject(MASK[H])
    try:
        torch.cuda.synchronize()  # torch's stream filled ws and Kd; the context runs on its own
        assert ctx.mixed_factor(N, Kd.data_ptr(), N, ws.data_ptr(), wsb) == 0
        x = torch.from_numpy(b.copy()).cuda()
        torch.cuda.synchronize()
        ctx.mixed_solve(N, Kd.data_ptr(), N, ws.data_ptr(), x.data_ptr(), 1e-30, 0)
        torch.cuda.synchronize()
    finally:
        I.debug_inject(0)
    return x.cpu().numpy()


@pytest.mark.parametrize("N", [300, 1000])
def test_split_fp32_solve_bitwise(ctx, N):
    K = _qd(N, N, scaled=True)
    b = np.random.default_rng(3).uniform(-1, 1, N)
    ref = _mixed(ctx, K, b, 1)
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() > 0
    for H in SPLITS:
        got = _mixed(ctx, K, b, H)
        assert np.array_equal(got, ref), (N, H, np.abs(got - ref).max())


def _newton_step(ctx, H):
    I.debug_inject(MASK[H])
    try:
        g = I.Optimizer(300, 70, 30, ctx)
        g.generate(11)
        g.step()
        ctx.sync()
        out = g.daff().copy(), g.dir().copy()
        g.close()
    finally:
        I.debug_inject(0)
    return out


def test_newton_step_bitwise(ctx):
    daff, dirn = _newton_step(ctx, 1)
    assert np.all(np.isfinite(daff)) and np.all(np.isfinite(dirn)) and np.abs(dirn).max() > 0
    for H in SPLITS:
        a, d = _newton_step(ctx, H)
        assert np.array_equal(a, daff), (H, np.abs(a - daff).max())
        assert np.array_equal(d, dirn), (H, np.abs(d - dirn).max())
