"""Multi-right-hand-side normal-equations solve (ipmz_normal_factor +
ipmz_normal_solve_multi) against the CPU oracle's LDL^T solve of the same
quasi-definite matrix, row by row.  Run on an MI355X: pytest -m gpu.

The systems are those of tests/test_gpu_solve_multi.py (x block first: a
positive definite leading block of order n, a negative diagonal trailing block
of order mp), the tolerance the project's rule for blocked solves,
|x - x_ref|_inf < 1e-10 max(1, |x_ref|_inf) per row.
"""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

TOL = 1e-10
MULTI_BLOCKED = 65536  # kernels.h IPMZ_DEBUG_MULTI_BLOCKED
SHAPES = [(225, 75), (417, 139)]  # N = 300; N = 556: three 256-column panels, the last one ragged


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _qd(N, seed):
    """Quasi-definite: positive definite leading block, negative diagonal trailing block."""
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
    return K


@functools.lru_cache(maxsize=None)
def _system(N):
    K = _qd(N, N)
    L, D = oracle.ldlt(K)
    B = np.random.default_rng(1000 + N).uniform(-1, 1, (100, N))
    X = np.stack([oracle.solve_ldlt(L, D, b) for b in B])
    for a in (K, B, X):
        a.setflags(write=False)
    return K, B, X


class Normal:
    """ipmz_normal_factor of K on the device."""

    def __init__(self, ctx, K, n):
        N = K.shape[0]
        assert (3 * N + 3) // 4 == n  # _qd's leading block is the x block
        self.ctx, self.n, self.mp, self.N = ctx, n, N - n, N
        self.K = torch.from_numpy(np.tril(K)).cuda()
        self.D = torch.zeros(N, dtype=torch.float64, device="cuda")
        self.wsb = ctx.normal_workspace_bytes(n, N - n)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ctx.normal_factor(n, N - n, self.K.data_ptr(), N, self.D.data_ptr(), self.ws.data_ptr(), self.wsb) == 0

    def _run(self, B, call):
        t = torch.from_numpy(np.array(B)).cuda()
        torch.cuda.synchronize()
        call(t)
        self.ctx.sync()
        return t.cpu().numpy()

    def solve_multi(self, B):
        return self._run(B, lambda t: self.ctx.normal_solve_multi(
            self.n, self.mp, self.K.data_ptr(), self.N, self.D.data_ptr(), self.ws.data_ptr(), t.data_ptr(), self.N,
            B.shape[0]))

    def solve_single(self, b):
        return self._run(b, lambda t: self.ctx.normal_solve(
            self.n, self.mp, self.K.data_ptr(), self.N, self.D.data_ptr(), self.ws.data_ptr(), t.data_ptr()))


def _check_rows(X, X_ref, label=""):
    assert np.isfinite(X).all(), label
    for r in range(X_ref.shape[0]):
        err = np.abs(X[r] - X_ref[r]).max()
        scale = max(1.0, np.abs(X_ref[r]).max())
        assert err < TOL * scale, (label, r, err, scale)


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("n,mp", SHAPES)
def test_normal_solve_multi_vs_oracle(ctx, n, mp, forced):
    K, B, X_ref = _system(n + mp)
    f = Normal(ctx, K, n)
    I.debug_inject(MULTI_BLOCKED if forced else 0)
    try:
        for nrhs in (17, 100):
            _check_rows(f.solve_multi(B[:nrhs]), X_ref[:nrhs], (n, mp, nrhs, forced))
    finally:
        I.debug_inject(0)


@pytest.mark.parametrize("n,mp", SHAPES)
def test_one_row_is_normal_solve_bitwise(ctx, n, mp):
    K, B, _ = _system(n + mp)
    f = Normal(ctx, K, n)
    x1 = f.solve_multi(B[:1])
    assert np.array_equal(x1[0].view(np.int64), f.solve_single(B[0]).view(np.int64))


def test_bad_arguments(ctx):
    n, mp = SHAPES[0]
    K, B, _ = _system(n + mp)
    f = Normal(ctx, K, n)
    N = f.N
    t = torch.zeros(4, N + 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    args = (n, mp, f.K.data_ptr(), N, f.D.data_ptr(), f.ws.data_ptr())
    with pytest.raises(I.IpmzError, match="invalid argument"):  # odd ldb
        ctx.normal_solve_multi(*args, t.data_ptr(), N + 1, 2)
    with pytest.raises(I.IpmzError, match="16-byte aligned"):
        ctx.normal_solve_multi(*args, t.data_ptr() + 8, N + 2, 2)
    with pytest.raises(I.IpmzError, match="invalid argument"):  # negative nrhs
        ctx.normal_solve_multi(*args, t.data_ptr(), N + 2, -1)
    assert ctx.normal_solve_multi(*args, t.data_ptr(), N + 2, 0) == 0
    ctx.sync()
    assert not t.cpu().numpy().any()
