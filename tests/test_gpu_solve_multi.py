"""Multi-right-hand-side LDL^T solve (ipmz_ldlt_solve_multi, the host
signature ipmz_overwriting_solve_ldlt_multi, ipmz_qp_kkt_solve) against the
CPU oracle, column by column.  Run on an MI355X: pytest -m gpu.

B holds one right-hand side per row.  Tolerance: the project's rule for
blocked solves, |x - x_ref|_inf < 1e-10 max(1, |x_ref|_inf), per row.

The blocked path runs from a crossover number of right-hand sides on (below it
the rows go through the single-vector solve one by one); the cases that probe
the kernels' ragged right-hand-side counts run a second time with debug bit
MULTI_BLOCKED, which sends every nrhs >= 2 through the blocked kernels.
"""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

TOL = 1e-10  # DX_TOL of tests/test_gpu_parity.py
MULTI_BLOCKED = 65536  # kernels.h IPMZ_DEBUG_MULTI_BLOCKED
W = I.SOLVE_MULTI_PANEL
N3 = 2 * W + W // 8 + 12  # three panels, the last one ragged (556 for 256-column panels)
BLOCKINGS = [(256, 64), (256, 128), (128, 64)]


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
    """K, the oracle's factor of it and 100 right-hand sides with their oracle
    solutions (computed once per order, never modified)."""
    K = _qd(N, N)
    L, D = oracle.ldlt(K)
    B = np.random.default_rng(1000 + N).uniform(-1, 1, (100, N))
    X = np.stack([oracle.solve_ldlt(L, D, b) for b in B])
    for a in (K, L, D, B, X):
        a.setflags(write=False)
    return K, L, D, B, X


class Factor:
    """ipmz_ldlt_factor of K on the device with leading dimension ld."""

    def __init__(self, ctx, K, ld=None):
        N = K.shape[0]
        self.N, self.ctx = N, ctx
        self.ld = ld if ld is not None else N + (N & 1)
        Kp = np.zeros((N, self.ld))
        Kp[:, :N] = K
        self.K = torch.from_numpy(Kp).cuda()
        self.D = torch.zeros(N, dtype=torch.float64, device="cuda")
        self.wsb = ctx.workspace_bytes(N)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ctx.ldlt_factor(N, self.K.data_ptr(), self.ld, self.D.data_ptr(), self.ws.data_ptr(), self.wsb) == 0

    def solve_multi(self, B, ldb=None, fill=0.0):
        """Rows of B solved on the device; returns the whole (nrhs, ldb) buffer."""
        nrhs, N = B.shape
        ldb = ldb if ldb is not None else N + (N & 1)
        Bp = np.full((nrhs, ldb), fill)
        Bp[:, :N] = B
        t = torch.from_numpy(Bp).cuda()
        torch.cuda.synchronize()
        self.ctx.ldlt_solve_multi(N, self.K.data_ptr(), self.ld, self.D.data_ptr(), self.ws.data_ptr(), t.data_ptr(),
                                  ldb, nrhs)
        self.ctx.sync()
        return t.cpu().numpy()

    def solve_single(self, b):
        t = torch.from_numpy(np.array(b)).cuda()
        torch.cuda.synchronize()
        self.ctx.ldlt_solve(self.N, self.K.data_ptr(), self.ld, self.D.data_ptr(), self.ws.data_ptr(), t.data_ptr())
        self.ctx.sync()
        return t.cpu().numpy()


def _check_rows(X, X_ref, label=""):
    assert np.isfinite(X).all(), label
    for r in range(X_ref.shape[0]):
        err = np.abs(X[r] - X_ref[r]).max()
        scale = max(1.0, np.abs(X_ref[r]).max())
        assert err < TOL * scale, (label, r, err, scale)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("blocking", BLOCKINGS)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 127, 129, 300, 513, N3])
def test_ragged_orders(ctx, N, blocking):
    K, _, _, B, X_ref = _system(N)
    ctx.set_blocking(*blocking)
    try:
        X = Factor(ctx, K).solve_multi(B[:17])
        _check_rows(X[:, :N], X_ref[:17], (N, blocking))
    finally:
        ctx.set_blocking(256, 64)


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("N", [300, N3])
def test_ragged_rhs_counts(ctx, N, forced):
    K, _, _, B, X_ref = _system(N)
    f = Factor(ctx, K)
    I.debug_inject(MULTI_BLOCKED if forced else 0)
    try:
        for nrhs in (1, 2, 15, 16, 17, 33, 64, 100):
            X = f.solve_multi(B[:nrhs])
            _check_rows(X[:, :N], X_ref[:nrhs], (N, nrhs, forced))
    finally:
        I.debug_inject(0)


@pytest.mark.parametrize("blocking", [(256, 64), (256, 128)])
@pytest.mark.parametrize("N", [300, N3])
def test_padding_untouched(ctx, N, blocking):
    K, _, _, B, X_ref = _system(N)
    ctx.set_blocking(*blocking)
    try:
        ldb = N + 6
        X = Factor(ctx, K, ld=N + 2).solve_multi(B[:17], ldb=ldb, fill=np.nan)
    finally:
        ctx.set_blocking(256, 64)
    pad = np.full((17, ldb - N), np.nan)
    assert np.array_equal(X[:, N:].view(np.int64), pad.view(np.int64)), "pad columns of B were written"
    _check_rows(X[:, :N], X_ref[:17], (N, blocking))


@pytest.mark.parametrize("N", [300, N3])
def test_one_rhs_is_the_single_vector_solve(ctx, N):
    K, _, _, B, _ = _system(N)
    f = Factor(ctx, K)
    x1 = f.solve_multi(B[:1])[0, :N]
    x0 = f.solve_single(B[0])
    assert np.array_equal(x1.view(np.int64), x0.view(np.int64))


@pytest.mark.parametrize("N", [300, N3])
def test_rows_are_independent(ctx, N):
    K, _, _, B, X_ref = _system(N)
    f = Factor(ctx, K)
    got = []
    for nrhs, r in ((17, 3), (40, 38)):
        Bz = np.zeros((nrhs, N))
        Bz[r] = B[5]
        X = f.solve_multi(Bz)[:, :N]
        others = np.delete(X, r, axis=0)
        assert np.all(others == 0.0), "a zero right-hand side picked up another row's data"
        _check_rows(X[r:r + 1], X_ref[5:6], (N, nrhs, r))
        got.append(X[r])
    _check_rows(got[0][None], got[1][None], "same vector, other row position and nrhs")


def test_deterministic(ctx):
    K, _, _, B, _ = _system(1100)
    f = Factor(ctx, K)
    a = f.solve_multi(B[:33])
    b = f.solve_multi(B[:33])
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_device_factor_torch_tensors_on_torch_stream(ctx):
    # ipmz_ldlt_factor's own factor, everything enqueued on torch's stream
    N, nrhs = N3, 24
    K, _, _, B, X_ref = _system(N)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        Kd = torch.from_numpy(np.array(K)).cuda()
        D = torch.zeros(N, dtype=torch.float64, device="cuda")
        wsb = ctx.workspace_bytes(N)
        ws = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda")
        assert ctx.ldlt_factor(N, Kd.data_ptr(), N, D.data_ptr(), ws.data_ptr(), wsb) == 0
        X = torch.from_numpy(np.array(B[:nrhs])).cuda()
        ctx.ldlt_solve_multi(N, Kd.data_ptr(), N, D.data_ptr(), ws.data_ptr(), X.data_ptr(), N, nrhs)
        torch.cuda.synchronize()
        ctx.sync()
        _check_rows(X.cpu().numpy(), X_ref[:nrhs])
        # residual against the unfactored matrix, on the device: a backward-stable
        # solve leaves about N eps |K| |x|, eps = 1.1e-16, |K| <= 2.5; 1e-13 N |x| is ~400 times that
        R = X @ torch.from_numpy(np.array(K)).cuda() - torch.from_numpy(np.array(B[:nrhs])).cuda()
        assert R.abs().max().item() < 1e-13 * N * max(1.0, X.abs().max().item())
    finally:
        ctx.set_stream(None)


@pytest.mark.parametrize("N,nrhs", [(300, 17), (N3, 20), (65, 3)])
def test_host_signature_with_oracle_factor(ctx, N, nrhs):
    # ipmz_ldlt_prepare_solve on the oracle's L, through the host signature
    _, L, D, B, X_ref = _system(N)
    Bc = np.array(B[:nrhs])
    X = I.LinearSolvers.overwriting_solve_ldlt_multi(L, D, Bc, ctx)
    assert X is Bc
    _check_rows(X, X_ref[:nrhs], (N, nrhs))
    with pytest.raises(I.IpmzError, match="size mismatch"):
        I.LinearSolvers.overwriting_solve_ldlt_multi(L, D, np.zeros((2, N + 1)), ctx)
    with pytest.raises(I.IpmzError):
        I.LinearSolvers.overwriting_solve_ldlt_multi(L, D, np.zeros(N), ctx)


def test_mid_size_against_single_vector_solve(ctx):
    # C2's order: several panels; the project's own solve is the reference
    N, nrhs = 2560, 40
    K = _qd(N, 2560)
    f = Factor(ctx, K)
    B = np.random.default_rng(7).uniform(-1, 1, (nrhs, N))
    X = f.solve_multi(B)
    X_ref = np.stack([f.solve_single(b) for b in B])
    _check_rows(X, X_ref, "N = 2560")


def test_arguments(ctx):
    N = 64
    K, _, _, B, _ = _system(N)
    f = Factor(ctx, K)
    t = torch.from_numpy(np.array(B[:4])).cuda()
    before = t.clone()
    args = (f.K.data_ptr(), f.ld, f.D.data_ptr(), f.ws.data_ptr(), t.data_ptr())
    torch.cuda.synchronize()
    assert ctx.ldlt_solve_multi(N, *args, N, 0) == 0  # nrhs = 0: no-op
    assert ctx.ldlt_solve_multi(0, 0, 0, 0, 0, 0, 0, 3) == 0  # N = 0: no-op
    ctx.sync()
    assert torch.equal(t, before)
    with pytest.raises(I.IpmzError):
        ctx.ldlt_solve_multi(N, *args, N - 2, 4)  # ldb < N
    with pytest.raises(I.IpmzError):
        ctx.ldlt_solve_multi(N, *args, N + 1, 2)  # odd ldb
    with pytest.raises(I.IpmzError):
        ctx.ldlt_solve_multi(N, *args, N, -1)  # negative nrhs
    with pytest.raises(I.IpmzError):
        ctx.ldlt_solve_multi(N, f.K.data_ptr(), f.ld, f.D.data_ptr(), f.ws.data_ptr(), 0, N, 4)  # null B
    ctx.sync()
    assert torch.equal(t, before)


# ---------------------------------------------------------------------------
# QP level: ipmz_qp_kkt_solve
QP = dict(n=48, m=16, p=8)  # N = 72: two inner blocks


def _sym(Kl):
    return Kl + np.tril(Kl, -1).T


@pytest.mark.parametrize("forced", [False, True])
def test_qp_kkt_solve_vs_oracle(ctx, forced):
    g = I.Optimizer(ctx=ctx, **QP)
    g.generate(21)
    g.step()
    g.step()
    N = g.N
    assert N == 72
    B = np.random.default_rng(3).uniform(-1, 1, (5, N))
    t = torch.from_numpy(B.copy()).cuda()
    torch.cuda.synchronize()
    I.debug_inject(MULTI_BLOCKED if forced else 0)
    try:
        assert g.kkt_solve(t.data_ptr(), 5, N) == 0
    finally:
        I.debug_inject(0)
    L, D = oracle.ldlt(_sym(g.kkt()))
    X_ref = np.stack([oracle.solve_ldlt(L, D, b) for b in B])
    _check_rows(t.cpu().numpy(), X_ref, forced)


def test_qp_kkt_solve_leaves_the_steps_unchanged(ctx):
    a = I.Optimizer(ctx=ctx, **QP)
    b = I.Optimizer(ctx=ctx, **QP)
    a.generate(22)
    b.generate(22)
    t = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (5, a.N))).cuda()
    torch.cuda.synchronize()
    for it in range(3):
        a.kkt_solve(t.data_ptr(), 5, a.N)
        a.step()
        b.step()
        assert np.array_equal(a.vars().view(np.int64), b.vars().view(np.int64)), it
        sa, sb = a.scalars(), b.scalars()
        assert list(sa) == list(sb)
        assert np.array_equal(np.array(list(sa.values())).view(np.int64),
                              np.array(list(sb.values())).view(np.int64)), it


def test_qp_kkt_solve_unsupported(ctx):
    t = torch.zeros(2, 80, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    batch = I.Batch(batch=2, ctx=ctx, **QP)
    batch.generate(1)
    with pytest.raises(I.IpmzError, match="batch"):
        batch.kkt_solve(t.data_ptr(), 2, 80)
    none = I.Optimizer(ctx=ctx, equality_handling=I.EQ_NONE, **QP)
    none.generate(1)
    with pytest.raises(I.IpmzError, match="Bunch-Kaufman"):
        none.kkt_solve(t.data_ptr(), 2, 80)
    normal = I.Optimizer(ctx=ctx, **QP)
    normal.generate(1)
    normal.set_reduction(I.REDUCTION_NORMAL)
    with pytest.raises(I.IpmzError, match="normal-equations"):
        normal.kkt_solve(t.data_ptr(), 2, 80)
    mixed = I.Optimizer(ctx=ctx, **QP)
    mixed.generate(1)
    mixed.set_mixed_precision(True)
    with pytest.raises(I.IpmzError, match="mixed precision"):
        mixed.kkt_solve(t.data_ptr(), 2, 80)
    # and switched back off, the same solver is served
    mixed.set_mixed_precision(False)
    assert mixed.kkt_solve(t.data_ptr(), 2, 80) == 0
