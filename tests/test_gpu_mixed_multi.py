"""Mixed-precision multi-right-hand-side solve (ipmz_mixed_solve_multi,
ipmz_sym_residual_multi, ipmz_qp_kkt_solve_mixed) through the C ABI, against
fp64 numpy references.  Run on an MI355X: pytest -m gpu.

B holds one right-hand side per row.  Wherever a row is said to converge:
  * its reported ratio <= tol,
  * recomputed in numpy, max|b - K x| / max|b| <= 2 tol,
  * max|x - x_ref| / max|x_ref| <= 2 cond_inf(K) tol + 1e-13 (the forward-error
    bound for a relative residual in the same norm).

The matrix is the quasi-definite, badly scaled one of tests/test_gpu_mixed.py
at seed 11 + N; a numpy emulation of the algorithm (fp32 LDL^T of S K S, fp64
residual) reaches tol = 1e-12 on these inputs in at most 2 corrections, so
max_refine = 30 leaves the reference far inside the limit.

The cases that probe the kernels run with debug bit MULTI_BLOCKED (the blocked
path from 2 right-hand sides on) and without it (the public dispatch).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

MULTI_BLOCKED = 65536  # kernels.h IPMZ_DEBUG_MULTI_BLOCKED
TOL = 1e-12
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _qd(N, seed):
    """Quasi-definite symmetric test matrix with badly scaled rows / columns
    (tests/test_gpu_mixed.py)."""
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
    sc = np.exp(rng.uniform(-1.5, 1.5, N))
    return K * sc[:, None] * sc[None, :]


class Factor:
    """ipmz_mixed_factor of K (lower triangle, leading dimension ld) on the device."""

    def __init__(self, ctx, K, ld=None):
        N = K.shape[0]
        self.N, self.ctx = N, ctx
        self.ld = ld if ld is not None else N + (N & 1)
        Kp = np.zeros((N, self.ld))
        Kp[:, :N] = np.tril(K)
        self.K_host = Kp
        self.K = torch.from_numpy(Kp).cuda()
        self.wsb = ctx.mixed_workspace_bytes(N)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ctx.mixed_factor(N, self.K.data_ptr(), self.ld, self.ws.data_ptr(), self.wsb) == 0

    def solve_multi(self, B, tol=TOL, max_refine=30, forced=False, ldb=None, fill=0.0):
        """Rows of B solved on the device; returns the whole (nrhs, ldb) buffer and the stats."""
        nrhs, N = B.shape
        ldb = ldb if ldb is not None else N + (N & 1)
        Bp = np.full((nrhs, ldb), fill)
        Bp[:, :N] = B
        t = torch.from_numpy(Bp).cuda()
        mwsb = self.ctx.mixed_multi_workspace_bytes(N, nrhs)
        mws = torch.zeros(mwsb + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        I.debug_inject(MULTI_BLOCKED if forced else 0)
        try:
            stat = self.ctx.mixed_solve_multi(N, self.K.data_ptr(), self.ld, self.ws.data_ptr(), t.data_ptr(), ldb,
                                              nrhs, mws.data_ptr(), mwsb, tol, max_refine)
        finally:
            I.debug_inject(0)
        self.ctx.sync()
        return t.cpu().numpy(), stat

    def solve_single(self, b, tol=TOL, max_refine=30):
        t = torch.from_numpy(np.array(b)).cuda()
        torch.cuda.synchronize()
        ratio, iters = self.ctx.mixed_solve(self.N, self.K.data_ptr(), self.ld, self.ws.data_ptr(), t.data_ptr(), tol,
                                            max_refine)
        self.ctx.sync()
        return t.cpu().numpy(), ratio, iters

    def unchanged(self):
        return np.array_equal(self.K.cpu().numpy().view(np.int64), self.K_host.view(np.int64))


@functools.lru_cache(maxsize=None)
def _system(N):
    """K, 100 right-hand sides, their fp64 solutions and cond_inf(K) (once per
    order, never modified)."""
    K = _qd(N, 11 + N)
    B = np.random.default_rng(N).uniform(-1, 1, (100, N))
    X = np.linalg.solve(K, B.T).T.copy()
    cond = float(np.linalg.cond(K, np.inf))
    for a in (K, B, X):
        a.setflags(write=False)
    return K, B, X, cond


_FACTORS = {}


def _factor(ctx, N):
    """The device factor of _system(N), once per order."""
    if N not in _FACTORS:
        _FACTORS[N] = Factor(ctx, _system(N)[0])
    return _FACTORS[N]


_SINGLE = {}


def _single_counts(ctx, N, nrows):
    """Corrections ipmz_mixed_solve reports for the first nrows vectors of _system(N)."""
    have = _SINGLE.setdefault(N, [])
    f = _factor(ctx, N)
    B = _system(N)[1]
    while len(have) < nrows:
        have.append(f.solve_single(B[len(have)])[2])
    return np.array(have[:nrows])


def _accept(K, B, X, X_ref, stat, cond, tol, label, forward=True):
    """The per-row acceptance of a converged solve."""
    assert np.isfinite(X).all(), label
    for r in range(B.shape[0]):
        ratio = stat[r, 0]
        res = np.abs(B[r] - K @ X[r]).max() / np.abs(B[r]).max()
        print(label, "row", r, "ratio", ratio, "corrections", stat[r, 1], "recomputed", res)
        assert ratio <= tol, (label, r, ratio)
        assert res <= 2 * tol, (label, r, res)
        if forward:
            err = np.abs(X[r] - X_ref[r]).max() / np.abs(X_ref[r]).max()
            assert err <= 2 * cond * tol + 1e-13, (label, r, err, cond)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 300, 513, 556])
def test_ragged_orders(ctx, N, forced):
    K, B, X_ref, cond = _system(N)
    X, stat = _factor(ctx, N).solve_multi(B[:17], forced=forced)
    _accept(K, B[:17], X[:, :N], X_ref[:17], stat, cond, TOL, (N, forced))


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("N", [300, 556])
def test_ragged_rhs_counts(ctx, N, forced):
    K, B, X_ref, cond = _system(N)
    f = _factor(ctx, N)
    single = _single_counts(ctx, N, 100)
    for nrhs in (1, 2, 15, 16, 17, 33, 64, 65, 100):
        X, stat = f.solve_multi(B[:nrhs], forced=forced)
        assert stat.shape == (nrhs, 2)
        _accept(K, B[:nrhs], X[:, :N], X_ref[:nrhs], stat, cond, TOL, (N, nrhs, forced))
        # the project's own single-vector path as the yardstick: a wrong fp32
        # solve shows up as extra passes even when refinement rescues the answer
        assert np.all(stat[:, 1] <= single[:nrhs] + 1), (N, nrhs, forced, stat[:, 1], single[:nrhs])


@pytest.mark.parametrize("N", [300, 556])
def test_one_rhs_is_the_single_vector_solve(ctx, N):
    _, B, _, _ = _system(N)
    f = _factor(ctx, N)
    for forced in (False, True):
        X, stat = f.solve_multi(B[:1], forced=forced)
        x0, ratio, iters = f.solve_single(B[0])
        assert np.array_equal(X[0, :N].view(np.int64), x0.view(np.int64))
        assert stat[0, 0] == ratio and stat[0, 1] == iters


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("N", [300, 556])
def test_padding_and_k_untouched(ctx, N, forced):
    K, B, X_ref, cond = _system(N)
    f = Factor(ctx, K, ld=N + 2)
    ldb = N + 6
    X, stat = f.solve_multi(B[:17], forced=forced, ldb=ldb, fill=np.nan)
    pad = np.full((17, ldb - N), np.nan)
    assert np.array_equal(X[:, N:].view(np.int64), pad.view(np.int64)), "pad columns of B were written"
    assert f.unchanged(), "K was written"
    _accept(K, B[:17], X[:, :N], X_ref[:17], stat, cond, TOL, (N, forced))


def test_freeze_and_max_refine(ctx):
    N, tol = 556, 3e-12
    K, B, X_ref, cond = _system(N)
    f = _factor(ctx, N)
    X, stat = f.solve_multi(B, tol=tol, forced=True)
    _accept(K, B, X[:, :N], X_ref, stat, cond, tol, "freeze")
    c = stat[:, 1].astype(int)
    print("corrections per row:", np.bincount(c))
    if c.max() - 1 >= 0:
        mr = c.max() - 1
        X2, stat2 = f.solve_multi(B, tol=tol, max_refine=mr, forced=True)
        early = c <= mr
        assert np.array_equal(X2[early].view(np.int64), X[early].view(np.int64)), "a frozen row moved"
        assert np.array_equal(stat2[early].view(np.int64), stat[early].view(np.int64))
        assert np.all(stat2[~early, 1] == mr) and np.all(stat2[~early, 0] > tol)
    # a tolerance nothing reaches: every row runs all corrections and follows its reported ratio
    X3, stat3 = f.solve_multi(B, tol=1e-30, max_refine=3, forced=True)
    assert np.all(stat3[:, 1] == 3) and np.all(stat3[:, 0] > 1e-30)
    for r in range(100):
        err = np.abs(X3[r, :N] - X_ref[r]).max() / np.abs(X_ref[r]).max()
        assert err <= 2 * cond * stat3[r, 0] + 1e-13, (r, err, stat3[r, 0], cond)


def test_rows_are_independent(ctx):
    N = 556
    K, B, X_ref, cond = _system(N)
    f = _factor(ctx, N)
    X100, stat100 = f.solve_multi(B, forced=True)
    X17, stat17 = f.solve_multi(B[:17], forced=True)
    assert np.array_equal(X100[:17].view(np.int64), X17.view(np.int64))
    assert np.array_equal(stat100[:17].view(np.int64), stat17.view(np.int64))
    # a batch that is zero except for one row
    Bz = np.zeros((40, N))
    Bz[38] = B[5]
    Xz, statz = f.solve_multi(Bz, forced=True)
    others = np.delete(Xz[:, :N], 38, axis=0)
    assert np.all(others == 0.0), "a zero right-hand side picked up another row's data"
    assert np.all(np.delete(statz, 38, axis=0) == 0.0)
    _accept(K, B[5:6], Xz[38:39, :N], X_ref[5:6], statz[38:39], cond, TOL, "one row")
    # two identical calls
    Xa, stata = f.solve_multi(B[:33], forced=True)
    Xb, statb = f.solve_multi(B[:33], forced=True)
    assert np.array_equal(Xa.view(np.int64), Xb.view(np.int64))
    assert np.array_equal(stata.view(np.int64), statb.view(np.int64))


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [1, 17, 100])
@pytest.mark.parametrize("N", [65, 300, 556])
def test_sym_residual_multi(ctx, N, nrhs):
    K, B, _, _ = _system(N)
    B = B[:nrhs]
    X = np.random.default_rng(5 * N + nrhs).uniform(-1, 1, (nrhs, N))
    ld = N + (N & 1)

    def pad(a, fill=0.0):
        out = np.full((a.shape[0], ld), fill)
        out[:, :a.shape[1]] = a
        return out

    Kl = pad(np.tril(K))
    Kl[:, :N][np.triu_indices(N, 1)] = np.nan  # the upper triangle is never read
    Kd, Xd, Bd = (torch.from_numpy(a).cuda() for a in (Kl, pad(X), pad(B, np.nan)))
    Rd = torch.full((nrhs, ld), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.sym_residual_multi(N, Kd.data_ptr(), ld, Xd.data_ptr(), ld, Bd.data_ptr(), ld, Rd.data_ptr(), ld, nrhs)
    ctx.sync()
    R = Rd.cpu().numpy()
    assert np.isnan(R[:, N:]).all(), "pad columns of R were written"
    R = R[:, :N]
    # the standard dot-product bound with slack 4, plus the final subtraction's rounding
    bound = 4 * N * EPS * (np.abs(X) @ np.abs(K)) + EPS * np.abs(B)
    diff = np.abs(R - (B - X @ K))
    print("max diff / bound:", (diff / bound).max())
    assert np.isfinite(R).all() and np.all(diff <= bound)
    # R aliasing B
    ctx.sym_residual_multi(N, Kd.data_ptr(), ld, Xd.data_ptr(), ld, Bd.data_ptr(), ld, Bd.data_ptr(), ld, nrhs)
    ctx.sync()
    assert np.array_equal(Bd.cpu().numpy()[:, :N].view(np.int64), R.view(np.int64))


# ---------------------------------------------------------------------------
def test_arguments(ctx):
    N = 64
    _, B, _, _ = _system(N)
    f = _factor(ctx, N)
    t = torch.from_numpy(np.array(B[:4])).cuda()
    before = t.clone()
    mwsb = ctx.mixed_multi_workspace_bytes(N, 4)
    assert mwsb > 0
    mws = torch.zeros(mwsb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    K, ld, ws = f.K.data_ptr(), f.ld, f.ws.data_ptr()
    assert ctx.mixed_solve_multi(N, K, ld, ws, t.data_ptr(), N, 0, mws.data_ptr(), mwsb).shape == (0, 2)  # nrhs = 0
    ctx.mixed_solve_multi(0, 0, 0, 0, 0, 0, 3, 0, 0)  # N = 0: no-op
    ctx.sync()
    assert torch.equal(t, before)
    I.debug_inject(MULTI_BLOCKED)
    try:
        with pytest.raises(I.IpmzError):
            ctx.mixed_solve_multi(N, K, ld, ws, t.data_ptr(), N - 2, 4, mws.data_ptr(), mwsb)  # ldb < N
        with pytest.raises(I.IpmzError):
            ctx.mixed_solve_multi(N, K, ld, ws, t.data_ptr(), N + 1, 2, mws.data_ptr(), mwsb)  # odd ldb
        with pytest.raises(I.IpmzError):
            ctx.mixed_solve_multi(N, K, ld + 1, ws, t.data_ptr(), N, 4, mws.data_ptr(), mwsb)  # odd ld
        with pytest.raises(I.IpmzError):
            ctx.mixed_solve_multi(N, K, ld, ws, t.data_ptr(), N, -1, mws.data_ptr(), mwsb)  # negative nrhs
        with pytest.raises(I.IpmzError):
            ctx.mixed_solve_multi(N, K, ld, ws, 0, N, 4, mws.data_ptr(), mwsb)  # null B
        with pytest.raises(I.IpmzError, match="workspace too small"):
            ctx.mixed_solve_multi(N, K, ld, ws, t.data_ptr(), N, 4, mws.data_ptr(), mwsb - 1)  # short mws
        with pytest.raises(I.IpmzError):
            ctx.mixed_solve_multi(N, K, ld, ws, t.data_ptr(), N, 4, mws.data_ptr(), mwsb, max_refine=-1)
    finally:
        I.debug_inject(0)
    ctx.sync()
    assert torch.equal(t, before)


def test_refused_during_graph_capture():
    N = 64
    K, B, _, _ = _system(N)
    s = torch.cuda.Stream()
    c = I.Context(0, stream=s.cuda_stream)
    try:
        f = Factor(c, K)
        t = torch.from_numpy(np.array(B[:4])).cuda()
        before = t.clone()
        z = torch.zeros(8, device="cuda")
        mwsb = c.mixed_multi_workspace_bytes(N, 4)
        mws = torch.zeros(mwsb, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            z.add_(1.0)
            with pytest.raises(I.IpmzError, match="bad state.*capturing a hipGraph"):
                c.mixed_solve_multi(N, f.K.data_ptr(), f.ld, f.ws.data_ptr(), t.data_ptr(), N, 4, mws.data_ptr(), mwsb)
        # the capture ended cleanly: it replays, and the call works again
        g.replay()
        torch.cuda.synchronize()
        assert z[0].item() == 1.0
        assert torch.equal(t, before)
        stat = c.mixed_solve_multi(N, f.K.data_ptr(), f.ld, f.ws.data_ptr(), t.data_ptr(), N, 4, mws.data_ptr(), mwsb)
        assert np.all(stat[:, 0] <= 1e-12)
    finally:
        c.close()


# ---------------------------------------------------------------------------
# QP level: ipmz_qp_kkt_solve_mixed
QP = dict(n=48, m=16, p=8)  # N = 72


def _sym(Kl):
    return Kl + np.tril(Kl, -1).T


@pytest.mark.parametrize("mixed_steps", [False, True])
@pytest.mark.parametrize("forced", [False, True])
def test_qp_kkt_solve_mixed_vs_numpy(ctx, forced, mixed_steps):
    g = I.Optimizer(ctx=ctx, **QP)
    g.generate(21)
    if mixed_steps:
        g.set_mixed_precision(True)
    g.step()
    g.step()
    N = g.N
    assert N == 72
    B = np.random.default_rng(3).uniform(-1, 1, (12, N))
    t = torch.from_numpy(B.copy()).cuda()
    torch.cuda.synchronize()
    I.debug_inject(MULTI_BLOCKED if forced else 0)
    try:
        info, stat = g.kkt_solve_mixed(t.data_ptr(), 12, N, tol=TOL, max_refine=30)
    finally:
        I.debug_inject(0)
    assert info == 0 and stat.shape == (12, 2)
    K = _sym(g.kkt())
    X_ref = np.linalg.solve(K, B.T).T
    _accept(K, B, t.cpu().numpy(), X_ref, stat, float(np.linalg.cond(K, np.inf)), TOL, ("qp", forced, mixed_steps))


@pytest.mark.parametrize("mixed_steps", [False, True])
def test_qp_kkt_solve_mixed_leaves_the_steps_unchanged(ctx, mixed_steps):
    a = I.Optimizer(ctx=ctx, **QP)
    b = I.Optimizer(ctx=ctx, **QP)
    a.generate(22)
    b.generate(22)
    if mixed_steps:
        a.set_mixed_precision(True)
        b.set_mixed_precision(True)
    rhs = np.random.default_rng(4).uniform(-1, 1, (12, a.N))
    for it in range(3):
        t = torch.from_numpy(rhs.copy()).cuda()
        torch.cuda.synchronize()
        a.kkt_solve_mixed(t.data_ptr(), 12 if it != 1 else 5, a.N)
        a.step()
        b.step()
        assert np.array_equal(a.vars().view(np.int64), b.vars().view(np.int64)), it
        sa, sb = a.scalars(), b.scalars()
        assert list(sa) == list(sb)
        assert np.array_equal(np.array(list(sa.values())).view(np.int64),
                              np.array(list(sb.values())).view(np.int64)), it


def test_qp_kkt_solve_mixed_unsupported(ctx):
    t = torch.zeros(2, 80, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    batch = I.Batch(batch=2, ctx=ctx, **QP)
    batch.generate(1)
    with pytest.raises(I.IpmzError, match="batch"):
        batch.kkt_solve_mixed(t.data_ptr(), 2, 80)
    none = I.Optimizer(ctx=ctx, equality_handling=I.EQ_NONE, **QP)
    none.generate(1)
    with pytest.raises(I.IpmzError, match="Bunch-Kaufman"):
        none.kkt_solve_mixed(t.data_ptr(), 2, 80)
    normal = I.Optimizer(ctx=ctx, **QP)
    normal.generate(1)
    normal.set_reduction(I.REDUCTION_NORMAL)
    with pytest.raises(I.IpmzError, match="normal-equations"):
        normal.kkt_solve_mixed(t.data_ptr(), 2, 80)
    for eq in (I.EQ_PENALTY, I.EQ_PENALTY_EXTRA_DUAL):
        pen = I.Optimizer(ctx=ctx, equality_handling=eq, **QP)
        pen.generate(1)
        with pytest.raises(I.IpmzError, match="PenaltyFunction"):
            pen.kkt_solve_mixed(t.data_ptr(), 2, 80)


# ---------------------------------------------------------------------------
def test_mid_size(ctx):
    # ten 256-column panels; the residual checks, and the looped single-vector solve as the reference
    N, nrhs = 2560, 40
    K = _qd(N, 11 + N)
    B = np.random.default_rng(N).uniform(-1, 1, (100, N))[:nrhs]
    f = Factor(ctx, K)
    X, stat = f.solve_multi(B)
    _accept(K, B, X, None, stat, None, TOL, "N = 2560", forward=False)
    for r in range(nrhs):
        x1 = f.solve_single(B[r])[0]
        assert np.abs(X[r] - x1).max() <= 1e-10 * max(1.0, np.abs(x1).max()), r
