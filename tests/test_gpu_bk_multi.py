"""Multi-right-hand-side Bunch-Kaufman solve (ipmz_bk_prepare_solve +
ipmz_bk_solve_multi, the host signature
ipmz_overwriting_solve_bunch_kaufman_multi, ipmz_qp_kkt_solve_bk) against the
CPU oracle's reference-order solve, row by row.  Run on an MI355X: pytest -m gpu.

B holds one right-hand side per row.  Tolerance: the project's rule for
blocked solves, |x - x_ref|_inf < 1e-10 max(1, |x_ref|_inf), per row.  On
these systems a CPU LU solve (other pivoting, other summation order) differs
from the oracle by at most 6.3e-12 in that measure (kktz(700, 300, 701)); the
two QP matrices below by 1.6e-15 (N = 72) and 3.7e-15 (N = 520).

The blocked path runs from a crossover number of right-hand sides on (below it
the rows go through ipmz_bk_solve's launches one by one); debug bit
MULTI_BLOCKED sends every nrhs >= 2 through the blocked kernels.  The factor
uploaded is the oracle's: the device factor is bitwise that one
(tests/test_gpu_bk.py), and this file is about the solve.
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
MULTI_W128 = 262144  # kernels.h IPMZ_DEBUG_MULTI_W128
BELOW = 4  # a count below the crossover of either multi-right-hand-side solve
FILL = -7.25  # sentinel of the pad columns


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _indef(N, seed, zeros=0):
    rng = np.random.default_rng(seed)
    K = rng.uniform(-1, 1, (N, N))
    K = np.tril(K) + np.tril(K, -1).T
    K[np.arange(N), np.arange(N)] *= 0.05
    for z in range(zeros):
        K[N // 2 + z, :] = 0
        K[:, N // 2 + z] = 0
    return K


def _kkt_zero_block(n, m, seed):
    # [[H, B^T], [B, 0]]: the zero block forces interchanges and 2x2 pivots
    rng = np.random.default_rng(seed)
    H = rng.uniform(-1, 1, (n, n))
    H = H + H.T
    H[np.arange(n), np.arange(n)] *= 0.01  # weak diagonal: interchanges and 2x2 pivots
    B = rng.uniform(-1, 1, (m, n))
    K = np.zeros((n + m, n + m))
    K[:n, :n] = H
    K[n:, :n] = B
    K[:n, n:] = B.T
    return K


@functools.lru_cache(maxsize=None)
def _system(kind, a, b=0, c=0, rows=17):
    """K, the oracle's factor of it, 100 right-hand sides and the oracle's
    solutions of the first `rows` of them (computed once, never modified)."""
    K = _indef(a, b, c) if kind == "indef" else _kkt_zero_block(a, b, c)
    N = K.shape[0]
    Fo, po, info = oracle.bk_factor(K)
    po = po.astype(np.int32)
    B = np.random.default_rng(1000 + N).uniform(-1, 1, (100, N))
    X = np.stack([oracle.bk_solve(Fo, po, r) for r in B[:rows]]) if rows else np.zeros((0, N))
    for arr in (K, Fo, po, B, X):
        arr.setflags(write=False)
    return K, Fo, po, info, B, X


def _pair_starts(po):
    out, k = [], 0
    while k < len(po):
        if po[k] < 0:
            out.append(k)
            k += 2
        else:
            k += 1
    return out


class Prepared:
    """F and ipiv on the device (leading dimension ld) and the prepared solve."""

    def __init__(self, ctx, F, ipiv, ld=None):
        N = F.shape[0]
        self.N, self.ctx = N, ctx
        self.ld = ld if ld is not None else N
        Fp = np.zeros((N, self.ld))
        Fp[:, :N] = F
        self.F = torch.from_numpy(Fp).cuda()
        self.piv = torch.from_numpy(np.array(ipiv, dtype=np.int32)).cuda()
        self.wsb = ctx.bk_solve_workspace_bytes(N)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.bk_prepare_solve(N, self.F.data_ptr(), self.ld, self.piv.data_ptr(), self.ws.data_ptr(), self.wsb)
        ctx.sync()

    def solve_multi(self, B, ldb=None, fill=0.0, debug=0):
        """Rows of B solved on the device; returns the whole (nrhs, ldb) buffer."""
        nrhs, N = B.shape
        ldb = ldb if ldb is not None else N + (N & 1)
        Bp = np.full((nrhs, ldb), fill)
        Bp[:, :N] = B
        t = torch.from_numpy(Bp).cuda()
        torch.cuda.synchronize()
        I.debug_inject(debug)
        try:
            self.ctx.bk_solve_multi(N, self.F.data_ptr(), self.ld, self.piv.data_ptr(), self.ws.data_ptr(),
                                    t.data_ptr(), ldb, nrhs)
            self.ctx.sync()
        finally:
            I.debug_inject(0)
        return t.cpu().numpy()

    def solve_single(self, b):
        """ipmz_bk_solve of one vector."""
        t = torch.from_numpy(np.array(b)).cuda()
        torch.cuda.synchronize()
        self.ctx.bk_solve(self.N, self.F.data_ptr(), self.ld, self.piv.data_ptr(), t.data_ptr())
        self.ctx.sync()
        return t.cpu().numpy()


def _check_rows(X, X_ref, label=""):
    assert np.isfinite(X).all(), label
    for r in range(X_ref.shape[0]):
        err = np.abs(X[r] - X_ref[r]).max()
        scale = max(1.0, np.abs(X_ref[r]).max())
        assert err < TOL * scale, (label, r, err, scale)


# ---------------------------------------------------------------------------
RAGGED = [("indef", N, N, 0) for N in (1, 2, 3, 63, 64, 65, 127, 129, 300, 513)]
RAGGED += [("kktz", 400, 156, 557),  # N = 556: three 256-column panels, the last one ragged
           ("kktz", 700, 300, 701)]


@pytest.mark.parametrize("key", RAGGED, ids=lambda k: "-".join(map(str, k)))
def test_ragged_orders(ctx, key):
    K, Fo, po, info, B, X_ref = _system(*key, rows=100 if key[-1] == 557 else 17)  # (557: shared with the tests below)
    N = K.shape[0]
    assert info == 0
    if N >= 63:  # both 2x2 pivots and interchanges
        assert (po < 0).any() and (po[po >= 0] != np.arange(N)[po >= 0]).any()
    X = Prepared(ctx, Fo, po).solve_multi(B[:17], debug=MULTI_BLOCKED)
    _check_rows(X[:, :N], X_ref[:17], key)


@pytest.mark.parametrize("width", [0, MULTI_W128])
@pytest.mark.parametrize("seed", [557, 558])
def test_pairs_across_block_and_panel_boundaries(ctx, seed, width):
    K, Fo, po, _, B, X_ref = _system("kktz", 400, 156, seed, rows=100 if seed == 557 else 33)
    N = K.shape[0]
    starts = _pair_starts(po)
    assert any(k % 64 == 63 for k in starts), starts  # a pair across a 64-column block boundary
    assert any(k % 256 == 255 for k in starts), starts  # ... and across a 256-column panel boundary
    X = Prepared(ctx, Fo, po).solve_multi(B[:33], debug=MULTI_BLOCKED | width)
    _check_rows(X[:, :N], X_ref[:33], (seed, width))


@pytest.mark.parametrize("forced", [False, True])
def test_ragged_rhs_counts(ctx, forced):
    K, Fo, po, _, B, X_ref = _system("kktz", 400, 156, 557, rows=100)
    N = K.shape[0]
    f = Prepared(ctx, Fo, po)
    for nrhs in (1, 2, 15, 16, 17, 33, 64, 100):
        X = f.solve_multi(B[:nrhs], debug=MULTI_BLOCKED if forced else 0)
        _check_rows(X[:, :N], X_ref[:nrhs], (nrhs, forced))


# ---------------------------------------------------------------------------
def _bitwise_system(N):
    return _system("indef", 300, 300, 0) if N == 300 else _system("kktz", 400, 156, 557, rows=100)


@pytest.mark.parametrize("N", [300, 556])  # the one-workgroup solve / the device-wide solve
def test_below_the_crossover_is_bk_solve_bitwise(ctx, N):
    _, Fo, po, _, B, _ = _bitwise_system(N)
    f = Prepared(ctx, Fo, po)
    single = np.stack([f.solve_single(b) for b in B[:BELOW]])
    for nrhs in (1, BELOW):
        X = f.solve_multi(B[:nrhs])
        assert np.array_equal(X[:, :N].view(np.int64), single[:nrhs].view(np.int64)), nrhs


def test_blocked_path_is_deterministic(ctx):
    _, Fo, po, _, B, _ = _bitwise_system(556)
    f = Prepared(ctx, Fo, po)
    X0 = f.solve_multi(B[:40], debug=MULTI_BLOCKED)
    X1 = f.solve_multi(B[:40], debug=MULTI_BLOCKED)
    assert np.array_equal(X0.view(np.int64), X1.view(np.int64))


def test_a_row_does_not_depend_on_its_neighbours(ctx):
    _, Fo, po, _, B, _ = _bitwise_system(556)
    f = Prepared(ctx, Fo, po)
    X17 = f.solve_multi(B[:17], debug=MULTI_BLOCKED)
    X100 = f.solve_multi(B, debug=MULTI_BLOCKED)
    assert np.array_equal(X17.view(np.int64), X100[:17].view(np.int64))


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("N", [300, 556])
def test_padding_untouched(ctx, N, forced):
    K, Fo, po, _, B, X_ref = _bitwise_system(N)
    f = Prepared(ctx, Fo, po, ld=N + 10)
    for nrhs in (BELOW, 17):
        X = f.solve_multi(B[:nrhs], ldb=N + 6, fill=FILL, debug=MULTI_BLOCKED if forced else 0)
        assert np.array_equal(X[:, N:], np.full((nrhs, 6), FILL)), (N, nrhs, forced)
        _check_rows(X[:, :N], X_ref[:nrhs], (N, nrhs, forced))


def test_singular_factor_runs_the_reference_sweeps(ctx):
    # all-zero columns: the reference divides by zero and its kp = 0 defect
    # swaps backwards.  The prepare raises the fallback flag, every blocked
    # kernel exits on it (an ungated sweep on the unbuilt L' would wreck the
    # rows first) and one launch runs the reference's sweeps on every row --
    # the kernel ipmz_bk_solve runs on each of them
    K, Fo, po, info, B, _ = _system("indef", 900, 11, 2, rows=0)
    N = 900
    assert info == 450
    ref = np.stack([oracle.bk_solve(Fo, po, b) for b in B[:20]])
    assert (~np.isfinite(ref[0])).sum() == 451
    f = Prepared(ctx, Fo, po)
    X = f.solve_multi(B[:20], debug=MULTI_BLOCKED)
    assert np.array_equal(np.isfinite(X[:, :N]), np.isfinite(ref))
    single = np.stack([f.solve_single(b) for b in B[:20]])
    assert np.array_equal(np.isfinite(single), np.isfinite(ref))
    assert np.array_equal(X[:, :N], single, equal_nan=True)
    fin = np.isfinite(ref)
    assert np.array_equal(X[:, :N][fin].view(np.int64), single[fin].view(np.int64))


def test_prepared_once_solved_often_and_bad_arguments(ctx):
    K, Fo, po, _, B, X_ref = _system("kktz", 400, 156, 557, rows=100)
    N = K.shape[0]
    f = Prepared(ctx, Fo, po)
    for nrhs in (3, 12, 40):  # looped, blocked, blocked over several row groups
        X = f.solve_multi(B[:nrhs])
        _check_rows(X[:, :N], X_ref[:nrhs], nrhs)
    args = (N, f.F.data_ptr(), f.ld, f.piv.data_ptr())
    t = torch.zeros(4, N + 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(I.IpmzError, match="workspace too small"):
        ctx.bk_prepare_solve(*args, f.ws.data_ptr(), f.wsb - 1)
    with pytest.raises(I.IpmzError, match="invalid argument"):  # odd ldb
        ctx.bk_solve_multi(*args, f.ws.data_ptr(), t.data_ptr(), N + 1, 2)
    with pytest.raises(I.IpmzError, match="16-byte aligned"):
        ctx.bk_solve_multi(*args, f.ws.data_ptr(), t.data_ptr() + 8, N + 2, 2)
    with pytest.raises(I.IpmzError, match="invalid argument"):  # negative nrhs
        ctx.bk_solve_multi(*args, f.ws.data_ptr(), t.data_ptr(), N + 2, -1)
    with pytest.raises(I.IpmzError, match="null pointer"):
        ctx.bk_solve_multi(*args, 0, t.data_ptr(), N + 2, 2)
    # no-ops: nothing is read or written
    assert ctx.bk_solve_multi(*args, f.ws.data_ptr(), t.data_ptr(), N + 2, 0) == 0
    assert ctx.bk_solve_multi(0, 0, 0, 0, 0, 0, 2, 3) == 0
    assert ctx.bk_prepare_solve(0, 0, 0, 0, 0, 0) == 0
    ctx.sync()
    assert not t.cpu().numpy().any()


def test_host_signature(ctx):
    K, Fo, po, _, B, X_ref = _system("kktz", 400, 156, 557, rows=100)
    X = B[:12].copy()
    out = I.overwriting_solve_bunch_kaufman_multi(Fo, po, X, ctx)
    assert out is X
    _check_rows(X, X_ref[:12])
    # an indefinite system solved: residual check in fp64 (test_bk_vs_oracle_bitwise)
    for x, b in zip(X, B[:12]):
        assert np.abs(K @ x - b).max() < 1e-10 * max(1.0, np.abs(K).max() * np.abs(x).max())
    assert I.LinearSolvers.overwriting_solve_bunch_kaufman_multi is I.overwriting_solve_bunch_kaufman_multi


# ---------------------------------------------------------------------------
# QP level: ipmz_qp_kkt_solve_bk (EqualityHandling::None).  (48, 16, 8): N = 72,
# the steps' one-workgroup factor, the prepared solve allocated on first use;
# (400, 60, 60): N = 520, the solver's own transposed factor, L' in K and
# device-wide solve workspace.
QPS = [(48, 16, 8), (400, 60, 60)]


@functools.lru_cache(maxsize=None)
def _qp_system(n, m, p):
    o = oracle.OracleQP(oracle.gen_qp(n, m, p, 21), eq_none=True)
    K = o.kkt()
    Fo, po, info = oracle.bk_factor(K)
    assert info == 0
    B = np.random.default_rng(5).uniform(-1, 1, (12, K.shape[0]))
    X = np.stack([oracle.bk_solve(Fo, po, b) for b in B])
    for arr in (K, B, X):
        arr.setflags(write=False)
    return K, B, X


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("n,m,p", QPS)
def test_qp_kkt_solve_bk_vs_oracle(ctx, n, m, p, forced):
    K, B, X_ref = _qp_system(n, m, p)
    g = I.Optimizer(n, m, p, ctx, equality_handling=I.EQ_NONE)
    g.generate(21)
    N = g.N
    assert N == K.shape[0] == {48: 72, 400: 520}[n]
    assert np.array_equal(g.kkt(), np.tril(K))
    t = torch.from_numpy(B.copy()).cuda()
    torch.cuda.synchronize()
    I.debug_inject(MULTI_BLOCKED if forced else 0)
    try:
        for nrhs in (BELOW, 12):  # the second call reuses the workspace of the first
            t.copy_(torch.from_numpy(B.copy()))
            torch.cuda.synchronize()
            assert g.kkt_solve_bk(t.data_ptr(), nrhs, N) == 0
            _check_rows(t.cpu().numpy()[:nrhs], X_ref[:nrhs], (n, forced, nrhs))
    finally:
        I.debug_inject(0)


@pytest.mark.parametrize("n,m,p", QPS)
def test_qp_kkt_solve_bk_leaves_the_steps_unchanged(ctx, n, m, p):
    a = I.Optimizer(n, m, p, ctx, equality_handling=I.EQ_NONE)
    b = I.Optimizer(n, m, p, ctx, equality_handling=I.EQ_NONE)
    a.generate(22)
    b.generate(22)
    t = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (12, a.N))).cuda()
    torch.cuda.synchronize()
    for it in range(3):
        a.kkt_solve_bk(t.data_ptr(), 12, a.N)
        a.step()
        b.step()
        assert np.array_equal(a.vars().view(np.int64), b.vars().view(np.int64)), it
        sa, sb = a.scalars(), b.scalars()
        assert list(sa) == list(sb)
        assert np.array_equal(np.array(list(sa.values())).view(np.int64),
                              np.array(list(sb.values())).view(np.int64)), it


def test_qp_kkt_solve_bk_unsupported(ctx):
    QP = dict(n=48, m=16, p=8)
    t = torch.zeros(2, 80, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    batch = I.Batch(batch=2, ctx=ctx, equality_handling=I.EQ_NONE, **QP)
    batch.generate(1)
    with pytest.raises(I.IpmzError, match="batch"):
        batch.kkt_solve_bk(t.data_ptr(), 2, 80)
    reg = I.Optimizer(ctx=ctx, equality_handling=I.EQ_REGULARIZATION, **QP)
    reg.generate(1)
    with pytest.raises(I.IpmzError, match="EqualityHandling::None only"):
        reg.kkt_solve_bk(t.data_ptr(), 2, 80)
    unloaded = I.Optimizer(ctx=ctx, equality_handling=I.EQ_NONE, **QP)
    with pytest.raises(I.IpmzError, match="bad state"):
        unloaded.kkt_solve_bk(t.data_ptr(), 2, 80)
