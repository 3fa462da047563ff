"""The LDL^T factors at zero, filled-in and non-finite pivots (include/ipmz.h,
"Conventions"): the zero-pivot rule of LinearSolvers.cpp:26-28 at every edge
of the blocking, the return value (first non-finite pivot, reset by the next
factor), a zero input diagonal that fills in, and "only the lower triangle of
K is read" -- for ipmz_ldlt_factor, ipmz_mixed_factor and ipmz_normal_factor.

The random quasi-definite matrices and generated QPs of the other files never
produce a zero or non-finite pivot; the matrices here (pivot_cases.py) do, at
pivot 0, the 16-tile edge (15/16), the inner-block edges (63/64, 127/128), the
outer-panel edge (nbo-1/nbo), inside the last ragged block and at N-1.
References: oracle.ldlt / oracle.solve_ldlt (the restatement of the
reference), and for the integer matrices of case 1 the closed-form factor,
compared without tolerance.  tests/test_oracle_pivot_cases.py checks the
generators' own conditions on the CPU.

Every tolerance is derived (the equalities) or an existing bound of this
project: the ragged test's 1e-12 max|D| / 1e-11 max(1, max|L|) / 1e-10 on x
(test_gpu_parity.py), the blocked path's rtol 1e-13, and test_gpu_mixed.py's
acceptance of a refined solve.  Each test prints its worst figure per
assertion before asserting it.

Follow-up, not covered here: the batched small-system kernels (small.hip: ONE,
PAIR, LEFT) and ldlt_diag64_blk_kernel take the colpass16_spec pass and are
reachable only through a Batch's Newton step, which factors the KKT matrix it
assembled from QP data (generated, or handed over with Batch.load_one) --
never with a zero pivot; testing them needs a way to hand the batched factor
a KKT matrix itself.  (The batched kernel chain and solves at ordinary pivots:
test_gpu_batch_large.py.)
"""
import contextlib

import numpy as np
import pytest

import oracle
import pivot_cases as pc

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

ALL_CONFIGS = pc.ORACLE_CONFIGS + pc.EXACT_ONLY_CONFIGS
_ids = lambda c: f"N{c[0]}-nbo{c[1][0]}-nbi{c[1][1]}"  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    c = I.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        yield c
    finally:
        c.set_blocking(0, 64)
        c.set_stream(None)


@contextlib.contextmanager
def _blocking(ctx, N, blocking):
    ctx.set_blocking(*blocking)
    try:
        nbo, nbi = ctx.blocking(N)
        assert (nbo, nbi) == pc.resolve_blocking(N, blocking)  # the position lists assume it
        yield nbo, nbi
    finally:
        ctx.set_blocking(0, 64)


def _chk(label, err, bound):
    print(f"{label}: {err:.3e} (bound {bound:.3e})", flush=True)
    assert err < bound, (label, err, bound)


# ---------------------------------------------------------------------------
# device plumbing
def _dev(K, ld=None, fill=0.0):
    """Lower triangle of K in an (N, ld) device array; the strict upper
    triangle and the pad columns hold `fill`."""
    N = K.shape[0]
    buf = np.full((N, ld or N), fill)
    il = np.tril_indices(N)
    buf[il] = K[il]
    return torch.from_numpy(buf).cuda()


class _Ldlt:
    """ipmz_ldlt_factor of K on one workspace (kept for further factors)."""

    def __init__(self, ctx, N):
        self.ctx, self.N = ctx, N
        self.wsb = ctx.workspace_bytes(N)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device="cuda")
        self.D = torch.zeros(N, dtype=torch.float64, device="cuda")

    def factor(self, K, ld=None, fill=0.0):
        self.K = _dev(K, ld, fill)
        self.ld = self.K.shape[1]
        self.D.zero_()
        info = self.ctx.ldlt_factor(self.N, self.K.data_ptr(), self.ld, self.D.data_ptr(), self.ws.data_ptr(), self.wsb)
        full = self.K.cpu().numpy()
        return info, np.tril(full[:, :self.N], -1), self.D.cpu().numpy(), full

    def solve(self, b):
        x = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).cuda()
        a = (self.N, self.K.data_ptr(), self.ld, self.D.data_ptr(), self.ws.data_ptr(), x.data_ptr())
        if x.ndim == 1:
            self.ctx.ldlt_solve(*a)
        else:
            self.ctx.ldlt_solve_multi(*a, x.shape[1], x.shape[0])
        self.ctx.sync()
        return x.cpu().numpy()


class _Mixed:
    """ipmz_mixed_factor / ipmz_mixed_solve; the fp32 factor is read back from
    the workspace (K32 first, then D32: mixed_ws_carve, as test_gpu_panel_forms.py)."""

    def __init__(self, ctx, N):
        self.ctx, self.N = ctx, N
        self.wsb = ctx.mixed_workspace_bytes(N)
        self.ws = torch.zeros(self.wsb // 4 + 64, dtype=torch.float32, device="cuda")
        self.ld32 = (N + 63) // 64 * 64
        self.doff = ((N * self.ld32 * 4 + 255) // 256 * 256) // 4

    def factor(self, K, ld=None, fill=0.0):
        self.K = _dev(K, ld, fill)
        self.ld = self.K.shape[1]
        self.K0 = self.K.cpu().numpy().copy()
        return self.ctx.mixed_factor(self.N, self.K.data_ptr(), self.ld, self.ws.data_ptr(), self.wsb)

    def factor32(self):
        torch.cuda.synchronize()
        N = self.N
        L = torch.tril(self.ws[:N * self.ld32].view(N, self.ld32)[:, :N], -1)
        return L.cpu().numpy(), self.ws[self.doff:self.doff + N].cpu().numpy()

    def solve(self, b, tol=1e-12, max_refine=10):
        x = torch.from_numpy(b.copy()).cuda()
        ratio, iters = self.ctx.mixed_solve(self.N, self.K.data_ptr(), self.ld, self.ws.data_ptr(), x.data_ptr(), tol,
                                            max_refine)
        torch.cuda.synchronize()
        # K itself is left intact, bit for bit (NaN fills included)
        assert np.array_equal(self.K.cpu().numpy().view(np.int64), self.K0.view(np.int64))
        return x.cpu().numpy(), ratio, iters


def _accept_mixed(label, K, K_ref, b, x, ratio, iters, tol=1e-12):
    """test_gpu_mixed.py's acceptance: the residual met tol (recomputed here in
    fp64) and the error follows it, against numpy's solve of K_ref."""
    r = np.abs(b - K @ x).max() / np.abs(b).max()
    print(f"{label}: mixed ratio {ratio:.2e}, recomputed {r:.2e}, {iters} corrections", flush=True)
    assert ratio <= tol and r <= tol, (label, ratio, r, iters)
    assert iters <= 10, (label, iters)
    x_ref = np.linalg.solve(K_ref, b)
    cond = np.linalg.cond(K_ref, np.inf)
    _chk(f"{label}: mixed |x - x_ref|/|x_ref| (cond_inf {cond:.1f})", np.abs(x - x_ref).max() / np.abs(x_ref).max(),
         2 * cond * tol + 1e-13)


def _ragged_bounds(label, L, D, L_o, D_o, keep=None):
    """The bounds of test_ldlt_ragged_vs_oracle, over the entries `keep`
    (index array; default all): D to 1e-12 max|D|, L to 1e-11 max(1, max|L|)."""
    if keep is not None:
        L, L_o, D, D_o = L[np.ix_(keep, keep)], L_o[np.ix_(keep, keep)], D[keep], D_o[keep]
    L_o = np.tril(L_o, -1)
    if D.size == 0:
        return
    _chk(f"{label}: |D - D_o|", np.abs(D - D_o).max(), 1e-12 * np.abs(D_o).max())
    _chk(f"{label}: |L - L_o|", np.abs(L - L_o).max(), 1e-11 * max(1.0, np.abs(L_o).max()))


_oracle_cache = {}


def _oracle_ldlt(key, K):
    """oracle.ldlt computed once per matrix and shared, never modified."""
    if key not in _oracle_cache:
        L, D = oracle.ldlt(K)
        L.setflags(write=False)
        D.setflags(write=False)
        _oracle_cache[key] = (L, D)
    return _oracle_cache[key]


# ---------------------------------------------------------------------------
# 1. exact integer factor with pivots that cancel to zero
@pytest.mark.parametrize("cfg", ALL_CONFIGS, ids=_ids)
def test_exact_integer_factor(ctx, cfg):
    """K = (L0 D0) L0^T of small integers with D0 = 0 at every edge position:
    each zero pivot appears only after the updates from its left neighbours
    cancelled it, and every intermediate of any blocked elimination order is an
    integer far below 2^53 divided by +-1 or +-2 only (condition asserted
    first), so the factor is exact: D == D0 with 1e-8 at the zeros, L == L0 with
    those columns zero -- np.array_equal, no tolerance.  A dropped, doubled or
    mis-addressed update tile anywhere breaks it.  The solves (single and 17
    rows) meet the blocked solve's 1e-10 max(1, |x_ref|_inf) against the
    oracle's solve with the expected factor.

    Observed on an MI355X: the factor is exact in all seven configurations
    (D0 keeps +-2: the reciprocal of +-2 after the Newton step is exact).
    A B 128 = 3.7e8 / 1.5e8 / 1.0e9 / 9.6e8 / 7.1e8 for N = 200 / 300 / 700 /
    2560 / 4100.  Worst solve error relative to max(1, |x_ref|_inf): single
    2.8e-14, 17 rows 1.0e-13 (both at N = 4100, where |x_ref|_inf ~ 1e211: L0's
    inverse grows with N); at N <= 700 at most 5.8e-15."""
    N, blocking = cfg
    with _blocking(ctx, N, blocking) as (nbo, nbi):
        pos = pc.positions(N, nbo, nbi)
        K, L0, D0, L_exp, D_exp = pc.int_factor(N, 11 * N, pos)
        A, B, prod = pc.exactness_product(L0, D0)
        print(f"exactness: A = {A:.3g}, B = {B:.3g}, A B 128 = {prod:.3g}", flush=True)
        assert prod < 2.0 ** 53
        f = _Ldlt(ctx, N)
        info, L, D, _ = f.factor(K)
        assert info == 0
        bad = np.flatnonzero(D != D_exp)
        assert bad.size == 0, ("pivots differ, first at", bad[:8], D[bad[:8]], D_exp[bad[:8]])
        badL = np.argwhere(L != L_exp)
        assert badL.size == 0, ("L differs, first at", badL[:8])
        assert np.array_equal(D[pos], np.full(len(pos), 1e-8))
        rng = np.random.default_rng(N)
        b = rng.integers(-3, 4, (17, N)).astype(np.float64)
        b[:, pos] = 0.0
        Lf = L_exp + np.eye(N)
        x_ref = np.stack([oracle.solve_ldlt(Lf, D_exp, b[r]) for r in range(17)])
        x1 = f.solve(b[0])
        rel = np.abs(x1 - x_ref[0]).max() / max(1.0, np.abs(x_ref[0]).max())
        _chk("solve: |x - x_ref| / max(1, |x_ref|)", rel, 1e-10)
        xm = f.solve(b)
        rel = max(np.abs(xm[r] - x_ref[r]).max() / max(1.0, np.abs(x_ref[r]).max()) for r in range(17))
        _chk("solve_multi (17 rows): worst |x - x_ref| / max(1, |x_ref|)", rel, 1e-10)


# ---------------------------------------------------------------------------
# 2. decoupled zero rows and columns, generic values
@pytest.mark.parametrize("cfg", pc.ORACLE_CONFIGS, ids=_ids)
def test_zero_rows_fp64_and_fp32(ctx, cfg):
    """_qd with the row and column of every edge position zeroed: D[j] == 1e-8
    and L[j+1:, j] == 0 == L[j, :j] exactly; the other entries are the factor of
    the matrix without those rows (ragged bounds over them).  b[j] = 1 gives
    x[j] = 1e8 (rtol 1e-13), the rest to 1e-10.  N = 300 / 700: the fp32 factor
    of ipmz_mixed_factor (k_mx_scale's s = 1 branch) has D32[j] == fp32(1e-8)
    and zero columns too, and its refined solve with b[j] = 0 is accepted as
    test_gpu_mixed.py accepts one.

    Observed on an MI355X, worst over the five configurations: |D - D_o|
    7.1e-15 (bound 2.5e-12), |L - L_o| 1.1e-16 (1e-11), x[j] == 1e8 exactly,
    |x - x_o| elsewhere 2.9e-15 (1e-10); mixed: ratio 6.0e-13 after 1
    correction, error 2.6e-13 (bound 1.5e-10 at cond_inf 74)."""
    N, blocking = cfg
    with _blocking(ctx, N, blocking) as (nbo, nbi):
        pos = pc.positions(N, nbo, nbi)
        keep = np.setdiff1d(np.arange(N), pos)
        K = pc.zero_rows(pc.qd(N, N), pos)
        L_o, D_o = _oracle_ldlt(("zero", N, tuple(pos)), K)
        f = _Ldlt(ctx, N)
        info, L, D, _ = f.factor(K)
        assert info == 0
        assert np.array_equal(D[pos], np.full(len(pos), 1e-8)), D[pos]
        for j in pos:
            assert not L[j + 1:, j].any() and not L[j, :j].any(), j
        _ragged_bounds("zero rows", L, D, L_o, D_o, keep)
        b = np.random.default_rng(1).uniform(-1, 1, N)
        b[pos] = 1.0
        x_o = oracle.solve_ldlt(L_o, D_o, b)
        x = f.solve(b)
        _chk("zero rows: x[j] / 1e8 - 1", np.abs(x[pos] / x_o[pos] - 1).max(), 1e-13)
        _chk("zero rows: |x - x_o| elsewhere", np.abs(x[keep] - x_o[keep]).max(), 1e-10)
        if N in (300, 700):
            m = _Mixed(ctx, N)
            assert m.factor(K) == 0
            L32, D32 = m.factor32()
            assert np.array_equal(D32[pos], np.full(len(pos), np.float32(1e-8))), D32[pos]
            for j in pos:
                assert not L32[j + 1:, j].any() and not L32[j, :j].any(), j
            assert np.isfinite(L32).all() and np.isfinite(D32).all()
            b[pos] = 0.0
            xm, ratio, iters = m.solve(b)
            K1 = K.copy()
            K1[pos, pos] = 1.0
            _accept_mixed("zero rows", K, K1, b, xm, ratio, iters)


# ---------------------------------------------------------------------------
# 3. a 1e8 multiplier crossing a boundary
@pytest.mark.parametrize("cfg", pc.ORACLE_CONFIGS, ids=_ids)
def test_large_multiplier_across_edges(ctx, cfg):
    """[[0, 1], [1, 2]] embedded at (j, j+1) across the 16-tile, inner-block and
    outer-panel edges and at the end: D[j] == 1e-8 exactly, L[j+1, j] = 1e8 and
    D[j+1] = 2 - 1e8 to rtol 1e-13, everything else to the ragged bounds
    evaluated over the ordinary entries only (with max|L| = 1e8 the bound would
    be an absolute 1e-3).  Solve with b[j] = 0, b[j+1] = 1 (the well-conditioned
    right-hand side): the special entries to rtol 1e-13, the others to 1e-10.

    Observed on an MI355X, worst over the five configurations: L[j+1, j],
    D[j+1], x[j] and x[j+1] equal the oracle's bit for bit; ordinary entries
    |D - D_o| 7.1e-15 (bound 2.5e-12), |L - L_o| 1.4e-16 (1e-11), |x - x_o|
    3.3e-15 (1e-10)."""
    N, blocking = cfg
    with _blocking(ctx, N, blocking) as (nbo, nbi):
        pairs = pc.pair_positions(N, nbo)
        js = np.array(pairs)
        sp = np.sort(np.concatenate([js, js + 1]))
        keep = np.setdiff1d(np.arange(N), sp)
        K = pc.embed_pairs(pc.qd(N, N), pairs)
        L_o, D_o = _oracle_ldlt(("pairs", N, tuple(pairs)), K)
        assert np.array_equal(D_o[js], np.full(len(js), 1e-8))
        assert np.array_equal(L_o[js + 1, js], np.full(len(js), 1e8))
        f = _Ldlt(ctx, N)
        info, L, D, _ = f.factor(K)
        assert info == 0
        assert np.array_equal(D[js], np.full(len(js), 1e-8)), D[js]
        _chk("pairs: L[j+1, j] / 1e8 - 1", np.abs(L[js + 1, js] / L_o[js + 1, js] - 1).max(), 1e-13)
        _chk("pairs: D[j+1] / (2 - 1e8) - 1", np.abs(D[js + 1] / D_o[js + 1] - 1).max(), 1e-13)
        # the pairs are decoupled: nothing else in their rows and columns
        Lz = L.copy()
        Lz[js + 1, js] = 0.0
        assert not Lz[sp, :].any() and not Lz[:, sp].any()
        _ragged_bounds("pairs", L, D, L_o, D_o, keep)
        b = np.random.default_rng(2).uniform(-1, 1, N)
        b[js], b[js + 1] = 0.0, 1.0
        x_o = oracle.solve_ldlt(L_o, D_o, b)
        x = f.solve(b)
        _chk("pairs: x[j], x[j+1] relative", np.abs(x[sp] / x_o[sp] - 1).max(), 1e-13)
        _chk("pairs: |x - x_o| elsewhere", np.abs(x[keep] - x_o[keep]).max(), 1e-10)


# ---------------------------------------------------------------------------
# 4. zero input diagonal that fills in
@pytest.mark.parametrize("n,mp,blocking", [(150, 50, (0, 64)), (450, 250, (0, 64)), (450, 250, (256, 128))])
def test_zero_diagonal_fills_in(ctx, n, mp, blocking):
    """K = [[H, B^T], [B, 0]]: the input diagonal of the second block is exactly
    zero, its pivots -(B H^-1 B^T) are not -- the zero test belongs to the
    updated entry.  fp64: info 0, D[n:] < 0, no 1e-8, ragged bounds, x to 1e-10.
    Mixed: k_mx_scale's s = 1 branch on mp rows; accepted as test_gpu_mixed.py
    does, with at most 10 corrections.

    Observed on an MI355X: |D - D_o| 4.2e-15 (bound 2.0e-12), |L - L_o| 1.1e-15
    (1e-11), |x - x_o| 1.0e-13 (1e-10); mixed: 1 correction (N = 200, ratio
    4.6e-13, error 2.7e-13) and 2 corrections (N = 700, ratio 4.9e-15, error
    1.9e-15, cond_inf 3050)."""
    N = n + mp
    with _blocking(ctx, N, blocking):
        K = pc.saddle(n, mp, N)
        L_o, D_o = _oracle_ldlt(("saddle", n, mp), K)
        f = _Ldlt(ctx, N)
        info, L, D, _ = f.factor(K)
        assert info == 0
        assert (D[:n] > 0).all() and (D[n:] < 0).all() and not (D == 1e-8).any()
        _ragged_bounds("saddle", L, D, L_o, D_o)
        b = np.random.default_rng(3).uniform(-1, 1, N)
        x = f.solve(b)
        _chk("saddle: |x - x_o|", np.abs(x - oracle.solve_ldlt(L_o, D_o, b)).max(), 1e-10)
        m = _Mixed(ctx, N)
        assert m.factor(K) == 0
        xm, ratio, iters = m.solve(b)
        _accept_mixed("saddle", K, K, b, xm, ratio, iters)


# ---------------------------------------------------------------------------
# 5. non-finite pivots and the info word
@pytest.mark.parametrize("cfg", pc.ORACLE_CONFIGS, ids=_ids)
def test_first_nonfinite_pivot_ldlt(ctx, cfg):
    """One Inf on the diagonal or one NaN off it per factor: the return value
    is row + 1 (earlier: a 0 * NaN leak through tile padding; later or 0: a
    missed check), the call returns, D[row] is non-finite, and rows [:row] are
    the clean factor's (a NaN enters the Schur complement through row and
    column `row` only).  A clean factor on the same workspace then returns 0
    and matches the oracle: the info word is reset.

    Observed on an MI355X: every return value is row + 1; rows before the
    pivot and the clean factor afterwards: |D - D_o| 7.1e-15 (bound 2.5e-12),
    |L - L_o| 1.2e-16 (1e-11)."""
    N, blocking = cfg
    with _blocking(ctx, N, blocking) as (nbo, nbi):
        K = pc.qd(N, N)
        L_o, D_o = _oracle_ldlt(("qd", N), K)
        dtol, ltol = 1e-12 * np.abs(D_o).max(), 1e-11 * max(1.0, np.abs(np.tril(L_o, -1)).max())
        f = _Ldlt(ctx, N)
        worst = [0.0, 0.0, 0.0, 0.0]
        for label, i, j, val in pc.contaminations(N, nbo):
            info, L, D, _ = f.factor(pc.contaminate(K, i, j, val))
            assert info == i + 1, (label, info)
            assert not np.isfinite(D[i]), (label, D[i])
            if i:
                worst[0] = max(worst[0], np.abs(D[:i] - D_o[:i]).max())
                worst[1] = max(worst[1], np.abs(L[:i, :i] - np.tril(L_o, -1)[:i, :i]).max())
                assert np.abs(D[:i] - D_o[:i]).max() < dtol, label
                assert np.abs(L[:i] - np.tril(L_o, -1)[:i]).max() < ltol, label
            info, L, D, _ = f.factor(K)
            assert info == 0, (label, info)
            worst[2] = max(worst[2], np.abs(D - D_o).max())
            worst[3] = max(worst[3], np.abs(L - np.tril(L_o, -1)).max())
            assert np.abs(D - D_o).max() < dtol and np.abs(L - np.tril(L_o, -1)).max() < ltol, label
        print(f"rows before the pivot: |D - D_o| {worst[0]:.3e} (bound {dtol:.3e}), |L - L_o| {worst[1]:.3e} "
              f"(bound {ltol:.3e}); clean factor after: {worst[2]:.3e}, {worst[3]:.3e}", flush=True)


def test_first_nonfinite_pivot_mixed(ctx):
    """The same contaminations through ipmz_mixed_factor (N = 300, three
    panels): return value row + 1; the clean factor afterwards returns 0."""
    N, blocking = 300, (128, 64)
    with _blocking(ctx, N, blocking) as (nbo, nbi):
        K = pc.qd(N, N)
        m = _Mixed(ctx, N)
        for label, i, j, val in pc.contaminations(N, nbo):
            assert m.factor(pc.contaminate(K, i, j, val)) == i + 1, label
            assert m.factor(K) == 0, label
        b = np.random.default_rng(4).uniform(-1, 1, N)
        x, ratio, iters = m.solve(b)
        _accept_mixed("after contaminated factors", K, K, b, x, ratio, iters)


class _Normal:
    def __init__(self, ctx, n, mp):
        self.ctx, self.n, self.mp, self.N = ctx, n, mp, n + mp
        self.wsb = ctx.normal_workspace_bytes(n, mp)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device="cuda")
        self.D = torch.zeros(self.N, dtype=torch.float64, device="cuda")

    def factor(self, K, ld=None, fill=0.0):
        self.K = _dev(K, ld, fill)
        self.ld = self.K.shape[1]
        self.D.zero_()
        info = self.ctx.normal_factor(self.n, self.mp, self.K.data_ptr(), self.ld, self.D.data_ptr(),
                                      self.ws.data_ptr(), self.wsb)
        torch.cuda.synchronize()
        full = self.K.cpu().numpy()
        return info, np.tril(full[:, :self.N], -1), self.D.cpu().numpy(), full

    def solve(self, b):
        x = torch.from_numpy(b.copy()).cuda()
        self.ctx.normal_solve(self.n, self.mp, self.K.data_ptr(), self.ld, self.D.data_ptr(), self.ws.data_ptr(),
                              x.data_ptr())
        torch.cuda.synchronize()
        return x.cpu().numpy()


def test_first_nonfinite_pivot_normal(ctx):
    """ipmz_normal_factor: a non-finite entry inside H returns row + 1, and
    "S not positive definite" -- K[n+q, n+q] = +10, i.e. E_q = -10 -- returns
    n + q + 1 (the oracle's pivots are < 0 before n + q and > 0 there: asserted
    first).  A clean factor on the same workspace returns 0 again."""
    n, mp = 150, 50
    N = n + mp
    with _blocking(ctx, N, (0, 64)) as (nbo, nbi):
        K = pc.aug(n, mp, N)
        f = _Normal(ctx, n, mp)
        for label, i, j, val in pc.contaminations(N, nbo, limit=n):
            assert f.factor(pc.contaminate(K, i, j, val))[0] == i + 1, label
            assert f.factor(K)[0] == 0, label
        for q in (0, mp - 1):
            Kq = pc.contaminate(K, n + q, n + q, 10.0)
            D_o = oracle.ldlt(Kq)[1]
            assert (D_o[:n] > 0).all() and (D_o[n:n + q] < 0).all() and D_o[n + q] > 0
            assert f.factor(Kq)[0] == n + q + 1, q
            info, L, D, _ = f.factor(K)
            assert info == 0 and (D[:n] > 0).all() and (D[n:] < 0).all(), q


# ---------------------------------------------------------------------------
# 6. the upper triangle and the pad columns are never read
def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _pads_hold(full, N, fill):
    pad, up = full[:, N:], full[np.triu_indices(N, 1)]
    return (np.isnan(pad).all() if np.isnan(fill) else (pad == fill).all()), up


@pytest.mark.parametrize("ld", [302, 384])
@pytest.mark.parametrize("which", ["ldlt", "normal", "mixed"])
def test_upper_triangle_and_pads_never_read(ctx, which, ld):
    """N = 300, three panels, ld = N + 2 and 384: a run with the strict upper
    triangle and the pad columns [N, ld) zero-filled and one with them
    NaN-filled give bitwise the same strict lower triangle, D and x; the pad
    columns keep their fill; ipmz_mixed_factor / _solve leave K untouched
    entirely.  (Whether the upper triangle is written is not asserted: the
    header does not promise it.)  The ld = N + 2 result meets the ragged bounds
    against the oracle.

    Observed on an MI355X: bitwise equal in all six combinations; ld = 302:
    |D - D_o| 4.4e-15 (bound 2.5e-12), |L - L_o| 1.9e-16 (1e-11), |x - x_ref|
    1.7e-15; mixed ratio 2.6e-13 after 1 correction, error 1.1e-13."""
    N, n, mp = 300, 225, 75
    with _blocking(ctx, N, (128, 64)):
        K = pc.aug(n, mp, N) if which == "normal" else pc.qd(N, N)
        b = np.random.default_rng(6).uniform(-1, 1, N)
        out = []
        for fill in (0.0, np.nan):
            if which == "mixed":
                f = _Mixed(ctx, N)
                assert f.factor(K, ld, fill) == 0
                L, D = f.factor32()
                x, ratio, iters = f.solve(b)
                assert ratio <= 1e-12, (ratio, iters)
            else:
                f = _Ldlt(ctx, N) if which == "ldlt" else _Normal(ctx, n, mp)
                info, L, D, full = f.factor(K, ld, fill)
                assert info == 0
                assert _pads_hold(full, N, fill)[0]
                x = f.solve(b)
            out.append((L, D, x))
        assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all() and np.isfinite(out[0][2]).all()
        for w, name in enumerate(("L", "D", "x")):
            assert np.array_equal(_bits(out[1][w]), _bits(out[0][w])), f"{name} depends on the upper triangle / pads"
        if ld == N + 2:
            L, D, x = out[0]
            if which == "mixed":
                _accept_mixed(f"{which} ld {ld}", K, K, b, x, ratio, iters)
            else:
                L_o, D_o = _oracle_ldlt((which, N), K)
                _ragged_bounds(f"{which} ld {ld}", L, D, L_o, D_o)
                if which == "ldlt":
                    _chk("ldlt: |x - x_o|", np.abs(x - oracle.solve_ldlt(L_o, D_o, b)).max(), 1e-10)
                else:  # test_gpu_normal.py's bound against numpy's solve
                    x_ref = np.linalg.solve(K, b)
                    _chk("normal: |x - x_ref|", np.abs(x - x_ref).max(), 1e-12 * max(1.0, np.abs(x_ref).max()))
