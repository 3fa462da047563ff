"""The Bunch-Kaufman factor's pivot CHOICES on the device (bk.hip): tied
column maxima, the three threshold tests at equality and one ulp off,
non-finite entries, overflowing scales -- the cases of tests/bk_pivot_cases.py,
whose claims tests/test_oracle_bk_pivot_cases.py checks without a GPU.  Run on
an MI355X: pytest -m gpu.

Contract: ipiv and F equal the oracle's bit for bit (NaN == NaN in the
non-finite families); info is 1 + the first all-zero column.  Both kernels
(one workgroup, whole device) take every case at every N and agree with each
other; the batched factor agrees with the single one.  The solves and the
Newton steps keep the bounds their own test files use.
"""
import numpy as np
import pytest

import bk_batch_cases
import bk_pivot_cases as C
import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")
DX_TOL = 1e-10  # tests/test_gpu_eqnone.py


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


_device = {}


def _dev_factor(ctx, K, algo):
    N = K.shape[0]
    A = torch.from_numpy(np.array(K, order="C")).cuda()
    piv = torch.full((N,), -12345, dtype=torch.int32, device="cuda")
    info = ctx.bk_factor(N, A.data_ptr(), N, piv.data_ptr(), algo=algo)
    ctx.sync()
    return A.cpu().numpy(), piv.cpu().numpy(), info


def _factored(ctx, name, algo):
    """The device factor of a case, made once per kernel."""
    if (name, algo) not in _device:
        _device[name, algo] = _dev_factor(ctx, C.cases()[name][1], algo)
    return _device[name, algo]


def _device_info(trace):
    zero = [r["k"] for r in trace if r["branch"] == "zero"]
    return zero[0] + 1 if zero else 0


def _assert_factor(got, want, nonfinite, label):
    (F, piv, info), (Fo, po, info_o) = got, want
    assert np.array_equal(piv, po), (label, np.flatnonzero(piv != po)[:8], piv[piv != po][:8], po[piv != po][:8])
    assert np.array_equal(np.isnan(F), np.isnan(Fo)), label
    bad = ~((F == Fo) | (np.isnan(F) & np.isnan(Fo)))
    assert not bad.any(), (label, np.argwhere(bad)[:8])
    if not nonfinite:
        assert np.isfinite(F).all(), label
    assert info == info_o, (label, info, info_o)


@pytest.mark.parametrize("name", C.names())
def test_factor_both_kernels(ctx, name):
    family, K, nonfinite = C.cases()[name]
    Fo, po, io = C.oracle_factor(name)
    want_info = _device_info(C.traced(name)[3])
    assert want_info == (io + 1 if io else want_info)  # the oracle's 0-based word + 1 (it stays 0 for column 0)
    wg = _factored(ctx, name, ctx.BK_WORKGROUP)
    _assert_factor(wg, (Fo, po, want_info), nonfinite, (name, "workgroup"))
    gr = _factored(ctx, name, ctx.BK_GRID)
    _assert_factor(gr, (Fo, po, want_info), nonfinite, (name, "grid"))
    _assert_factor(gr, wg, nonfinite, (name, "grid vs workgroup"))
    if not any(r["kp_lt_k"] for r in C.traced(name)[3]):  # (a backward interchange reaches above the diagonal)
        assert np.array_equal(np.triu(wg[0], 1), np.triu(K, 1), equal_nan=nonfinite)
        assert np.array_equal(np.triu(gr[0], 1), np.triu(K, 1), equal_nan=nonfinite)


@pytest.mark.parametrize("k", sorted(C.SPREAD_COLUMNS))
def test_spread_tie_one_ulp_hands_the_tie_on(ctx, k):
    # the first tied entry one ulp lower: the second tied row wins, a 1x1 interchange instead of the 2x2 pivot
    K = C.spread_tie(ulp_column=k)
    Fo, po, io = oracle.bk_factor(K)
    po = po.astype(np.int32)
    rows = C.SPREAD_COLUMNS[k]
    assert po[k] == rows[1] and C.oracle_factor("spread_tie")[1][k] == -rows[0]
    for algo in (ctx.BK_WORKGROUP, ctx.BK_GRID):
        _assert_factor(_dev_factor(ctx, K, algo), (Fo, po, 0), False, (k, algo))


def _by_order():
    groups = {}
    for name in C.names():
        groups.setdefault(C.cases()[name][1].shape[0], []).append(name)
    return {N: g for N, g in groups.items() if len(g) > 1}


@pytest.mark.parametrize("N", sorted(_by_order()))
def test_factor_batch(ctx, N):
    # different cases of one order in one launch, strided storage, NaN in every gap
    group = _by_order()[N]
    B, ld, sP = len(group), N + 3, N + 5
    sA = ld * N + 6 + ((ld * N) & 1)
    host = np.full(B * sA, np.nan)
    mask = np.ones(B * sA, dtype=bool)  # the padding
    for q, name in enumerate(group):
        host[q * sA:q * sA + N * ld].reshape(N, ld)[:, :N] = C.cases()[name][1]
        mask[q * sA:q * sA + N * ld].reshape(N, ld)[:, :N] = False
    hp = np.full(B * sP, -777, dtype=np.int32)
    A, piv = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(hp.copy()).cuda()
    torch.cuda.synchronize()
    rc, info = ctx.bk_factor_batch(N, B, A.data_ptr(), ld, sA, piv.data_ptr(), sP)
    ctx.sync()
    got, gp = A.cpu().numpy(), piv.cpu().numpy()
    assert np.isnan(got[mask]).all() and mask.sum() >= B * (3 * N + 6)
    assert np.array_equal(got[mask].view(np.int64), host[mask].view(np.int64))  # the padding keeps its bits
    want = []
    for q, name in enumerate(group):
        nonfinite = C.cases()[name][2]
        Fq = got[q * sA:q * sA + N * ld].reshape(N, ld)[:, :N]
        pq = gp[q * sP:q * sP + N]
        assert (gp[q * sP + N:(q + 1) * sP] == -777).all()
        single = _factored(ctx, name, ctx.BK_WORKGROUP)
        _assert_factor((Fq, pq, info[q]), single, nonfinite, (name, "batch vs single"))
        Fo, po, _ = C.oracle_factor(name)
        _assert_factor((Fq, pq, info[q]), (Fo, po, _device_info(C.traced(name)[3])), nonfinite, (name, "batch"))
        want.append(single[2])
    assert rc == (min(w for w in want if w) if any(want) else 0)


def _solvable(name):
    """info == 0 on the device (no all-zero column, column 0 included) and a finite factor."""
    K = C.cases()[name][1]
    Fo, _, io = C.oracle_factor(name)
    return io == 0 and K[:, 0].any() and bool(np.isfinite(Fo).all())


SOLVABLE = [n for n in C.names() if _solvable(n)]


def _rhs(N, rows):
    return np.random.default_rng(8000 + N).uniform(-1.0, 1.0, (rows, N))


def _assert_solution(x, ref, tol, label):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(x), fin), label
    if fin.any():
        err = np.abs(x[fin] - ref[fin]).max() / max(1.0, np.abs(ref[fin]).max())
        print(f"{label}: err {err:.3e}")
        assert err <= tol, (label, err)


@pytest.mark.parametrize("name", SOLVABLE)
def test_solves(ctx, name):
    K = C.cases()[name][1]
    Fo, po, io = C.oracle_factor(name)
    assert io == 0 and _device_info(C.traced(name)[3]) == 0 and np.isfinite(Fo).all()
    N = K.shape[0]
    B = _rhs(N, 5)
    with np.errstate(all="ignore"):
        ref = np.stack([oracle.bk_solve(Fo, po, b) for b in B])
    x = B[0].copy()
    I.LinearSolvers.overwriting_solve_bunch_kaufman(np.array(Fo), np.array(po), x, ctx)
    _assert_solution(x, ref[0], 1e-12, (name, "solve"))  # the bound of test_bk_fast_solve_kkt_vs_oracle
    # the prepared multi-right-hand-side solve, 5 rows
    ldb = N + (N & 1)
    F_d = torch.from_numpy(np.array(Fo)).cuda()
    p_d = torch.from_numpy(np.array(po)).cuda()
    wsb = ctx.bk_solve_workspace_bytes(N)
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda")
    Bp = np.zeros((5, ldb))
    Bp[:, :N] = B
    t = torch.from_numpy(Bp).cuda()
    torch.cuda.synchronize()
    ctx.bk_prepare_solve(N, F_d.data_ptr(), N, p_d.data_ptr(), ws.data_ptr(), wsb)
    ctx.bk_solve_multi(N, F_d.data_ptr(), N, p_d.data_ptr(), ws.data_ptr(), t.data_ptr(), ldb, 5)
    ctx.sync()
    X = t.cpu().numpy()[:, :N]
    assert bk_batch_cases.TOL == DX_TOL
    for r in range(5):
        _assert_solution(X[r], ref[r], bk_batch_cases.TOL, (name, "solve_multi", r))


def _data(qp):
    return I.Data(qp["Q"], qp["c"], qp["lx"], qp["ux"], qp["A"], qp["lA"], qp["uA"], qp["C"], qp["d"])


def _compare(o, g, label):
    for got, ref in ((g.daff(), o.daff()), (g.dir(), o.dir())):
        so, sg = o.split(ref), o.split(got)
        for s in o.order:
            err = np.abs(sg[s] - so[s]).max()
            assert err < 1e-9 * max(1.0, np.abs(so[s]).max()), (label, s, err)
        assert np.abs(sg["x"] - so["x"]).max() < DX_TOL, label


@pytest.mark.parametrize("n,m,p,seed", C.STRUCTURED, ids=[f"n{c[0]}m{c[1]}" for c in C.STRUCTURED])
def test_structured_qp_steps(ctx, n, m, p, seed):
    qp = C.structured_qp(n, m, p, seed)
    o = oracle.OracleQP(qp, eq_none=True)
    g = I.Optimizer(n, m, p, ctx, equality_handling=I.EQ_NONE)
    g.load(_data(qp))
    assert np.array_equal(g.vars(), o.vars())
    for it in range(4):
        K = o.kkt()
        assert np.array_equal(g.kkt(), np.tril(K)), it  # bitwise, the zero block included
        Fo, po, io = oracle.bk_factor(K)
        assert io == 0
        for algo in (ctx.BK_WORKGROUP, ctx.BK_GRID):
            F, piv, info = _dev_factor(ctx, K, algo)
            assert np.array_equal(piv, po.astype(np.int32)), (it, algo)
            assert np.array_equal(np.tril(F), np.tril(Fo)), (it, algo)
            assert info == 0
        done, rec = o.iterate()
        assert not done
        g.step()
        s1 = g.scalars()
        for k in ("alpha_aff", "mu_aff", "sigma", "alpha"):
            assert abs(s1[k] - rec[k]) <= 1e-9 * max(1.0, abs(rec[k])), (it, k)
        _compare(o, g, f"iter {it}")
        g.set_vars(o.vars())


@pytest.mark.parametrize("n", sorted(C.STRUCTURED_BATCH))
def test_structured_qp_batch(ctx, n):
    n, m, p, seeds = C.STRUCTURED_BATCH[n]
    qps = [C.structured_qp(n, m, p, s) for s in seeds]
    assert len(qps) == 4
    bt = I.Batch(n, m, p, len(qps), ctx, equality_handling=I.EQ_NONE)
    for i, qp in enumerate(qps):
        bt.load_one(i, _data(qp))
    bt.initialize()
    orcs = [oracle.OracleQP(qp, eq_none=True) for qp in qps]
    for i, o in enumerate(orcs):
        assert np.array_equal(bt.state(i, 0), o.vars()), i
        assert np.array_equal(bt.kkt_of(i), np.tril(o.kkt())), i
    for it in range(4):
        for o in orcs:
            o.iterate()
        bt.step()
        for i, o in enumerate(orcs):
            got, ref = bt.state(i, 2), o.dir()
            assert np.abs(got - ref).max() < 1e-9 * max(1.0, np.abs(ref).max()), (it, i)
            assert np.abs(got[:n] - ref[:n]).max() < DX_TOL, (it, i)
            bt.set_state(i, o.vars())
