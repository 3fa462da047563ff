"""Newton directions for a block of residual vectors on the device
(ipmz_qp_newton_solve_multi / ipmz_batch_newton_solve_multi:
Optimizer.newton_solve, Batch.newton_solve_all), through the public ABI only.

Reference (tests/newton_multi_cases.py): the dense Jacobian J of the full
Newton system at the iterate read back from the device, numpy.linalg.solve(J,
-R^T), and get_max_step_ in numpy; bound |d - d_ref|_inf <= 1e-10 max(1,
|d_ref|_inf) per row.  tests/test_oracle_newton_multi.py pins that reference
to the oracle's own step to 1e-13 on the CPU, so 1e-10 is the device's
summation order and reciprocals.  Every test prints its worst figure before it
asserts.
"""
import numpy as np
import pytest

import newton_multi_cases as nc
import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

NAN = float("nan")
ALPHA_TOL = 1e-9  # the step-control bar of tests/test_gpu_headline.py


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _single(c, ctx, eq_none=False, seed=nc.SEED, **kw):
    n, m, p = c[:3]
    g = I.Optimizer(n, m, p, ctx, equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION, **kw)
    g.generate(seed)
    return g


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _pack(R, ld, stride=None, fill=NAN):
    """(B, nrhs, L) rows laid out with row stride ld and QP stride `stride`; the padding holds `fill`."""
    B, nrhs, L = R.shape
    stride = nrhs * ld if stride is None else stride
    host = np.full((B, max(stride, 2)), fill)
    for q in range(B):
        for r in range(nrhs):
            host[q, r * ld:r * ld + L] = R[q, r]
    return host


def _unpack(buf, nrhs, L, ld):
    return np.stack([[buf[q, r * ld:r * ld + L] for r in range(nrhs)] for q in range(buf.shape[0])])


def _solve(g, R, ldr=None, ldd=None, sR=None, sD=None, alpha=True, inplace=False, raw=False):
    """newton_solve / newton_solve_all of R ((nrhs, L), or (B, nrhs, L) for a batch).  Returns (Dir,
    alpha, rc) -- or, raw=True, every buffer as the device left it."""
    batch = isinstance(g, I.Batch)
    R3 = np.asarray(R) if batch else np.asarray(R)[None]
    B, nrhs, L = R3.shape
    ldr = ldr or nc.even(L)
    ldd = ldr if inplace else (ldd or nc.even(L))
    hR = _pack(R3, ldr, sR)
    hD = hR if inplace else _pack(np.full_like(R3, NAN), ldd, sD)
    tR = _dev(hR)
    tD = tR if inplace else _dev(hD)
    tA = _dev(np.full(max(B * nrhs, 1), NAN)) if alpha else None
    ap = tA.data_ptr() if alpha else None
    if batch:
        rc = g.newton_solve_all(tR.data_ptr(), tD.data_ptr(), nrhs, ldr, hR.shape[1], ldd, hD.shape[1], ap)
    else:
        rc = g.newton_solve(tR.data_ptr(), tD.data_ptr(), nrhs, ldr, ldd, ap)
    torch.cuda.synchronize()
    dD, dR = tD.cpu().numpy(), tR.cpu().numpy()
    D = _unpack(dD, nrhs, L, ldd)
    A = tA.cpu().numpy()[:B * nrhs].reshape(B, nrhs) if alpha else None
    if raw:
        return dict(D=D, alpha=A, rc=rc, bufD=dD, bufR=dR, hostR=hR, hostD=hD)
    return (D, A, rc) if batch else (D[0], None if A is None else A[0], rc)


def _alpha_check(q, v, D, A, eq_none, label):
    """alpha against get_max_step_ in numpy of the device's own direction: the same division of
    the same numbers.  Equal bits expected; a device division may differ in the last bit."""
    worst = 0
    for r in range(D.shape[0]):
        worst = max(worst, nc.ulps(A[r], nc.max_step_numpy(q, v, D[r], eq_none)))
    print(f"{label}: alpha vs numpy get_max_step_, worst {worst} ulp (bound 4)", flush=True)
    assert worst <= 4, label


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
@pytest.mark.parametrize("c", nc.SHAPES, ids=nc.case_id)
def test_random_rows_vs_jacobian(ctx, c, eq_none):
    q = nc.qp(*c)
    g = _single(c, ctx, eq_none)
    L = g.state_len
    assert L == nc.offsets(q, eq_none)[3]
    for label in ("initial", "after two steps"):
        v = g.vars()
        worst = {}
        for nrhs in nc.RHS_COUNTS:
            R = np.array(nc.rows(L)[0, :nrhs])
            D, A, rc = _solve(g, R)
            assert rc == 0
            worst[nrhs] = nc.row_err(D, nc.reference(q, v, R, eq_none))
            _alpha_check(q, v, D, A, eq_none, f"{nc.case_id(c)} {label} nrhs {nrhs}")
        print(f"{nc.case_id(c)} eq_none={eq_none} {label}: worst vs J reference {max(worst.values()):.3e} at nrhs "
              f"{max(worst, key=worst.get)} (bound {nc.TOL:.1e})", flush=True)
        for nrhs, e in worst.items():
            assert e <= nc.TOL, (label, nrhs, e)
        g.step()
        g.step()


@pytest.mark.parametrize("c", nc.RATIO_SHAPES, ids=nc.case_id)
def test_step_length_kernel_threshold(ctx, c):
    """Both widths of the step-length kernel (256 threads per row up to n + m = 2048, 1024 beyond): alpha
    against numpy on the device's own directions, and the residual row against the step.  (No J here: L > 10^4.)"""
    q = nc.qp(*c)
    g = _single(c, ctx)
    L = g.state_len
    v, R0 = g.vars(), g.residuals()
    R = np.stack([nc.rows(L)[0, 0], R0, nc.rows(L)[0, 1]])
    D, A, rc = _solve(g, R)
    assert rc == 0
    _alpha_check(q, v, D, A, False, nc.case_id(c))
    g.step()
    e, da = nc.row_err(D[1][None], g.daff()[None]), abs(A[1] - g.scalars()["alpha_aff"])
    print(f"{nc.case_id(c)}: residual row vs step daff {e:.3e} (bound {nc.TOL:.1e}), |alpha - alpha_aff| {da:.3e} "
          f"(bound {ALPHA_TOL:.1e})", flush=True)
    assert e <= nc.TOL and da <= ALPHA_TOL


# 2 ---------------------------------------------------------------------------
ABI_BOUNDS = {3: I.BOUNDS_BOTH, 1: I.BOUNDS_LOWER, 2: I.BOUNDS_UPPER, 0: I.BOUNDS_NONE}


def _abi(form):
    return dict(inequality_handling=I.INEQ_SLACKS if form.slacks else I.INEQ_SLACKED_SLACKS,
                inequality_bounds=ABI_BOUNDS[form.ineq_bounds], variable_bounds=ABI_BOUNDS[form.var_bounds])


# the formulation list of tests/test_gpu_formulations.py (FORMS, EQ_CASES) minus the two equality-slack handlings:
# (tag, n, m, p, Optimizer keywords, oracle factory)
FORMS = [(tag, 48, m, 0, _abi(f), (lambda f: lambda qp: oracle.OracleQP(qp, form=f))(f)) for tag, m, f in (
    ("vlo", 16, oracle.Form(False, 3, 1)), ("vup", 16, oracle.Form(False, 3, 2)), ("vnone", 16, oracle.Form(False, 3, 0)),
    ("alo", 16, oracle.Form(False, 1, 3)), ("aup", 16, oracle.Form(False, 2, 3)), ("vlo0", 0, oracle.Form(False, 0, 1)),
    ("sl", 16, oracle.Form(True, 3, 3)), ("slbox", 0, oracle.Form(True, 0, 3)))] + [
    ("reg", 48, 16, 8, dict(), lambda qp: oracle.OracleQP(qp)),
    ("none", 48, 16, 8, dict(equality_handling=I.EQ_NONE), lambda qp: oracle.OracleQP(qp, eq_none=True)),
    ("pen", 48, 16, 8, dict(equality_handling=I.EQ_PENALTY), lambda qp: oracle.OracleQP(qp, eq_penalty=True)),
    ("pex", 48, 16, 8, dict(equality_handling=I.EQ_PENALTY_EXTRA_DUAL), lambda qp: oracle.OracleQP(qp, eq_penalty=True)),
    ("naive", 48, 16, 0, dict(inequality_handling=I.INEQ_NAIVE_SLACKS),
     lambda qp: oracle.OracleQP(qp, form=oracle.Form(naive=True))),
    ("naivereg", 48, 16, 8, dict(inequality_handling=I.INEQ_NAIVE_SLACKS),
     lambda qp: oracle.OracleQP(qp, form=oracle.Form(naive=True))),
]


@pytest.mark.parametrize("tag,n,m,p,kw,mk", FORMS, ids=[f[0] for f in FORMS])
def test_parity_with_the_step_and_the_oracle(ctx, tag, n, m, p, kw, mk):
    g = I.Optimizer(n, m, p, ctx, **kw)
    g.generate(nc.SEED)
    o = mk(nc.qp(n, m, p))
    assert np.array_equal(g.vars(), o.vars())
    L = g.state_len
    R0 = g.residuals()
    D1, A1, rc = _solve(g, R0[None])
    assert rc == 0
    R3 = np.stack([nc.rows(L)[0, 0], R0, nc.rows(L)[0, 1]])
    D3, A3, rc = _solve(g, R3)
    assert rc == 0
    g.step()
    o.iterate()
    alpha_aff = g.scalars()["alpha_aff"]
    figs = {}
    for name, d, a in (("nrhs 1", D1[0], A1[0]), ("nrhs 3 middle row", D3[1], A3[1])):
        figs[name] = (nc.row_err(d[None], g.daff()[None]), nc.row_err(d[None], o.daff()[None]), abs(a - alpha_aff))
    print(f"{tag}: (vs step daff, vs oracle daff, |alpha - alpha_aff|) " +
          "; ".join(f"{k}: {a:.3e} {b:.3e} {c:.3e}" for k, (a, b, c) in figs.items()) +
          f" (bounds {nc.TOL:.1e}, {nc.TOL:.1e}, {ALPHA_TOL:.1e})", flush=True)
    for k, (a, b, c) in figs.items():
        assert a <= nc.TOL and b <= nc.TOL, (tag, k, a, b)
        assert c <= ALPHA_TOL * max(1.0, abs(alpha_aff)), (tag, k, c)


# 3 ---------------------------------------------------------------------------
def _batch(c, ctx, eq_none=False, **kw):
    n, m, p, B, seed0 = c
    bt = I.Batch(n, m, p, B, ctx, equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION, **kw)
    bt.generate(seed0)
    return bt


@pytest.mark.parametrize("eq_none", (False, True), ids=("ldlt", "bk"))
@pytest.mark.parametrize("c", nc.BATCHES, ids=nc.case_id)
def test_batches(ctx, c, eq_none):
    n, m, p, B, seed0 = c
    bt = _batch(c, ctx, eq_none)
    L = bt.state_len
    singles = [_single(c, ctx, eq_none, seed=seed0 + i) for i in range(B)]
    for label in ("initial", "after two steps"):
        worst_single = worst_ref = 0.0
        for nrhs in nc.RHS_COUNTS:
            R = np.array(nc.rows(L, B)[:, :nrhs])
            D, A, rc = _solve(bt, R)
            if eq_none:
                rc, info = rc
                assert rc == 0 and info.shape == (B,) and not info.any()
            else:
                assert rc == 0
            for i, g in enumerate(singles):
                v = bt.state(i)
                g.set_vars(v)
                Ds, As, rcs = _solve(g, R[i])
                assert rcs == 0
                worst_single = max(worst_single, nc.row_err(D[i], Ds))
                worst_ref = max(worst_ref, nc.row_err(D[i], nc.reference(nc.qp(n, m, p, seed0 + i), v, R[i], eq_none)))
                _alpha_check(nc.qp(n, m, p, seed0 + i), v, D[i], A[i], eq_none, f"batch QP {i} {label} nrhs {nrhs}")
        print(f"{nc.case_id(c)} eq_none={eq_none} {label}: worst vs single solver {worst_single:.3e}, vs J reference "
              f"{worst_ref:.3e} (bound {nc.TOL:.1e})", flush=True)
        assert worst_single <= nc.TOL and worst_ref <= nc.TOL
        bt.step()
        bt.step()


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
def test_rows_and_qps_are_independent_and_deterministic(ctx, eq_none):
    c = nc.SHAPES[1]
    g = _single(c, ctx, eq_none)
    L = g.state_len
    for nrhs in (3, 17):
        R = np.array(nc.rows(L)[0, :nrhs])
        D, A, _ = _solve(g, R)
        D2, A2, _ = _solve(g, R)
        assert np.array_equal(D, D2) and np.array_equal(A, A2), "same call twice"
        other = np.random.default_rng(5).standard_normal(R.shape) * 3.0
        for keep in (0, nrhs // 2, nrhs - 1):
            R2 = other.copy()
            R2[keep] = R[keep]
            D3, A3, _ = _solve(g, R2)
            assert np.array_equal(D3[keep], D[keep]) and A3[keep] == A[keep], (nrhs, keep)
    bc = nc.BATCHES[0]
    bt = _batch(bc, ctx, eq_none)
    B, Lb = bc[3], bt.state_len
    for nrhs in (3, 17):
        R = np.array(nc.rows(Lb, B)[:, :nrhs])
        D, A, _ = _solve(bt, R)
        D2, A2, _ = _solve(bt, R)
        assert np.array_equal(D, D2) and np.array_equal(A, A2), "same batch call twice"
        for keep in range(B):
            R2 = np.random.default_rng(6 + keep).standard_normal(R.shape) * 3.0
            R2[keep] = R[keep]
            D3, A3, _ = _solve(bt, R2)
            assert np.array_equal(D3[keep], D[keep]) and np.array_equal(A3[keep], A[keep]), (nrhs, keep)
    print("independence and determinism: all bitwise equal", flush=True)


RPG_BITS = {1: 2097152, 8: 4194304, 2: 2097152 | 4194304}  # csrc/kernels.h IPMZ_DEBUG_NEWTON_RPG1 / RPG8 / both


@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
def test_rows_per_thread_choices_agree_bitwise(ctx, eq_none):
    """The element-wise kernels take 4 rows per thread; the debug bits select 1, 2 or 8 (the A/B of
    tools/newton_multi_bench.py).  Every choice gives every row the same bits, ragged last groups included."""
    g = _single(nc.SHAPES[2], ctx, eq_none)
    bt = _batch(nc.BATCHES[0], ctx, eq_none)
    for nrhs in (3, 17):
        R = np.array(nc.rows(g.state_len)[0, :nrhs])
        Rb = np.array(nc.rows(bt.state_len, bt.batch)[:, :nrhs])
        D, A, _ = _solve(g, R)
        Db, Ab, _ = _solve(bt, Rb)
        for rp, bits in RPG_BITS.items():
            I.debug_inject(bits)
            try:
                D2, A2, _ = _solve(g, R)
                Db2, Ab2, _ = _solve(bt, Rb)
                Di, _, _ = _solve(g, R, inplace=True)
            finally:
                I.debug_inject(0)
            assert np.array_equal(D2, D) and np.array_equal(A2, A) and np.array_equal(Di, D), (rp, nrhs)
            assert np.array_equal(Db2, Db) and np.array_equal(Ab2, Ab), (rp, nrhs)
    print("rows per thread 1 / 2 / 4 / 8: all bitwise equal", flush=True)


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
def test_layout_padding_in_place_and_null_alpha(ctx, eq_none):
    c = nc.SHAPES[2]  # with EqualityHandling::None L is odd
    g = _single(c, ctx, eq_none)
    L, nrhs = g.state_len, 6
    R = np.array(nc.rows(L)[0, :nrhs])
    D, A, _ = _solve(g, R)
    out = _solve(g, R, ldr=nc.even(L) + 6, ldd=nc.even(L) + 2, raw=True)
    assert np.array_equal(out["D"][0], D) and np.array_equal(out["alpha"][0], A)
    assert np.array_equal(out["bufR"], out["hostR"], equal_nan=True), "R is never written"
    ldd = nc.even(L) + 2
    pad = np.ones(out["bufD"].shape, bool)
    for r in range(nrhs):
        pad[0, r * ldd:r * ldd + L] = False
    assert np.isnan(out["bufD"][pad]).all() and np.array_equal(out["bufD"].view(np.int64)[pad],
                                                                out["hostD"].view(np.int64)[pad]), "padding keeps its bits"
    Dn, _, _ = _solve(g, R, alpha=False)
    assert np.array_equal(Dn, D), "alpha = NULL"
    Di, Ai, _ = _solve(g, R, inplace=True)
    assert np.array_equal(Di, D) and np.array_equal(Ai, A), "in place"
    Di, Ai, _ = _solve(g, R, ldr=nc.even(L) + 4, inplace=True)
    assert np.array_equal(Di, D) and np.array_equal(Ai, A), "in place, padded"
    # batches: sR, sD with slack
    bc = nc.BATCHES[0]
    bt = _batch(bc, ctx, eq_none)
    B, Lb = bc[3], bt.state_len
    Rb = np.array(nc.rows(Lb, B)[:, :nrhs])
    Db, Ab, _ = _solve(bt, Rb)
    ldr, ldd = nc.even(Lb) + 2, nc.even(Lb) + 4
    out = _solve(bt, Rb, ldr=ldr, ldd=ldd, sR=nrhs * ldr + 10, sD=nrhs * ldd + 6, raw=True)
    assert np.array_equal(out["D"], Db) and np.array_equal(out["alpha"], Ab)
    assert np.array_equal(out["bufR"], out["hostR"], equal_nan=True)
    pad = np.ones(out["bufD"].shape, bool)
    for r in range(nrhs):
        pad[:, r * ldd:r * ldd + Lb] = False
    assert np.array_equal(out["bufD"].view(np.int64)[pad], out["hostD"].view(np.int64)[pad])
    Di, Ai, _ = _solve(bt, Rb, ldr=ldr, sR=nrhs * ldr + 10, inplace=True)
    assert np.array_equal(Di, Db) and np.array_equal(Ai, Ab), "batch in place"
    Dn, _, _ = _solve(bt, Rb, alpha=False)
    assert np.array_equal(Dn, Db)
    print("layout: strides, padding, in place and alpha = NULL all bitwise equal", flush=True)


# 6 ---------------------------------------------------------------------------
def _everything(g):
    if isinstance(g, I.Batch):
        return [g.state(i, w) for i in range(g.batch) for w in range(4)] + [g.batch_scalars()]
    return [g.vars(), g.daff(), g.dir(), g.residuals(), np.array(list(g.scalars().values()))]


@pytest.mark.parametrize("kind", ("single_reg", "single_none", "batch_reg_graph", "batch_none_graph"))
def test_nothing_else_moves(ctx, kind):
    eq_none = "none" in kind
    if kind.startswith("single"):
        a, b = (_single(nc.SHAPES[1], ctx, eq_none) for _ in range(2))
        flags = 0
    else:
        a, b = (_batch(nc.BATCHES[0], ctx, eq_none) for _ in range(2))
        flags = I.STEP_GRAPH
    L = a.state_len
    rows = nc.rows(L, a.batch if flags else 1)
    for k in range(3):
        R = np.array(rows[:, :(3, 17, 1)[k]]) if flags else np.array(rows[0, :(3, 17, 1)[k]])
        _solve(b, R)
        a.step(flags)
        b.step(flags)
        _solve(b, R, inplace=True)
    if flags:
        assert a.last_step_graph() and b.last_step_graph()
    for x, y in zip(_everything(a), _everything(b)):
        assert np.array_equal(x, y, equal_nan=True), kind
    print(f"{kind}: vars, daff, dir, residuals and scalars bitwise equal after three steps", flush=True)


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
def test_workspace_growth(ctx, eq_none):
    c = nc.SHAPES[1]
    g = _single(c, ctx, eq_none)
    bt = _batch(nc.BATCHES[0], ctx, eq_none)
    L, Lb, B = g.state_len, bt.state_len, bt.batch
    for nrhs in (3, 17, 3):
        R = np.array(nc.rows(L)[0, :nrhs])
        D, A, _ = _solve(g, R)
        Df, Af, _ = _solve(_single(c, ctx, eq_none), R)
        assert np.array_equal(D, Df) and np.array_equal(A, Af), nrhs
        Rb = np.array(nc.rows(Lb, B)[:, :nrhs])
        D, A, _ = _solve(bt, Rb)
        Df, Af, _ = _solve(_batch(nc.BATCHES[0], ctx, eq_none), Rb)
        assert np.array_equal(D, Df) and np.array_equal(A, Af), nrhs
    print("workspace growth 3 -> 17 -> 3: equal to fresh solvers, bitwise", flush=True)


# 8 ---------------------------------------------------------------------------
def test_errors(ctx):
    c = nc.SHAPES[1]
    n, m, p = c
    g = _single(c, ctx)
    L = g.state_len
    ld = nc.even(L)
    tR = _dev(np.zeros(4 * (ld + 8)))
    tD = _dev(np.full(4 * (ld + 8), NAN))
    tA = _dev(np.full(4, NAN))
    R, D, A = tR.data_ptr(), tD.data_ptr(), tA.data_ptr()

    def invalid(f, *a):
        with pytest.raises(I.IpmzError, match="invalid argument"):
            f(*a)

    def state(f, *a):
        with pytest.raises(I.IpmzError, match="bad state"):
            f(*a)

    invalid(g.newton_solve, R, D, 2, ld, ld + 1, A)    # odd ldd
    invalid(g.newton_solve, R, D, 2, L - 2, ld, A)     # ldr < L
    invalid(g.newton_solve, R, D + 8, 2, ld, ld, A)    # misaligned Dir
    invalid(g.newton_solve, R, D, -1, ld, ld, A)
    # nrhs = 0: the info word, nothing touched
    assert g.newton_solve(R, D, 0, ld, ld, A) == 0
    assert g.newton_solve(None, None, 0, ld, ld, None) == 0
    torch.cuda.synchronize()
    assert np.isnan(tD.cpu().numpy()).all() and np.isnan(tA.cpu().numpy()).all() and not tR.cpu().numpy().any()
    g.set_reduction(I.REDUCTION_NORMAL)
    invalid(g.newton_solve, R, D, 2, ld, ld, A)
    g.set_reduction(I.REDUCTION_AUGMENTED)
    g.set_mixed_precision(True)
    invalid(g.newton_solve, R, D, 2, ld, ld, A)
    g.set_mixed_precision(False)
    assert g.newton_solve(R, D, 2, ld, ld, A) == 0
    for kw in (dict(equality_handling=I.EQ_SLACKED_SLACKS),
               dict(equality_handling=I.EQ_NAIVE_SLACKS, inequality_handling=I.INEQ_NAIVE_SLACKS)):
        e = I.Optimizer(n, m, p, ctx, **kw)
        e.generate(nc.SEED)
        big = _dev(np.zeros(2 * nc.even(e.state_len)))
        invalid(e.newton_solve, big.data_ptr(), big.data_ptr(), 2, nc.even(e.state_len), nc.even(e.state_len), None)
    fresh = I.Optimizer(n, m, p, ctx)
    state(fresh.newton_solve, R, D, 2, ld, ld, A)      # before a load
    # batches
    bc = nc.BATCHES[0]
    bt = _batch(bc, ctx)
    B = bc[3]
    tRb = _dev(np.zeros(B * (2 * ld + 8)))
    tDb = _dev(np.zeros(B * (2 * ld + 8)))
    Rb, Db = tRb.data_ptr(), tDb.data_ptr()
    assert bt.newton_solve_all(Rb, Db, 2, ld, 2 * ld, ld, 2 * ld, None) == 0
    invalid(bt.newton_solve_all, Rb, Db, 2, ld, 2 * ld, ld, 2 * ld - 2, None)   # sD < nrhs * ldd
    invalid(bt.newton_solve_all, Rb, Db, 2, ld, 2 * ld + 1, ld, 2 * ld, None)   # odd sR
    invalid(bt.newton_solve, Rb, Db, 2, ld, ld, None)                          # the single call on a batch
    q = nc.qp(n, m, p, bc[4])
    bt.load_one(0, I.Data(q["Q"], q["c"], q["lx"], q["ux"], q["A"], q["lA"], q["uA"], q["C"], q["d"]))
    state(bt.newton_solve_all, Rb, Db, 2, ld, 2 * ld, ld, 2 * ld, None)         # between load_one and initialize
    bt.initialize()
    assert bt.newton_solve_all(Rb, Db, 2, ld, 2 * ld, ld, 2 * ld, None) == 0
    one = I.Batch(n, m, p, 1, ctx)  # a batch of one forwards to the single call: sR, sD ignored
    one.generate(nc.SEED)
    assert one.newton_solve_all(R, D, 2, ld, 0, ld, 0, A) == 0
