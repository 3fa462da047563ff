"""The adjoint Newton solve for a block of cotangent vectors on the device
(ipmz_qp_newton_adjoint_multi / ipmz_batch_newton_adjoint_multi:
Optimizer.newton_adjoint, Batch.newton_adjoint_all), through the public ABI only.

References (tests/newton_adjoint_cases.py): numpy.linalg.solve(J^T, -G^T)^T with
the dense Jacobian J of the full Newton system at the iterate read back from
the device (tests/test_oracle_newton_adjoint.py pins it to 1e-13 on the CPU);
for the formulations without a numpy J, the forward call of R = I_L, which this
feature leaves untouched.  Bound: the project's Newton-direction bar, 1e-10 per
row (nc.TOL, nc.row_err).  Every test prints its worst figure before it asserts.
"""
import numpy as np
import pytest

import newton_adjoint_cases as ac
import newton_multi_cases as nc
import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _single(c, ctx, eq_none=False, seed=nc.SEED, **kw):
    n, m, p = c[:3]
    g = I.Optimizer(n, m, p, ctx, equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION, **kw)
    g.generate(seed)
    return g


def _batch(c, ctx, eq_none=False, **kw):
    n, m, p, B, seed0 = c
    bt = I.Batch(n, m, p, B, ctx, equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION, **kw)
    bt.generate(seed0)
    return bt


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


def _call(g, X, adjoint, ldi=None, ldo=None, sI=None, sO=None, inplace=False, raw=False):
    """newton_adjoint(_all) -- or, adjoint=False, newton_solve(_all) with alpha = NULL -- of X ((nrhs, L), or
    (B, nrhs, L) for a batch).  Returns (Out, rc), or, raw=True, every buffer as the device left it."""
    batch = isinstance(g, I.Batch)
    X3 = np.asarray(X) if batch else np.asarray(X)[None]
    B, nrhs, L = X3.shape
    ldi = ldi or nc.even(L)
    ldo = ldi if inplace else (ldo or nc.even(L))
    hI = _pack(X3, ldi, sI)
    hO = hI if inplace else _pack(np.full_like(X3, NAN), ldo, sO)
    tI = _dev(hI)
    tO = tI if inplace else _dev(hO)
    if batch and adjoint:
        rc = g.newton_adjoint_all(tI.data_ptr(), tO.data_ptr(), nrhs, ldi, hI.shape[1], ldo, hO.shape[1])
    elif batch:
        rc = g.newton_solve_all(tI.data_ptr(), tO.data_ptr(), nrhs, ldi, hI.shape[1], ldo, hO.shape[1], None)
    elif adjoint:
        rc = g.newton_adjoint(tI.data_ptr(), tO.data_ptr(), nrhs, ldi, ldo)
    else:
        rc = g.newton_solve(tI.data_ptr(), tO.data_ptr(), nrhs, ldi, ldo, None)
    torch.cuda.synchronize()
    dO, dI = tO.cpu().numpy(), tI.cpu().numpy()
    Out = _unpack(dO, nrhs, L, ldo)
    if raw:
        return dict(Out=Out, rc=rc, bufO=dO, bufI=dI, hostI=hI, hostO=hO)
    return (Out, rc) if batch else (Out[0], rc)


def _adj(g, G, **kw):
    return _call(g, G, True, **kw)


def _fwd(g, R, **kw):
    return _call(g, R, False, **kw)


def _ok(rc, eq_none, B):
    if eq_none:
        rc, info = rc
        assert info.shape == (B,) and not info.any()
    assert rc == 0


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
@pytest.mark.parametrize("c", nc.SHAPES, ids=nc.case_id)
def test_random_rows_vs_transposed_jacobian(ctx, c, eq_none):
    q = nc.qp(*c)
    g = _single(c, ctx, eq_none)
    L = g.state_len
    assert L == nc.offsets(q, eq_none)[3]
    for label in ("initial", "after two steps"):
        v = g.vars()
        worst = {}
        for nrhs in nc.RHS_COUNTS:
            G = np.array(ac.rows(L)[0, :nrhs])
            W, rc = _adj(g, G)
            assert rc == 0
            worst[nrhs] = nc.row_err(W, ac.reference_adjoint(q, v, G, eq_none))
        print(f"{nc.case_id(c)} eq_none={eq_none} {label}: worst vs J^T reference {max(worst.values()):.3e} at nrhs "
              f"{max(worst, key=worst.get)} (bound {nc.TOL:.1e})", flush=True)
        for nrhs, e in worst.items():
            assert e <= nc.TOL, (label, nrhs, e)
        g.step()
        g.step()


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
            G = np.array(ac.rows(L, B)[:, :nrhs])
            W, rc = _adj(bt, G)
            _ok(rc, eq_none, B)
            for i, g in enumerate(singles):
                v = bt.state(i)
                g.set_vars(v)
                Ws, rcs = _adj(g, G[i])
                assert rcs == 0
                worst_single = max(worst_single, nc.row_err(W[i], Ws))
                worst_ref = max(worst_ref, nc.row_err(W[i], ac.reference_adjoint(nc.qp(n, m, p, seed0 + i), v, G[i],
                                                                                 eq_none)))
        print(f"{nc.case_id(c)} eq_none={eq_none} {label}: worst vs single solver {worst_single:.3e}, vs J^T "
              f"reference {worst_ref:.3e} (bound {nc.TOL:.1e})", flush=True)
        assert worst_single <= nc.TOL and worst_ref <= nc.TOL
        bt.step()
        bt.step()


# 2 ---------------------------------------------------------------------------
ABI_BOUNDS = {3: I.BOUNDS_BOTH, 1: I.BOUNDS_LOWER, 2: I.BOUNDS_UPPER, 0: I.BOUNDS_NONE}


def _abi(form):
    return dict(inequality_handling=I.INEQ_SLACKS if form.slacks else I.INEQ_SLACKED_SLACKS,
                inequality_bounds=ABI_BOUNDS[form.ineq_bounds], variable_bounds=ABI_BOUNDS[form.var_bounds])


# the FORMS list of tests/test_gpu_newton_multi.py: (tag, n, m, p, Optimizer keywords)
FORMS = [(tag, 48, m, 0, _abi(f)) for tag, m, f in (
    ("vlo", 16, oracle.Form(False, 3, 1)), ("vup", 16, oracle.Form(False, 3, 2)), ("vnone", 16, oracle.Form(False, 3, 0)),
    ("alo", 16, oracle.Form(False, 1, 3)), ("aup", 16, oracle.Form(False, 2, 3)), ("vlo0", 0, oracle.Form(False, 0, 1)),
    ("sl", 16, oracle.Form(True, 3, 3)), ("slbox", 0, oracle.Form(True, 0, 3)))] + [
    ("reg", 48, 16, 8, dict()),
    ("none", 48, 16, 8, dict(equality_handling=I.EQ_NONE)),
    ("pen", 48, 16, 8, dict(equality_handling=I.EQ_PENALTY)),
    ("pex", 48, 16, 8, dict(equality_handling=I.EQ_PENALTY_EXTRA_DUAL)),
    ("naive", 48, 16, 0, dict(inequality_handling=I.INEQ_NAIVE_SLACKS)),
    ("naivereg", 48, 16, 8, dict(inequality_handling=I.INEQ_NAIVE_SLACKS)),
]


@pytest.mark.parametrize("tag,n,m,p,kw", FORMS, ids=[f[0] for f in FORMS])
def test_every_served_formulation_vs_the_forward_call(ctx, tag, n, m, p, kw):
    """No numpy J for these forms: the forward call of R = I_L gives D_I (row j = column j of M), and
    Adj_ref[r][j] = D_I[j] . G[r].  At the initial iterate and after two steps."""
    g = I.Optimizer(n, m, p, ctx, **kw)
    g.generate(nc.SEED)
    L = g.state_len
    assert L <= 368
    G = np.array(ac.rows(L)[0])
    for label in ("initial", "after two steps"):
        D_I, rc = _fwd(g, np.eye(L))
        assert rc == 0
        W, rc = _adj(g, G)
        assert rc == 0
        ref = ac.identity_reference(D_I, G)
        bound = ac.identity_bound(D_I, G, ref)
        err = np.abs(W - np.asarray(ref, dtype=np.float64))
        err = np.where(np.isnan(err), np.inf, err)
        print(f"{tag} L={L} {label}: worst |Adj - Adj_ref| {err.max():.3e}, worst error / bound "
              f"{(err / bound).max():.3e} (bound min {bound.min():.3e})", flush=True)
        assert (err <= bound).all(), (tag, label)
        g.step()
        g.step()


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("ldlt", "bk"))
@pytest.mark.parametrize("c", nc.BATCHES, ids=nc.case_id)
def test_dot_product_identity_on_the_device(ctx, c, eq_none):
    """<g_a, Dir(r_b)> = <Adj(g_a), r_b> for all 17 x 17 pairs, both sides from the device."""
    B = c[3]
    bt = _batch(c, ctx, eq_none)
    L = bt.state_len
    G, R = np.array(ac.rows(L, B)), np.array(nc.rows(L, B))
    assert G.shape[1] == R.shape[1] == 17
    for label in ("initial", "after two steps"):
        Dir, rc = _fwd(bt, R)
        _ok(rc, eq_none, B)
        Adj, rc = _adj(bt, G)
        _ok(rc, eq_none, B)
        worst = 0.0
        for i in range(B):
            gap, bound = ac.dot_gap(G[i], Dir[i], Adj[i], R[i])
            gap = np.where(np.isnan(gap), np.inf, gap)
            worst = max(worst, float((gap / bound).max()))
        print(f"{nc.case_id(c)} eq_none={eq_none} {label}: worst |<g, Dir r> - <Adj g, r>| / bound {worst:.3e} "
              f"over {B} x 17 x 17 pairs", flush=True)
        assert worst <= 1.0
        bt.step()
        bt.step()


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
def test_rows_and_qps_are_independent_and_deterministic(ctx, eq_none):
    c = nc.SHAPES[1]
    g = _single(c, ctx, eq_none)
    L = g.state_len
    for nrhs in (3, 17):
        G = np.array(ac.rows(L)[0, :nrhs])
        W, _ = _adj(g, G)
        W2, _ = _adj(g, G)
        assert not np.isnan(W).any() and np.array_equal(W, W2), "same call twice"
        other = np.random.default_rng(5).standard_normal(G.shape) * 3.0
        for keep in (0, nrhs // 2, nrhs - 1):
            G2 = other.copy()
            G2[keep] = G[keep]
            W3, _ = _adj(g, G2)
            assert np.array_equal(W3[keep], W[keep]), (nrhs, keep)
    bc = nc.BATCHES[0]
    bt = _batch(bc, ctx, eq_none)
    B, Lb = bc[3], bt.state_len
    for nrhs in (3, 17):
        G = np.array(ac.rows(Lb, B)[:, :nrhs])
        W, _ = _adj(bt, G)
        W2, _ = _adj(bt, G)
        assert not np.isnan(W).any() and np.array_equal(W, W2), "same batch call twice"
        for keep in range(B):
            G2 = np.random.default_rng(6 + keep).standard_normal(G.shape) * 3.0
            G2[keep] = G[keep]
            W3, _ = _adj(bt, G2)
            assert np.array_equal(W3[keep], W[keep]), (nrhs, keep)
    print("independence and determinism: all bitwise equal", flush=True)


RPG_BITS = {1: 2097152, 8: 4194304, 2: 2097152 | 4194304}  # csrc/kernels.h IPMZ_DEBUG_NEWTON_RPG1 / RPG8 / both


@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
def test_rows_per_thread_choices_agree_bitwise(ctx, eq_none):
    """4 rows per thread by default; the debug bits select 1, 2 or 8.  Every choice gives every row the same
    bits, ragged last groups (3 and 17 rows) included."""
    g = _single(nc.SHAPES[2], ctx, eq_none)
    bt = _batch(nc.BATCHES[0], ctx, eq_none)
    for nrhs in (3, 17):
        G = np.array(ac.rows(g.state_len)[0, :nrhs])
        Gb = np.array(ac.rows(bt.state_len, bt.batch)[:, :nrhs])
        W, _ = _adj(g, G)
        Wb, _ = _adj(bt, Gb)
        assert not np.isnan(W).any() and not np.isnan(Wb).any()
        for rp, bits in RPG_BITS.items():
            I.debug_inject(bits)
            try:
                W2, _ = _adj(g, G)
                Wb2, _ = _adj(bt, Gb)
                Wi, _ = _adj(g, G, inplace=True)
            finally:
                I.debug_inject(0)
            assert np.array_equal(W2, W) and np.array_equal(Wi, W), (rp, nrhs)
            assert np.array_equal(Wb2, Wb), (rp, nrhs)
    print("rows per thread 1 / 2 / 4 / 8: all bitwise equal", flush=True)


@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
def test_workspace_growth(ctx, eq_none):
    c = nc.SHAPES[1]
    g = _single(c, ctx, eq_none)
    bt = _batch(nc.BATCHES[0], ctx, eq_none)
    L, Lb, B = g.state_len, bt.state_len, bt.batch
    for nrhs in (3, 17, 3):
        G = np.array(ac.rows(L)[0, :nrhs])
        W, _ = _adj(g, G)
        Wf, _ = _adj(_single(c, ctx, eq_none), G)
        assert not np.isnan(W).any() and np.array_equal(W, Wf), nrhs
        Gb = np.array(ac.rows(Lb, B)[:, :nrhs])
        W, _ = _adj(bt, Gb)
        Wf, _ = _adj(_batch(nc.BATCHES[0], ctx, eq_none), Gb)
        assert not np.isnan(W).any() and np.array_equal(W, Wf), nrhs
    print("workspace growth 3 -> 17 -> 3: equal to fresh solvers, bitwise", flush=True)


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
def test_layout_padding_and_in_place(ctx, eq_none):
    c = nc.SHAPES[2]  # with EqualityHandling::None L is odd
    g = _single(c, ctx, eq_none)
    L, nrhs = g.state_len, 6
    G = np.array(ac.rows(L)[0, :nrhs])
    W, _ = _adj(g, G)
    assert not np.isnan(W).any(), "every element of every row is written"
    ldo = nc.even(L) + 2
    out = _adj(g, G, ldi=nc.even(L) + 6, ldo=ldo, raw=True)
    assert np.array_equal(out["Out"][0], W)
    assert np.array_equal(out["bufI"].view(np.int64), out["hostI"].view(np.int64)), "G is never written"
    pad = np.ones(out["bufO"].shape, bool)
    for r in range(nrhs):
        pad[0, r * ldo:r * ldo + L] = False
    assert not np.isnan(out["bufO"][~pad]).any(), "no NaN left inside rows"
    assert np.isnan(out["bufO"][pad]).all() and np.array_equal(out["bufO"].view(np.int64)[pad],
                                                                out["hostO"].view(np.int64)[pad]), "padding keeps its bits"
    Wi, _ = _adj(g, G, inplace=True)
    assert np.array_equal(Wi, W), "in place"
    Wi, _ = _adj(g, G, ldi=nc.even(L) + 4, inplace=True)
    assert np.array_equal(Wi, W), "in place, padded"
    # batches: sG, sO with slack
    bc = nc.BATCHES[0]
    bt = _batch(bc, ctx, eq_none)
    B, Lb = bc[3], bt.state_len
    Gb = np.array(ac.rows(Lb, B)[:, :nrhs])
    Wb, _ = _adj(bt, Gb)
    assert not np.isnan(Wb).any()
    ldg, ldo = nc.even(Lb) + 2, nc.even(Lb) + 4
    out = _adj(bt, Gb, ldi=ldg, ldo=ldo, sI=nrhs * ldg + 10, sO=nrhs * ldo + 6, raw=True)
    assert np.array_equal(out["Out"], Wb)
    assert np.array_equal(out["bufI"].view(np.int64), out["hostI"].view(np.int64)), "G is never written"
    pad = np.ones(out["bufO"].shape, bool)
    for r in range(nrhs):
        pad[:, r * ldo:r * ldo + Lb] = False
    assert not np.isnan(out["bufO"][~pad]).any()
    assert np.array_equal(out["bufO"].view(np.int64)[pad], out["hostO"].view(np.int64)[pad])
    Wi, _ = _adj(bt, Gb, inplace=True)
    assert np.array_equal(Wi, Wb), "batch in place"
    Wi, _ = _adj(bt, Gb, ldi=ldg, sI=nrhs * ldg + 10, inplace=True)
    assert np.array_equal(Wi, Wb), "batch in place, padded"
    print("layout: strides, padding and in place all bitwise equal", flush=True)


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
    rows, rrows = ac.rows(L, a.batch if flags else 1), nc.rows(L, a.batch if flags else 1)
    for k in range(3):
        nrhs = (3, 17, 1)[k]
        G = np.array(rows[:, :nrhs]) if flags else np.array(rows[0, :nrhs])
        R = np.array(rrows[:, :nrhs]) if flags else np.array(rrows[0, :nrhs])
        D0, _ = _fwd(b, R)
        _adj(b, G)
        D1, _ = _fwd(b, R)
        assert np.array_equal(D0, D1), "the forward call's output after an adjoint call"
        a.step(flags)
        b.step(flags)
        _adj(b, G, inplace=True)
    if flags:
        assert a.last_step_graph() and b.last_step_graph()
    for x, y in zip(_everything(a), _everything(b)):
        assert np.array_equal(x, y, equal_nan=True), kind
    print(f"{kind}: vars, daff, dir, residuals and scalars bitwise equal after three steps", flush=True)


# 7 ---------------------------------------------------------------------------
def test_errors(ctx):
    c = nc.SHAPES[1]
    n, m, p = c
    g = _single(c, ctx)
    L = g.state_len
    ld = nc.even(L)
    tG = _dev(np.zeros(4 * (ld + 8)))
    tO = _dev(np.full(4 * (ld + 8), NAN))
    G, O = tG.data_ptr(), tO.data_ptr()

    def invalid(f, *a):
        with pytest.raises(I.IpmzError, match="invalid argument"):
            f(*a)

    def state(f, *a):
        with pytest.raises(I.IpmzError, match="bad state"):
            f(*a)

    invalid(g.newton_adjoint, G, O, 2, ld, ld + 1)    # odd ldo
    invalid(g.newton_adjoint, G, O, 2, ld + 1, ld)    # odd ldg
    invalid(g.newton_adjoint, G, O, 2, L - 2, ld)     # ldg < L
    invalid(g.newton_adjoint, G, O, 2, ld, L - 2)     # ldo < L
    invalid(g.newton_adjoint, G, O + 8, 2, ld, ld)    # misaligned Out
    invalid(g.newton_adjoint, G + 8, O, 2, ld, ld)    # misaligned G
    invalid(g.newton_adjoint, G, O, -1, ld, ld)
    # nrhs = 0: the info word, nothing touched
    assert g.newton_adjoint(G, O, 0, ld, ld) == 0
    assert g.newton_adjoint(None, None, 0, ld, ld) == 0
    torch.cuda.synchronize()
    assert np.isnan(tO.cpu().numpy()).all() and not tG.cpu().numpy().any()
    g.set_reduction(I.REDUCTION_NORMAL)
    invalid(g.newton_adjoint, G, O, 2, ld, ld)
    g.set_reduction(I.REDUCTION_AUGMENTED)
    g.set_mixed_precision(True)
    invalid(g.newton_adjoint, G, O, 2, ld, ld)
    g.set_mixed_precision(False)
    assert g.newton_adjoint(G, O, 2, ld, ld) == 0
    for kw in (dict(equality_handling=I.EQ_SLACKED_SLACKS),
               dict(equality_handling=I.EQ_NAIVE_SLACKS, inequality_handling=I.INEQ_NAIVE_SLACKS)):
        e = I.Optimizer(n, m, p, ctx, **kw)
        e.generate(nc.SEED)
        big = _dev(np.zeros(2 * nc.even(e.state_len)))
        invalid(e.newton_adjoint, big.data_ptr(), big.data_ptr(), 2, nc.even(e.state_len), nc.even(e.state_len))
    fresh = I.Optimizer(n, m, p, ctx)
    state(fresh.newton_adjoint, G, O, 2, ld, ld)      # before a load
    # batches
    bc = nc.BATCHES[0]
    bt = _batch(bc, ctx)
    B = bc[3]
    tGb = _dev(np.zeros(B * (2 * ld + 8)))
    tOb = _dev(np.zeros(B * (2 * ld + 8)))
    Gb, Ob = tGb.data_ptr(), tOb.data_ptr()
    assert bt.newton_adjoint_all(Gb, Ob, 2, ld, 2 * ld, ld, 2 * ld) == 0
    invalid(bt.newton_adjoint_all, Gb, Ob, 2, ld, 2 * ld, ld, 2 * ld - 2)   # sO < nrhs * ldo
    invalid(bt.newton_adjoint_all, Gb, Ob, 2, ld, 2 * ld + 1, ld, 2 * ld)   # odd sG
    invalid(bt.newton_adjoint, Gb, Ob, 2, ld, ld)                          # the single call on a batch
    q = nc.qp(n, m, p, bc[4])
    bt.load_one(0, I.Data(q["Q"], q["c"], q["lx"], q["ux"], q["A"], q["lA"], q["uA"], q["C"], q["d"]))
    state(bt.newton_adjoint_all, Gb, Ob, 2, ld, 2 * ld, ld, 2 * ld)         # between load_one and initialize
    bt.initialize()
    assert bt.newton_adjoint_all(Gb, Ob, 2, ld, 2 * ld, ld, 2 * ld) == 0
    one = I.Batch(n, m, p, 1, ctx)  # a batch of one forwards to the single call: sG, sO ignored
    one.generate(nc.SEED)
    assert one.newton_adjoint_all(G, O, 2, ld, 0, ld, 0) == 0
    print("errors: every refusal of the forward pair, and nrhs = 0 touching nothing", flush=True)
