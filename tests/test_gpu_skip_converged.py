"""IPMZ_STEP_SKIP_CONVERGED: a converged QP of a batch takes no part in any launch of a step.

The reference is the flag-off step of the same build.  Two solvers A (flags 0) and S (the skip flag) hold the same
data and are stepped one step at a time; after every step the three state blocks (iterate, affine direction,
direction: ipmz_batch_copy_state) and the scalar blocks of all QPs are read.  With c_q the first step after which A
shows QP q converged: up to c_q S is A bit for bit, after it S keeps its own bits of step c_q (and A's iterate, which
the flag-off step freezes too), and S's IPMZ_SC_STEPS is c_q.  Everything here is an equality of bits: no tolerance.

The stagger is made, not hoped for: slots 2i and 2i + 1 hold the same QP, and after 3 steps the odd slots of both
solvers go back to their initial iterate, so an odd slot converges 3 steps after its even twin.
"""
import ctypes

import numpy as np
import pytest

import newton_multi_cases as nc

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

SEED0 = 1000
RESET_AFTER = 3               # the odd slots restart after this many steps
TAIL = 3                      # steps past the last convergence: every QP is skipped at least this often
T_MAX = 40
DEBUG_NO_FUSED_SOLVES = 16384  # csrc/kernels.h IPMZ_DEBUG_NO_FUSED_SOLVES: the solves, mid and post as launches
DEBUG_NO_K0 = 8192             # IPMZ_DEBUG_NO_K0: the whole matrix assembled into K every step
SOLVE_CASE = (64, 24, 8, 6)


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


@pytest.fixture(autouse=True)
def clear_debug():
    yield
    I.debug_inject(0)


def _data(q):
    return I.Data(q["Q"], q["c"], q["lx"], q["ux"], q["A"], q["lA"], q["uA"], q["C"], q["d"])


def _batch(ctx, n, m, p, B, seeds, kernel=None, **kw):
    bt = I.Batch(n, m, p, B, ctx, **kw)
    for i, s in enumerate(seeds):
        bt.load_one(i, _data(nc.qp(n, m, p, s)))
    bt.initialize()
    if kernel is not None:
        bt.set_factor_kernel(kernel)
    return bt


def _snap(bt):
    """(the three state blocks, the scalar blocks) of every QP, on the host."""
    return [bt.state_tensor(w).cpu().numpy().copy() for w in range(3)], bt.batch_scalars()


def _same(a, b):
    """bitwise (NaN-safe)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _twins(B):
    return [SEED0 + i // 2 for i in range(B)]


def _trajectory(A, S, flags_s, reset=True):
    """Steps both until A shows every QP converged, then TAIL more; returns (snapshots of A, of S, c)."""
    B = A.batch
    init = [A.state(i) for i in range(B)]
    snaps_a, snaps_s = [_snap(A)], [_snap(S)]
    c = np.zeros(B, dtype=np.int64)  # 0: not yet
    t = 0
    while t < T_MAX:
        A.step(0)
        S.step(flags_s)
        t += 1
        if reset and t == RESET_AFTER:
            for bt in (A, S):
                for i in range(1, B, 2):
                    bt.set_state(i, init[i])
        snaps_a.append(_snap(A))
        snaps_s.append(_snap(S))
        conv = snaps_a[-1][1][:, I.SC["converged"]] != 0.0
        c[(c == 0) & conv] = t
        if (c > 0).all() and t >= c.max() + TAIL:
            break
    return snaps_a, snaps_s, c


def _check_trajectory(snaps_a, snaps_s, c, what):
    T, B = len(snaps_a) - 1, len(c)
    assert (c > 0).all(), f"{what}: not every QP converged in {T} steps: c = {c}"
    assert c.max() - c.min() >= 3, f"{what}: no stagger, c = {c}"
    assert (T - c >= 3).any(), f"{what}: no QP was skipped 3 times, c = {c}, T = {T}"
    assert c.min() > RESET_AFTER, f"{what}: a QP converged before the odd slots went back: c = {c}"
    print(f"{what}: T = {T}, c = {c.tolist()}", flush=True)
    for q in range(B):
        cq = int(c[q])
        for t in range(T + 1):
            (va, sa), (vs, ss) = snaps_a[t], snaps_s[t]
            if t <= cq:
                for w in range(3 if t else 1):  # (no step has written the direction blocks yet at t = 0)
                    assert _same(vs[w][q], va[w][q]), f"{what}: QP {q} step {t} state {w} differs from flag-off"
                assert _same(ss[q, :14], sa[q, :14]), f"{what}: QP {q} step {t} scalars differ from flag-off"
            else:
                vc, sc = snaps_s[cq]
                for w in range(3):
                    assert _same(vs[w][q], vc[w][q]), f"{what}: QP {q} step {t} state {w} moved after convergence"
                assert _same(ss[q], sc[q]), f"{what}: QP {q} step {t} scalars moved after convergence"
                assert _same(vs[0][q], va[0][q]), f"{what}: QP {q} step {t} iterate differs from flag-off"
            # the steps before which A's flag was 0 (those from the solver's first skip step on)
            assert ss[q, I.SC["steps"]] == min(t, cq), f"{what}: QP {q} step {t}: steps {ss[q, I.SC['steps']]}"
            assert sa[q, I.SC["steps"]] == 0.0, f"{what}: a flag-off step touched IPMZ_SC_STEPS"


# (n, m, p, B, Batch keywords, factor kernel, debug mask)
CASES = [
    ("N64-left", 40, 16, 8, 6, {}, None, 0),
    ("N96-ws", 64, 24, 8, 6, {}, None, 0),
    ("N96-one", 64, 24, 8, 6, {}, I.Batch.FACTOR_ONE, 0),
    ("N96-left", 64, 24, 8, 6, {}, I.Batch.FACTOR_LEFT, 0),
    ("N96-pair", 64, 24, 8, 6, {}, I.Batch.FACTOR_PAIR, 0),
    ("N384", 256, 96, 32, 4, {}, None, 0),
    ("N1024", 768, 192, 64, 2, {}, None, 0),
    ("box", 64, 0, 0, 4, {}, None, 0),
    ("naive", 48, 16, 8, 6, dict(inequality_handling=I.INEQ_NAIVE_SLACKS), None, 0),
    ("penalty", 64, 24, 8, 6, dict(equality_handling=I.EQ_PENALTY), None, 0),
    ("eqnone", 64, 24, 8, 6, dict(equality_handling=I.EQ_NONE), None, 0),
    ("separate", 64, 24, 8, 6, {}, None, DEBUG_NO_FUSED_SOLVES),
    ("no-k0", 64, 24, 8, 6, {}, None, DEBUG_NO_K0),
    # more QPs than CUs: the 8-wave forms of k_fused_solves, and (separate) of trsv_small_kernel
    ("N64-w8", 40, 16, 8, None, {}, None, 0),
    ("N64-w8-separate", 40, 16, 8, None, {}, None, DEBUG_NO_FUSED_SOLVES),
]


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bitwise_trajectory(ctx, case):
    name, n, m, p, B, kw, kernel, mask = case
    if B is None:
        B = torch.cuda.get_device_properties(0).multi_processor_count + 2
    try:
        I.debug_inject(mask)
        A = _batch(ctx, n, m, p, B, _twins(B), kernel, **kw)
        S = _batch(ctx, n, m, p, B, _twins(B), kernel, **kw)
        assert S.can_skip_converged()
        snaps_a, snaps_s, c = _trajectory(A, S, I.STEP_SKIP_CONVERGED)
        _check_trajectory(snaps_a, snaps_s, c, name)
        assert not S.last_step_graph()
    finally:
        I.debug_inject(0)
    A.close()
    S.close()


# 2 ---------------------------------------------------------------------------
def test_graph_replay_equals_eager_skip_steps(ctx):
    n, m, p, B = SOLVE_CASE
    E = _batch(ctx, n, m, p, B, _twins(B))
    G = _batch(ctx, n, m, p, B, _twins(B))
    # (E in A's place: its flag-off role is only to say when to stop, and a skip solver's flags are A's)
    snaps_e, snaps_g, c = _trajectory(E, G, I.STEP_SKIP_CONVERGED | I.STEP_GRAPH, reset=True)
    assert G.last_step_graph() == 1
    S = _batch(ctx, n, m, p, B, _twins(B))
    init = [S.state(i) for i in range(B)]
    for t in range(1, len(snaps_g)):
        S.step(I.STEP_SKIP_CONVERGED)
        if t == RESET_AFTER:
            for i in range(1, B, 2):
                S.set_state(i, init[i])
        (vs, ss), (vg, sg) = _snap(S), snaps_g[t]
        for w in range(3):
            assert _same(vs[w], vg[w]), f"step {t} state {w}: graph replay differs from the eager skip step"
        assert _same(ss, sg), f"step {t}: scalars of the graph replay differ"
    assert (c > 0).all() and c.max() - c.min() >= 3
    for b in (E, G, S):
        b.close()


# 3 ---------------------------------------------------------------------------
def _plain_counts(ctx):
    """c_q of SOLVE_CASE with a QP of its own per slot, from flag-off steps taken one at a time."""
    n, m, p, B = SOLVE_CASE
    A = _batch(ctx, n, m, p, B, [SEED0 + i for i in range(B)])
    c = np.zeros(B, dtype=np.int64)
    for t in range(1, T_MAX):
        A.step(0)
        conv = A.batch_scalars()[:, I.SC["converged"]] != 0.0
        c[(c == 0) & conv] = t
        if (c > 0).all():
            break
    assert (c > 0).all()
    A.close()
    return c


def test_solve_all(ctx):
    n, m, p, B = SOLVE_CASE
    seeds = [SEED0 + i for i in range(B)]
    c = _plain_counts(ctx)
    P = _batch(ctx, n, m, p, B, seeds)
    its, nconv = P.solve_all()
    assert (its, nconv) == (int(c.max()), B)
    vp, sp = _snap(P)
    print(f"solve_all: c = {c.tolist()}, plain iterations {its}", flush=True)
    for k in (1, 4):
        S = _batch(ctx, n, m, p, B, seeds)
        its_k, nconv_k = S.solve_all(skip_converged=True, check_every=k)
        vs, ss = _snap(S)
        assert _same(vs[0], vp[0]), f"check_every {k}: the iterates differ from solve_all()'s"
        assert np.array_equal(S.step_counts(), c), f"check_every {k}: {S.step_counts()} vs {c}"
        assert its_k == -(-int(c.max()) // k) * k and nconv_k == B, (k, its_k, nconv_k)
        # max_iter in the middle of a round of k steps
        S2 = _batch(ctx, n, m, p, B, seeds)
        cap = int(c.max()) - 1
        its_c, nconv_c = S2.solve_all(max_iter=cap, skip_converged=True, check_every=k)
        assert its_c == cap and nconv_c == int((c <= cap).sum()), (k, cap, its_c, nconv_c)
        assert np.array_equal(S2.step_counts(), np.minimum(c, cap))
        S.close()
        S2.close()
    # ipmz_batch_solve_ex(flags 0, check 1) is ipmz_batch_solve
    X = _batch(ctx, n, m, p, B, seeds)
    it, nc_ = ctypes.c_int(-1), ctypes.c_int(-1)
    assert I.lib.ipmz_batch_solve_ex(X.h, 100, 0, 1, ctypes.byref(it), ctypes.byref(nc_)) == 0
    vx, sx = _snap(X)
    assert (it.value, nc_.value) == (its, nconv)
    for w in range(3):
        assert _same(vx[w], vp[w])
    assert _same(sx, sp)
    # ... and with the graph alone
    Gs = _batch(ctx, n, m, p, B, seeds)
    assert Gs.solve_all(graph=True, check_every=2) == (-(-its // 2) * 2, B)
    assert Gs.last_step_graph() == 1 and _same(_snap(Gs)[0][0], vp[0])
    # bad arguments
    for args in ((100, 0, 0), (100, 1, 1), (100, 8, 1), (-1, 0, 1)):
        assert I.lib.ipmz_batch_solve_ex(X.h, args[0], args[1], args[2], None, None) == -1, args
    for b in (P, X, Gs):
        b.close()


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("ldlt", "eqnone"))
def test_nothing_moves_after_convergence_and_the_backward_factor_is_whole(ctx, eq_none):
    n, m, p, B = SOLVE_CASE
    kw = dict(equality_handling=I.EQ_NONE) if eq_none else {}
    seeds = [SEED0 + i for i in range(B)]
    A = _batch(ctx, n, m, p, B, seeds, **kw)
    S = _batch(ctx, n, m, p, B, seeds, **kw)
    assert A.solve_all()[1] == B and S.solve_all(skip_converged=True, check_every=4)[1] == B
    before = _snap(S)
    res = S.state_tensor(3).cpu().numpy().copy()
    for _ in range(5):
        S.step(I.STEP_SKIP_CONVERGED)
    after = _snap(S)
    for w in range(3):
        assert _same(before[0][w], after[0][w]), f"state {w} moved"
    assert _same(before[1], after[1]), "a scalar block moved"
    assert _same(res, S.state_tensor(3).cpu().numpy()), "the residuals moved"
    assert _same(after[0][0], _snap(A)[0][0])
    # the calls that reuse the step's factor factor every QP, converged or not
    L, ld, nrhs = S.state_len, nc.even(S.state_len), 3
    G = np.zeros((B, nrhs, ld))
    G[:, :, :L] = nc.rows(L, B)[:, :nrhs]
    outs = []
    for bt in (A, S):
        g = torch.from_numpy(G).cuda()
        bt.newton_adjoint_all(g.data_ptr(), g.data_ptr(), nrhs, ld, nrhs * ld, ld, nrhs * ld)
        torch.cuda.synchronize()
        outs.append(g.cpu().numpy())
    assert _same(outs[0], outs[1]), "newton_adjoint_all after skip steps differs from the flag-off solver's"
    assert np.isfinite(outs[1]).all()
    N, ldn = S.N, nc.even(S.N)
    R = np.zeros((B, nrhs, ldn))
    R[:, :, :N] = nc.rows(N, B)[:, :nrhs]
    outs = []
    for bt in (A, S):
        r = torch.from_numpy(R).cuda()
        (bt.kkt_solve_all_bk if eq_none else bt.kkt_solve_all)(r.data_ptr(), nrhs, ldn, nrhs * ldn)
        torch.cuda.synchronize()
        outs.append(r.cpu().numpy())
    assert _same(outs[0], outs[1]), "kkt_solve_all after skip steps differs from the flag-off solver's"
    A.close()
    S.close()


# 5 ---------------------------------------------------------------------------
def test_layer(ctx):
    import data_vjp_cases as dc
    from ipmz_amd import layer
    n, m, p = nc.SHAPES[0]
    B = 3
    qs = [nc.qp(n, m, p, SEED0 + i) for i in range(B)]
    stack = {k: np.stack([q[dc.KEYS[k]] for q in qs]) for k in dc.present(n, m, p)}
    G = torch.from_numpy(np.random.default_rng(77).standard_normal((B, n))).cuda()
    got = []
    for kw in ({}, dict(skip_converged=True, check_every=4)):
        bt = I.Batch(n, m, p, B, ctx)
        leaves = {k: torch.from_numpy(np.array(a)).cuda().requires_grad_(True) for k, a in stack.items()}
        torch.cuda.synchronize()
        x = layer.solve_qp(bt, **leaves, **kw)
        (G * x).sum().backward()
        torch.cuda.synchronize()
        got.append((x.detach().cpu().numpy(), {k: t.grad.cpu().numpy() for k, t in leaves.items()}))
        if kw:
            assert bt.step_counts().min() > 0
        bt.close()
    assert _same(got[0][0], got[1][0]), "x differs"
    assert set(got[0][1]) == set(stack)
    for k in stack:
        assert _same(got[0][1][k], got[1][1][k]), f"the gradient of {k} differs"
    # a solver that cannot skip: named
    one = I.Batch(n, m, p, 1, ctx)
    with pytest.raises(I.IpmzError, match="can_skip_converged"):
        layer.solve_qp(one, **{k: torch.from_numpy(a[:1].copy()).cuda() for k, a in stack.items()}, skip_converged=True)
    one.close()


# 6 ---------------------------------------------------------------------------
def test_guards(ctx):
    n, m, p = 64, 24, 8
    o = I.Optimizer(n, m, p, ctx)
    o.generate(SEED0)
    b1 = I.Batch(n, m, p, 1, ctx)
    b1.generate(SEED0)
    big = I.Batch(800, 200, 64, 2, ctx)  # N = 1064: refused before the check for a load
    ctx128 = I.Context(0, nbi=128)
    b128 = I.Batch(n, m, p, 3, ctx128)
    b128.generate(SEED0)
    for s in (o, b1, big, b128):
        assert not s.can_skip_converged()
        with pytest.raises(I.IpmzError, match="invalid argument"):
            s.step(I.STEP_SKIP_CONVERGED)
    for s in (b1, big, b128):
        with pytest.raises(I.IpmzError, match="invalid argument"):
            s.solve_all(skip_converged=True)
    ok = I.Batch(n, m, p, 3, ctx)
    assert ok.can_skip_converged()
    with pytest.raises(I.IpmzError, match="bad state"):
        ok.step(I.STEP_SKIP_CONVERGED)
    with pytest.raises(I.IpmzError, match="bad state"):
        ok.solve_all(skip_converged=True)
    with pytest.raises(I.IpmzError, match="invalid argument"):
        ok.step(I.STEP_SKIP_CONVERGED | I.STEP_RESTART_IF_CONVERGED)
    ok.generate(SEED0)
    with pytest.raises(I.IpmzError, match="invalid argument"):
        ok.step(I.STEP_SKIP_CONVERGED | I.STEP_RESTART_IF_CONVERGED)
    ok.step(I.STEP_SKIP_CONVERGED)
    assert ok.step_counts().tolist() == [1, 1, 1]
    ok.generate(SEED0)  # the count restarts with the scalar block
    assert ok.step_counts().tolist() == [0, 0, 0]
    assert I.lib.ipmz_batch_can_skip_converged(None) == 0
    for s in (o, b1, big, b128, ok):
        s.close()
    ctx128.close()
