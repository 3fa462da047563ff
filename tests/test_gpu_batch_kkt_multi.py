"""Batched multi-right-hand-side KKT solve (ipmz_batch_get_kkt /
ipmz_batch_kkt_solve: Batch.kkt_of, Batch.kkt_solve_all) on the device, through
the public ABI only.

Three paths serve a call (csrc/qp.cpp batch_multi_impl):
  looped   few rows: one launch of the step's single-vector batched solve per row;
  fused    one launch per batch, a QP's 16 right-hand sides resident in LDS
           (trsm.hip trsm_fused_kernel; N <= 832 with nbi 64, <= 768 with 128);
  panels   the panel chain of the single-system solve with the QP on a grid
           dimension (larger N, or a forced panel width).
The debug bits reach them: MULTI_BLOCKED skips the loop for nrhs >= 2,
MULTI_W128 / MULTI_W512 force the panel chain at that width.

Reference (tests/batch_kkt_cases.py): for QP i, K_i = sym(batch.kkt_of(i)),
X_ref = oracle.solve_ldlt(*oracle.ldlt(K_i), b) per row; bound |x - x_ref|_inf
< 1e-12 max(1, |x_ref|_inf) per row.  tests/test_oracle_batch_kkt_multi.py
checks on the CPU that two CPU solves of these matrices agree to 1e-13 in the
same measure, so 1e-12 is the summation order and the device factor's
reciprocals, not the reference.  Every case prints its worst figure before
asserting it.
"""
import numpy as np
import pytest

import batch_kkt_cases as kc
import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

DISPATCH = (("default", 0), ("w128", kc.MULTI_W128), ("w512", kc.MULTI_W512))


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


@pytest.fixture(scope="module")
def ctx128():
    """A context of its own with nbi = 128, set before any Batch is sized for it."""
    c = I.Context(0, nbi=128)
    yield c
    c.close()


def _batch(c, ctx, **kw):
    n, m, p, B, seed0 = c
    bt = I.Batch(n, m, p, B, ctx, **kw)
    bt.generate(seed0)
    return bt


def _solve(bt, rows, bits=0, ldb=None, sB=None, fill=None):
    """kkt_solve_all on a copy of rows (B, nrhs, N) laid out with (ldb, sB); returns
    the whole device buffer as a (B, sB) array.  fill: what the padding holds."""
    B, nrhs, N = rows.shape
    ldb = ldb or kc.ldb_of(N)
    sB = sB if sB is not None else nrhs * ldb
    host = np.full((B, max(sB, 1)), 0.0 if fill is None else fill)
    for q in range(B):
        for r in range(nrhs):
            host[q, r * ldb:r * ldb + N] = rows[q, r]
    t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    I.debug_inject(bits)
    try:
        assert bt.kkt_solve_all(t.data_ptr(), nrhs, ldb, sB) == 0
    finally:
        I.debug_inject(0)
    return t.cpu().numpy(), host


def _rows(buf, nrhs, N, ldb):
    return np.stack([[buf[q, r * ldb:r * ldb + N] for r in range(nrhs)] for q in range(buf.shape[0])])


def _x(bt, rows, bits=0):
    B, nrhs, N = rows.shape
    buf, _ = _solve(bt, rows, bits)
    return _rows(buf, nrhs, N, kc.ldb_of(N))


# 1 ---------------------------------------------------------------------------
def test_kkt_of_equals_the_single_solvers(ctx):
    c = kc.SHAPES[0]
    n, m, p, B, seed0 = c
    bt = _batch(c, ctx)
    singles = []
    for i in range(B):
        g = I.Optimizer(n, m, p, ctx)
        g.generate(seed0 + i)
        singles.append(g)
    for i, g in enumerate(singles):
        assert np.array_equal(bt.state(i), g.vars()), i
        assert np.array_equal(bt.kkt_of(i), g.kkt()), i
    for _ in range(2):
        bt.step()
        for g in singles:
            g.step()
    # A batch and a single solver step through different factor and solve
    # kernels, so after two steps their iterates agree to rounding, not bitwise
    # (the figure is printed): the single solver is given the batch's iterate,
    # and the two assemblies of that iterate are compared bitwise.
    for i, g in enumerate(singles):
        v = bt.state(i)
        print(f"QP {i}: |v_batch - v_single|_inf after two steps {np.abs(v - g.vars()).max():.3e}", flush=True)
        assert np.allclose(v, g.vars(), rtol=1e-9, atol=1e-9), i
        g.set_vars(v)
        assert np.array_equal(bt.kkt_of(i), g.kkt()), i
    assert np.array_equal(bt.kkt_of(0), bt.kkt())  # ipmz_qp_get_kkt keeps addressing QP 0
    for bad in (-1, B):
        with pytest.raises(I.IpmzError):
            bt.kkt_of(bad)


# 2 ---------------------------------------------------------------------------
def _vs_reference(bt, label):
    """Every dispatch x right-hand-side count at the current iterate."""
    N, B = bt.N, bt.batch
    rows = kc.rhs(N, B)
    X_ref = np.stack([kc.reference(bt.kkt_of(q), rows[q]) for q in range(B)])
    worst, got = {}, {}
    for dname, dbits in DISPATCH:
        for nrhs in kc.RHS_COUNTS:
            for blocked in ((True, False) if nrhs >= 16 else (True,)):
                bits = dbits | (kc.MULTI_BLOCKED if blocked else 0)
                X = _x(bt, np.array(rows[:, :nrhs]), bits)
                key = (dname, nrhs, blocked)
                worst[key] = kc.row_err(X, X_ref[:, :nrhs])
                got[key] = X
    # default vs forced panels: the same bound between them
    cross = {}
    for dname in ("w128", "w512"):
        for nrhs in kc.RHS_COUNTS:
            a, b = got[("default", nrhs, True)], got[(dname, nrhs, True)]
            cross[(dname, nrhs)] = kc.row_err(a, b)
    print(f"{label}: worst vs reference {max(worst.values()):.3e} at {max(worst, key=worst.get)}; "
          f"default vs panels {max(cross.values()):.3e} at {max(cross, key=cross.get)} (bound {kc.TOL:.1e})", flush=True)
    for key, e in worst.items():
        assert e < kc.TOL, (label, key, e)
    for key, e in cross.items():
        assert e < kc.TOL, (label, "default vs", key, e)


@pytest.mark.parametrize("c", kc.SHAPES, ids=kc.case_id)
def test_vs_reference(ctx, c):
    bt = _batch(c, ctx)
    _vs_reference(bt, f"N{bt.N} initial")
    bt.step()
    bt.step()
    _vs_reference(bt, f"N{bt.N} after two steps")


@pytest.mark.parametrize("c", [c for c in kc.SHAPES if kc.order(c) in kc.NBI128_ORDERS], ids=kc.case_id)
def test_vs_reference_nbi128(ctx128, c):
    assert ctx128.blocking(kc.order(c))[1] == 128
    bt = _batch(c, ctx128)
    _vs_reference(bt, f"N{bt.N} nbi128 initial")
    bt.step()
    bt.step()
    _vs_reference(bt, f"N{bt.N} nbi128 after two steps")


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [kc.SHAPES[2], kc.SHAPES[5]], ids=kc.case_id)
def test_looped_rows_are_single_solves(ctx, c):
    bt = _batch(c, ctx)
    rows = np.array(kc.rhs(bt.N, bt.batch)[:, :3])
    X3 = _x(bt, rows)
    for r in range(3):
        assert np.array_equal(_x(bt, rows[:, r:r + 1])[:, 0], X3[:, r]), r


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["looped", "fused", "w128", "default-panels"])
def test_padding_keeps_its_bits(ctx, path):
    c = kc.SHAPES[5] if path == "default-panels" else kc.SHAPES[2]
    bt = _batch(c, ctx)
    N, B = bt.N, bt.batch
    nrhs = 3 if path == "looped" else 17
    bits = {"looped": 0, "fused": kc.MULTI_BLOCKED, "w128": kc.MULTI_BLOCKED | kc.MULTI_W128,
            "default-panels": kc.MULTI_BLOCKED}[path]
    ldb = N + 6 + (N & 1)  # even
    sB = nrhs * ldb + 10
    sentinel = np.frombuffer(np.uint64(0x7ff8dead0000beef).tobytes(), dtype=np.float64)[0]  # a NaN with a payload
    rows = np.array(kc.rhs(N, B)[:, :nrhs])
    out, before = _solve(bt, rows, bits, ldb=ldb, sB=sB, fill=sentinel)
    pad = np.ones(sB, dtype=bool)
    for r in range(nrhs):
        pad[r * ldb:r * ldb + N] = False
    assert np.array_equal(out.view(np.uint64)[:, pad], before.view(np.uint64)[:, pad])
    X = _rows(out, nrhs, N, ldb)
    assert np.array_equal(X, _x(bt, rows, bits))  # and the layout does not change the rows


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, kc.MULTI_BLOCKED, kc.MULTI_BLOCKED | kc.MULTI_W128],
                         ids=["looped-or-default", "blocked", "w128"])
def test_rows_and_qps_are_independent(ctx, bits):
    c = kc.SHAPES[2]
    n, m, p, B, seed0 = c
    bt = _batch(c, ctx)
    nrhs = 3 if bits == 0 else 17
    rows = np.array(kc.rhs(bt.N, B)[:, :nrhs])
    full = _x(bt, rows, bits)
    z = rows.copy()
    z[1] = 0.0      # a QP whose rows are all zero
    z[0, 1] = 0.0   # a zero row inside a QP
    X = _x(bt, z, bits)
    assert not X[1].any() and not X[0, 1].any()
    assert np.array_equal(X[2], full[2]) and np.array_equal(X[0, 0], full[0, 0]) and np.array_equal(X[0, 2:], full[0, 2:])
    # QPs 0 and 1 of this 3-batch against the same QPs of a 2-batch
    two = _batch((n, m, p, 2, seed0), ctx)
    assert np.array_equal(_x(two, rows[:2], bits), full[:2])


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [kc.SHAPES[2], kc.SHAPES[4]], ids=kc.case_id)
def test_deterministic(ctx, c):
    bt = _batch(c, ctx)
    rows = np.array(kc.rhs(bt.N, bt.batch))
    for _, dbits in DISPATCH:
        a = _x(bt, rows, dbits | kc.MULTI_BLOCKED)
        b = _x(bt, rows, dbits | kc.MULTI_BLOCKED)
        assert np.array_equal(a, b), dbits


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("c,flags,steps", [(kc.SHAPES[0], 0, 3), (kc.SHAPES[0], I.STEP_GRAPH, 3), (kc.SHAPES[5], 0, 2)],
                         ids=["N72-eager", "N72-graph", "N1040-eager"])
def test_steps_unchanged(ctx, c, flags, steps):
    a, b = _batch(c, ctx), _batch(c, ctx)
    rows = np.array(kc.rhs(a.N, a.batch)[:, :17])
    for it in range(steps):
        _x(a, rows, kc.MULTI_BLOCKED if it % 2 == 0 else 0)
        a.step(flags)
        b.step(flags)
        if flags & I.STEP_GRAPH:
            assert a.last_step_graph() and b.last_step_graph(), it
        assert np.array_equal(a.batch_scalars(), b.batch_scalars()), it
        for i in range(a.batch):
            for which in range(4):
                assert np.array_equal(a.state(i, which), b.state(i, which)), (it, i, which)


# 8 ---------------------------------------------------------------------------
def test_arguments_and_states(ctx):
    c = kc.SHAPES[0]
    n, m, p, B, seed0 = c
    bt = _batch(c, ctx)
    N = bt.N
    t = torch.zeros(B * 4 * (N + 2) + 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = t.data_ptr()
    assert bt.kkt_solve_all(ptr, 0, N, 0) == 0  # nrhs == 0: assembles, factors, returns the info word
    for nrhs, ldb, sB, off in ((-1, N, 4 * N, 0), (2, N - 2, 2 * N, 0), (2, N + 1, 2 * (N + 1), 0), (2, N, 2 * N - 2, 0),
                               (2, N, 2 * N + 1, 0), (2, N, 2 * N, 8)):
        with pytest.raises(I.IpmzError):
            bt.kkt_solve_all(ptr + off, nrhs, ldb, sB)
    with pytest.raises(I.IpmzError, match="batch"):
        bt.kkt_solve(ptr, 2, N)
    none = I.Batch(n, m, p, 2, ctx, equality_handling=I.EQ_NONE)
    none.generate(seed0)
    with pytest.raises(I.IpmzError, match="Bunch-Kaufman"):
        none.kkt_solve_all(ptr, 2, N, 2 * N)
    # a load leaves the batch uninitialized
    q = oracle.gen_qp(n, m, p, seed0)
    bt.load_one(0, I.Data(q["Q"], q["c"], q["lx"], q["ux"], q["A"], q["lA"], q["uA"], q["C"], q["d"]))
    with pytest.raises(I.IpmzError, match="bad state"):
        bt.kkt_solve_all(ptr, 2, N, 2 * N)
    bt.initialize()
    assert bt.kkt_solve_all(ptr, 2, N, 2 * N) == 0


def test_batch_of_one_is_the_single_solve(ctx):
    n, m, p, _, seed0 = kc.SHAPES[0]
    one = I.Batch(n, m, p, 1, ctx)
    one.generate(seed0)
    g = I.Optimizer(n, m, p, ctx)
    g.generate(seed0)
    N = one.N
    rows = np.array(kc.rhs(N, 1)[0, :17])
    ta, tb = torch.from_numpy(rows.copy()).cuda(), torch.from_numpy(rows.copy()).cuda()
    torch.cuda.synchronize()
    assert one.kkt_solve_all(ta.data_ptr(), 17, N, 12345) == 0  # (sB ignored)
    assert g.kkt_solve(tb.data_ptr(), 17, N) == 0
    assert torch.equal(ta, tb)
    assert kc.row_err(ta.cpu().numpy(), kc.reference(g.kkt(), rows)) < kc.TOL
