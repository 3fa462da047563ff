"""Batched multi-right-hand-side Bunch-Kaufman solve on caller-owned storage
(ipmz_bk_factor_batch, ipmz_bk_prepare_solve_batch, ipmz_bk_solve_multi_batch)
and for EqualityHandling::None batches of QPs (ipmz_batch_kkt_solve_bk),
against the CPU oracle's reference-order solve, row by row.  Run on an MI355X:
pytest -m gpu.

Cases, reference and tolerance: tests/bk_batch_cases.py (its facts are checked
without a GPU in tests/test_oracle_bk_batch_cases.py).  Three routes serve a
row count from the crossover on: the one-launch solve where a system's slab
fits the LDS (the default up to N = 832), the panel chain (MULTI_BLOCKED alone
changes nothing there; with MULTI_W128 the panel chain runs at every order,
128 columns wide), and below the crossover one launch of the step's kernel
per row, which MULTI_BLOCKED turns into the blocked routes for nrhs >= 2.
Except in the factor test the factors uploaded are the oracle's: the device
factor is bitwise that one (test_factor_batch), the rest is about the solve.
"""
import numpy as np
import pytest

import bk_batch_cases as C
import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

ROUTES = (("default", 0), ("blocked", C.MULTI_BLOCKED), ("w128", C.MULTI_BLOCKED | C.MULTI_W128))
FILL = -7.25  # sentinel of the padding


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


class DevBatch:
    """Matrices (or factors) of one order on the device, system q at q * sA, pivots at q * sP."""

    def __init__(self, ctx, mats, pivs=None, ld=None, sA=None, sP=None):
        self.ctx, self.batch, self.N = ctx, len(mats), mats[0].shape[0]
        N = self.N
        self.ld = ld or N
        self.sA = sA or N * self.ld + ((N * self.ld) & 1)
        self.sP = sP or N
        host = np.zeros(self.batch * self.sA)
        hp = np.zeros(self.batch * self.sP, dtype=np.int32)
        for q, M in enumerate(mats):
            host[q * self.sA:q * self.sA + N * self.ld].reshape(N, self.ld)[:, :N] = M
            if pivs is not None:
                hp[q * self.sP:q * self.sP + N] = pivs[q]
        self.A = torch.from_numpy(host).cuda()
        self.piv = torch.from_numpy(hp).cuda()
        self.ws = None
        torch.cuda.synchronize()

    def args(self):
        return (self.N, self.batch, self.A.data_ptr(), self.ld, self.sA, self.piv.data_ptr(), self.sP)

    def factor(self):
        return self.ctx.bk_factor_batch(*self.args())

    def lower(self, q):
        a = self.A.cpu().numpy()[q * self.sA:q * self.sA + self.N * self.ld].reshape(self.N, self.ld)
        return np.tril(a[:, :self.N])

    def pivots(self, q):
        return self.piv.cpu().numpy()[q * self.sP:q * self.sP + self.N]

    def prepare(self):
        self.wsb = self.ctx.bk_batch_solve_workspace_bytes(self.N, self.batch)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        self.ctx.bk_prepare_solve_batch(*self.args(), self.ws.data_ptr(), self.wsb)
        self.ctx.sync()
        return self

    def solve(self, rows, bits=0, ldb=None, sB=None, fill=0.0):
        """bk_solve_multi_batch on a copy of rows (batch, nrhs, N) laid out with (ldb, sB);
        returns the whole device buffer (batch, sB) and what it held before."""
        B, nrhs, N = rows.shape
        ldb = ldb or C.ldb_of(N)
        sB = sB if sB is not None else nrhs * ldb
        host = np.full((B, max(sB, 1)), fill)
        for q in range(B):
            for r in range(nrhs):
                host[q, r * ldb:r * ldb + N] = rows[q, r]
        t = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        I.debug_inject(bits)
        try:
            self.ctx.bk_solve_multi_batch(*self.args(), self.ws.data_ptr(), t.data_ptr(), ldb, sB, nrhs)
            self.ctx.sync()
        finally:
            I.debug_inject(0)
        return t.cpu().numpy(), host

    def x(self, rows, bits=0):
        B, nrhs, N = rows.shape
        return _rows(self.solve(rows, bits)[0], nrhs, N, C.ldb_of(N))

    def single(self, q, b):
        """ipmz_bk_solve of one vector with system q's factor."""
        t = torch.from_numpy(np.array(b)).cuda()
        torch.cuda.synchronize()
        self.ctx.bk_solve(self.N, self.A.data_ptr() + 8 * q * self.sA, self.ld, self.piv.data_ptr() + 4 * q * self.sP,
                          t.data_ptr())
        self.ctx.sync()
        return t.cpu().numpy()


def _rows(buf, nrhs, N, ldb):
    return np.stack([[buf[q, r * ldb:r * ldb + N] for r in range(nrhs)] for q in range(buf.shape[0])])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


_prepared = {}


def _factors(ctx, keys, **kw):
    """The oracle's factors of the batch on the device, prepared (one per batch and layout, shared)."""
    tag = (tuple(keys), tuple(sorted(kw.items())))
    if tag not in _prepared:
        sys = [C.system(k) for k in keys]
        _prepared[tag] = DevBatch(ctx, [s[1] for s in sys], [s[2] for s in sys], **kw).prepare()
    return _prepared[tag]


def _rhs(keys, nrhs):
    return np.array(C.rhs(C.order(keys[0]), len(keys))[:, :nrhs])


ALL = list(C.BATCHES.items()) + [("singular", C.SINGULAR)]


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["packed", "strided"])
@pytest.mark.parametrize("name,keys", ALL, ids=[n for n, _ in ALL])
def test_factor_batch(ctx, name, keys, strided):
    sys = [C.system(k) for k in keys]
    N = C.order(keys[0])
    ld = N + 10 if strided else N
    kw = dict(ld=ld, sA=N * ld + 6, sP=N + 3) if strided else {}
    d = DevBatch(ctx, [s[0] for s in sys], **kw)
    rc, info = d.factor()
    want = [s[3] + 1 if s[3] else 0 for s in sys]  # 1 + the oracle's 0-based word, as ipmz_bk_factor
    assert list(info) == want, name
    assert rc == (min(i for i in want if i) if any(want) else 0)
    if name == "singular":
        assert [s[3] for s in sys] == C.SINGULAR_INFO
        assert list(info) == C.SINGULAR_DEVICE_INFO and rc == 162
    for q, (K, Fo, po, _) in enumerate(sys):
        assert np.array_equal(_bits(d.lower(q)), _bits(np.tril(Fo))), (name, q)
        assert np.array_equal(d.pivots(q), po), (name, q)
        one = DevBatch(ctx, [K])
        ctx.bk_factor(N, one.A.data_ptr(), one.ld, one.piv.data_ptr(), algo=I.Context.BK_WORKGROUP)
        ctx.sync()
        assert np.array_equal(_bits(d.lower(q)), _bits(one.lower(0))), (name, q)
        assert np.array_equal(d.pivots(q), one.pivots(0)), (name, q)


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("route,bits", ROUTES, ids=[r for r, _ in ROUTES])
@pytest.mark.parametrize("name", list(C.BATCHES))
def test_vs_oracle(ctx, name, route, bits):
    keys = C.BATCHES[name]
    f = _factors(ctx, keys)
    X_ref = C.batch_reference(keys)
    for nrhs in C.RHS_COUNTS:
        X = f.x(_rhs(keys, nrhs), bits)
        err = C.row_err(X, X_ref[:, :nrhs])
        print(f"{name} {route} nrhs={nrhs}: err {err:.3e}")
        assert err < C.TOL, (name, route, nrhs, err)


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["indef72", "indef321", "kktz832", "indef1040"])
def test_looped_rows(ctx, name):
    keys = C.BATCHES[name]
    f = _factors(ctx, keys)
    N, x = C.order(keys[0]), C.crossover()
    for nrhs in sorted({3, x - 1} - {0}):
        assert nrhs < x
        rows = _rhs(keys, nrhs)
        X = f.x(rows)
        ones = np.concatenate([f.x(rows[:, r:r + 1]) for r in range(nrhs)], axis=1)
        assert np.array_equal(_bits(X), _bits(ones)), (name, nrhs)  # k rows are k calls with one row
        assert C.row_err(X, C.batch_reference(keys)[:, :nrhs]) < C.TOL
        if N < C.BK_GRID_MIN:  # ipmz_bk_solve is the one-workgroup kernel on F there
            single = np.stack([[f.single(q, rows[q, r]) for r in range(nrhs)] for q in range(len(keys))])
            assert np.array_equal(_bits(X), _bits(single)), (name, nrhs)


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("route,bits", ROUTES, ids=[r for r, _ in ROUTES])
@pytest.mark.parametrize("name", ["indef192", "indef321", "kktz832", "indef834"])
def test_rows_and_systems_are_independent_and_deterministic(ctx, name, route, bits):
    keys = C.BATCHES[name]
    f = _factors(ctx, keys)
    X17 = f.x(_rhs(keys, 17), bits)
    assert np.array_equal(_bits(X17), _bits(f.x(_rhs(keys, 17), bits)))       # a second identical call
    assert np.array_equal(_bits(X17), _bits(f.x(_rhs(keys, 33), bits)[:, :17]))  # among 33 rows
    for q, k in enumerate(keys):                                                  # the system alone
        alone = _factors(ctx, [k])
        assert np.array_equal(_bits(X17[q]), _bits(alone.x(_rhs(keys, 17)[q:q + 1], bits)[0])), (name, route, q)


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,nrhs,bits", [("indef72", 3, 0), ("indef72", 17, 0), ("indef72", 17, C.MULTI_W128),
                                            ("kktz832", 17, 0), ("indef834", 3, 0), ("indef834", 17, 0)],
                         ids=["N72-looped", "N72-fused", "N72-panels", "N832-fused", "N834-looped", "N834-panels"])
def test_padding_keeps_its_bits(ctx, name, nrhs, bits):
    keys = C.BATCHES[name]
    N = C.order(keys[0])
    f = _factors(ctx, keys, ld=N + 10)
    ldb, sB = N + 6, nrhs * (N + 6) + 10
    buf, before = f.solve(_rhs(keys, nrhs), bits, ldb=ldb, sB=sB, fill=FILL)
    pad = np.ones(sB, dtype=bool)
    for r in range(nrhs):
        pad[r * ldb:r * ldb + N] = False
    assert pad.sum() == nrhs * 6 + 10
    assert np.array_equal(_bits(buf[:, pad]), _bits(before[:, pad]))
    assert (before[:, pad] == FILL).all()
    assert C.row_err(_rows(buf, nrhs, N, ldb), C.batch_reference(keys)[:, :nrhs]) < C.TOL


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [C.MULTI_BLOCKED, C.MULTI_BLOCKED | C.MULTI_W128], ids=["fused", "panels"])
def test_a_singular_system_between_two_regular_ones(ctx, bits):
    # system 1 has two all-zero columns: the reference divides by zero and its
    # kp = 0 defect swaps backwards.  The prepare raises that system's flag only:
    # its blocked launches exit and one launch runs the reference's sweeps on
    # its rows (inf and NaN values, no fault); systems 0 and 2 stay blocked.
    keys = C.SINGULAR
    N = C.order(keys[0])
    d = DevBatch(ctx, [C.system(k)[0] for k in keys])
    rc, info = d.factor()
    assert rc == 162 and list(info) == C.SINGULAR_DEVICE_INFO
    d.prepare()
    rows = _rhs(keys, 17)
    X = d.x(rows, bits)
    X_ref = C.batch_reference(keys)[:, :17]
    regular = _factors(ctx, [keys[0], keys[2]])
    Xr = regular.x(rows[[0, 2]], bits)
    for q, qq in ((0, 0), (2, 1)):
        assert C.row_err(X[q], X_ref[q]) < C.TOL, q
        assert np.array_equal(_bits(X[q]), _bits(Xr[qq])), q
    assert not np.isfinite(X_ref[1]).all()
    assert np.array_equal(np.isfinite(X[1]), np.isfinite(X_ref[1]))
    single = np.stack([d.single(1, b) for b in rows[1]])
    assert np.array_equal(X[1], single, equal_nan=True)
    fin = np.isfinite(single)
    assert np.array_equal(_bits(X[1][fin]), _bits(single[fin]))


# 7 ---------------------------------------------------------------------------
QPS = [(48, 16, 8, 3, 2000), (640, 160, 32, 2, 2100)]


def _qp_batch(c, ctx, **kw):
    n, m, p, B, seed0 = c
    kw.setdefault("equality_handling", I.EQ_NONE)
    bt = I.Batch(n, m, p, B, ctx, **kw)
    bt.generate(seed0)
    return bt


def _qp_solve(bt, rows, bits=0):
    B, nrhs, N = rows.shape
    t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    I.debug_inject(bits)
    try:
        rc, info = bt.kkt_solve_all_bk(t.data_ptr(), nrhs, N, nrhs * N)
    finally:
        I.debug_inject(0)
    assert rc == 0 and not info.any()
    return t.cpu().numpy()


def _qp_reference(K_lower, rows):
    F, piv, info = oracle.bk_factor(K_lower + np.tril(K_lower, -1).T)
    assert info == 0
    return np.stack([oracle.bk_solve(F, piv, np.array(b)) for b in rows])


@pytest.mark.parametrize("c", QPS, ids=["N72", "N832"])
def test_qp_level(ctx, c):
    n, m, p, B, seed0 = c
    bt = _qp_batch(c, ctx)
    N = bt.N
    rows = np.array(C.rhs(N, B)[:, :17])
    for q in range(B):
        o = oracle.OracleQP(oracle.gen_qp(n, m, p, seed0 + q), eq_none=True)
        assert np.array_equal(_bits(bt.kkt_of(q)), _bits(np.tril(o.kkt()))), q
    for it in range(2):  # iterate 0, and after one step
        X_ref = [_qp_reference(bt.kkt_of(q), rows[q]) for q in range(B)]
        for bits in (0, C.MULTI_BLOCKED | C.MULTI_W128):
            for nrhs in (3, 17):
                X = _qp_solve(bt, rows[:, :nrhs], bits)
                for q in range(B):
                    err = C.row_err(X[q], X_ref[q][:nrhs])
                    assert err < C.TOL, (it, bits, nrhs, q, err)
        bt.step()


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, I.STEP_GRAPH], ids=["eager", "graph"])
def test_steps_unchanged(ctx, flags):
    a, b = _qp_batch(QPS[0], ctx), _qp_batch(QPS[0], ctx)
    rows = np.array(C.rhs(a.N, a.batch)[:, :17])
    for it in range(3):
        _qp_solve(a, rows, C.MULTI_BLOCKED if it % 2 else 0)
        a.step(flags)
        b.step(flags)
        if flags & I.STEP_GRAPH:
            assert a.last_step_graph() and b.last_step_graph(), it
        assert np.array_equal(_bits(a.batch_scalars()), _bits(b.batch_scalars())), it
        for i in range(a.batch):
            for which in range(4):
                assert np.array_equal(_bits(a.state(i, which)), _bits(b.state(i, which))), (it, i, which)


# 9 ---------------------------------------------------------------------------
def test_arguments(ctx):
    keys = C.BATCHES["indef72"]
    f = _factors(ctx, keys)
    N, B = f.N, f.batch
    t = torch.zeros(B * 4 * (N + 2) + 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr, ws = t.data_ptr(), f.ws.data_ptr()
    head = f.args()
    for nrhs, ldb, sB, off in ((-1, N, 4 * N, 0), (2, N - 2, 2 * N, 0), (2, N + 1, 2 * (N + 1), 0), (2, N, 2 * N - 2, 0),
                               (2, N, 2 * N + 1, 0), (2, N, 2 * N, 8)):
        with pytest.raises(I.IpmzError):
            ctx.bk_solve_multi_batch(*head, ws, ptr + off, ldb, sB, nrhs)
    odd_sA = (N, B, f.A.data_ptr(), f.ld, f.sA + 1, f.piv.data_ptr(), f.sP)
    with pytest.raises(I.IpmzError, match="sA even"):
        ctx.bk_solve_multi_batch(*odd_sA, ws, ptr, N, 2 * N, 2)
    with pytest.raises(I.IpmzError, match="sA even"):
        ctx.bk_prepare_solve_batch(*odd_sA, ws, f.wsb)
    with pytest.raises(I.IpmzError, match="4096"):
        ctx.bk_solve_multi_batch(4098, 1, f.A.data_ptr(), 4098, 4098 * 4098, f.piv.data_ptr(), 4098, ws, ptr, 4098,
                                 2 * 4098, 2)
    with pytest.raises(I.IpmzError, match="4096"):
        ctx.bk_factor_batch(4098, 1, f.A.data_ptr(), 4098, 4098 * 4098, f.piv.data_ptr(), 4098)
    with pytest.raises(I.IpmzError, match="null pointer"):
        ctx.bk_solve_multi_batch(*head, 0, ptr, N, 2 * N, 2)
    with pytest.raises(I.IpmzError, match="workspace too small"):
        ctx.bk_prepare_solve_batch(*head, ws, f.wsb - 1)
    assert ctx.bk_batch_solve_workspace_bytes(N, B) == f.wsb > B * 16 * N * N
    # no-ops: nothing is read or written
    assert ctx.bk_solve_multi_batch(*head, ws, ptr, N, 0, 0) == 0
    assert ctx.bk_solve_multi_batch(0, B, 0, 0, 0, 0, 0, 0, 0, 2, 6, 3) == 0
    assert ctx.bk_solve_multi_batch(N, 0, 0, N, 0, 0, 0, 0, 0, N, 2 * N, 2) == 0
    assert ctx.bk_prepare_solve_batch(0, B, 0, 0, 0, 0, 0, 0, 0) == 0
    assert ctx.bk_prepare_solve_batch(N, 0, 0, N, 0, 0, 0, 0, 0) == 0
    rc, info = ctx.bk_factor_batch(N, 0, 0, N, 0, 0, 0)
    assert rc == 0 and info.size == 0
    rc, info = ctx.bk_factor_batch(0, 2, 0, 0, 0, 0, 0)
    assert rc == 0 and list(info) == [0, 0]
    ctx.sync()
    assert not t.cpu().numpy().any()


def test_states_and_handlings(ctx):
    c = QPS[0]
    n, m, p, B, seed0 = c
    bt = _qp_batch(c, ctx)
    N = bt.N
    t = torch.zeros(B * 4 * (N + 2) + 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = t.data_ptr()
    rc, info = bt.kkt_solve_all_bk(ptr, 0, N, 0)  # nrhs == 0: assembles, factors, returns the info words
    assert rc == 0 and list(info) == [0] * B
    assert not t.cpu().numpy().any()
    for nrhs, ldb, sB, off in ((-1, N, 4 * N, 0), (2, N - 2, 2 * N, 0), (2, N + 1, 2 * (N + 1), 0), (2, N, 2 * N - 2, 0),
                               (2, N, 2 * N + 1, 0), (2, N, 2 * N, 8)):
        with pytest.raises(I.IpmzError):
            bt.kkt_solve_all_bk(ptr + off, nrhs, ldb, sB)
    reg = _qp_batch(c, ctx, equality_handling=I.EQ_REGULARIZATION)
    with pytest.raises(I.IpmzError, match="EqualityHandling::None"):
        reg.kkt_solve_all_bk(ptr, 2, N, 2 * N)
    unloaded = I.Batch(n, m, p, B, ctx, equality_handling=I.EQ_NONE)
    with pytest.raises(I.IpmzError, match="bad state"):
        unloaded.kkt_solve_all_bk(ptr, 2, N, 2 * N)
    q = oracle.gen_qp(n, m, p, seed0)
    bt.load_one(0, I.Data(q["Q"], q["c"], q["lx"], q["ux"], q["A"], q["lA"], q["uA"], q["C"], q["d"]))
    with pytest.raises(I.IpmzError, match="bad state"):  # a load leaves the batch uninitialized
        bt.kkt_solve_all_bk(ptr, 2, N, 2 * N)
    bt.initialize()
    assert bt.kkt_solve_all_bk(ptr, 2, N, 2 * N)[0] == 0


def test_batch_of_one_is_the_single_solve(ctx):
    n, m, p, _, seed0 = QPS[0]
    one = I.Batch(n, m, p, 1, ctx, equality_handling=I.EQ_NONE)
    one.generate(seed0)
    g = I.Optimizer(n, m, p, ctx, equality_handling=I.EQ_NONE)
    g.generate(seed0)
    N = one.N
    rows = np.array(C.rhs(N, 1)[0, :17])
    ta, tb = torch.from_numpy(rows.copy()).cuda(), torch.from_numpy(rows.copy()).cuda()
    torch.cuda.synchronize()
    rc, info = one.kkt_solve_all_bk(ta.data_ptr(), 17, N, 12345)  # (sB ignored)
    assert rc == 0 and list(info) == [0]
    assert g.kkt_solve_bk(tb.data_ptr(), 17, N) == 0
    assert torch.equal(ta, tb)
    assert C.row_err(ta.cpu().numpy(), _qp_reference(g.kkt(), rows)) < C.TOL
