"""The forked single-QP step runs memory-bound work in the factor's two idle
edges (DESIGN.md §4 "The factor's idle edges"): the assembly of the columns
beyond the first outer panel beside that panel, and -- with the affine
right-hand side moved ahead of the factor -- the solve preparation and the
forward sweep of the rows that are already final beside the factor's
chain-bound tail.  It is reordering under stream order and events only: every
element goes through the same operations in the same order, so everything a
step leaves must equal, bit for bit, what the serial order
(debug bit DEBUG_SERIAL_EDGES) leaves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

SEED = 77
SMALL = dict(nbo=128, nbi=64)  # three or more outer panels at small N
FLAGS = I.STEP_RESTART_IF_CONVERGED


@pytest.fixture(autouse=True)
def clean_mask():
    yield
    I.debug_inject(0)


def _snapshot(q, factor):
    s = dict(vars=q.vars(), daff=q.daff(), dir=q.dir(), res=q.residuals(),
             scal=np.array([v for _, v in sorted(q.scalars().items())], dtype=np.float64))
    if factor:
        s["L"], s["D"], s["P"] = q.factor()
    return s


def _steps(shape, blocking, mask, steps=3, graph=False, factor_every_step=True):
    """`steps` Newton steps from generate(SEED) under debug mask `mask`; a snapshot after each"""
    n, m, p = shape
    I.debug_inject(mask)
    ctx = I.Context(0, **blocking)
    try:
        N = n + m + p
        q = I.Optimizer(n, m, p, ctx)
        q.generate(SEED)
        out = []
        for it in range(steps):
            q.step(FLAGS | (I.STEP_GRAPH if graph else 0))
            ctx.sync()
            assert q.last_step_graph() == (1 if graph else 0)
            out.append(_snapshot(q, factor_every_step or it == steps - 1))
        q.close()
        return N, out
    finally:
        ctx.close()
        I.debug_inject(0)


_serial = {}


def _reference(shape, blocking, **kw):
    """the serial order's snapshots, computed once per case"""
    key = (shape, tuple(sorted(blocking.items())), tuple(sorted(kw.items())))
    if key not in _serial:
        _serial[key] = _steps(shape, blocking, I.DEBUG_SERIAL_EDGES, **kw)
    return _serial[key]


def _assert_same(got, ref):
    assert len(got) == len(ref)
    for it, (a, b) in enumerate(zip(got, ref)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (it, k)


def _panels(ctx_blocking, N):
    ctx = I.Context(0, **ctx_blocking)
    try:
        nbo = ctx.blocking(N)[0]
    finally:
        ctx.close()
    return nbo, (N + nbo - 1) // nbo


@pytest.mark.parametrize("shape,blocking,panels,big", [
    ((320, 96, 64), SMALL, 4, False),   # N = 480: a partial last panel
    ((300, 70, 33), SMALL, 4, False),   # N = 403: not a multiple of 64
    ((256, 0, 0), SMALL, 2, False),     # two panels: the factor does not fork, neither split applies
    ((3072, 768, 260), {}, 9, True),    # N = 4100, default blocking: a GEMM-paced panel before the chain-paced
                                        # ones, so the early sweep runs by itself (512 rows)
])
def test_step_bitwise_equals_serial_order(shape, blocking, panels, big):
    N = sum(shape)
    assert _panels(blocking, N)[1] == panels
    kw = dict(factor_every_step=not big)
    _, ref = _reference(shape, blocking, **kw)
    _, got = _steps(shape, blocking, 0, **kw)
    _assert_same(got, ref)


@pytest.mark.parametrize("shape", [(300, 70, 33), (320, 96, 64)])  # N = 403, 480
@pytest.mark.parametrize("where", ["none", "one_block", "last", "beyond"])
def test_forced_split_boundaries(shape, where):
    N = sum(shape)
    rows = {"none": 0, "one_block": 128, "last": (N - 128) // 128 * 128, "beyond": (N + 127) // 128 * 128 + 128}[where]
    _, ref = _reference(shape, SMALL)
    _, got = _steps(shape, SMALL, I.debug_edge_rows(rows))
    _assert_same(got, ref)


DEBUG_TRACE = 64  # csrc/kernels.h: the host calls of a step to stderr


@pytest.mark.parametrize("shape,blocking,mask,head,rows", [
    ((3072, 768, 260), {}, 0, 512, 512),                               # by itself at N = 4100
    ((320, 96, 64), SMALL, 0, 128, 0),                                 # chain-bound throughout: the front edge only
    ((320, 96, 64), SMALL, I.debug_edge_rows(256), 128, 256),
    ((320, 96, 64), SMALL, I.debug_edge_rows(384), 128, 0),            # >= N - 128: no split
    ((320, 96, 64), SMALL, I.DEBUG_SERIAL_EDGES, None, 0),
    ((256, 0, 0), SMALL, 0, None, 0),                                  # two panels
])
def test_the_edges_are_used(capfd, shape, blocking, mask, head, rows):
    """the equalities above compare two orders: here, that the order under test is the overlapped one"""
    _steps(shape, blocking, mask | DEBUG_TRACE, steps=1, factor_every_step=False)
    err = capfd.readouterr().err
    if head is None:
        assert "step: edges" not in err and "work on B" not in err and "final with panel" not in err
        return
    assert f"step: edges, head columns {head}, early sweep rows {rows}" in err
    assert "factor: the caller's work on B before its first update" in err
    assert (f"step: forward sweep from row {rows} on" in err) == (rows > 0)
    assert ("final with panel" in err) == (rows > 0)


def test_captured_step_equals_eager_and_serial():
    """IPMZ_STEP_GRAPH capture of the forked step (INJECT_GRAPH_FORKS) with both edges at work: the
    early sweep forced to 256 of the N = 480 rows"""
    shape = (320, 96, 64)
    mask = I.INJECT_GRAPH_FORKS | I.debug_edge_rows(256)
    _, eager = _steps(shape, SMALL, mask)
    _, graph = _steps(shape, SMALL, mask, graph=True)
    _assert_same(graph, eager)
    _assert_same(graph, _reference(shape, SMALL)[1])


@pytest.mark.parametrize("mask_of", [lambda: 0, lambda: I.debug_edge_rows(256)])
def test_newton_solve_after_step(mask_of):
    """the multi-right-hand-side Newton solve directly after a step finds the factor and the prepared
    operators as the serial order leaves them"""
    shape = (320, 96, 64)
    rng = np.random.default_rng(5)
    res = {}
    for name, mask in (("serial", I.DEBUG_SERIAL_EDGES), ("edges", mask_of())):
        I.debug_inject(mask)
        ctx = I.Context(0, **SMALL)
        try:
            q = I.Optimizer(*shape, ctx)
            q.generate(SEED)
            q.step(FLAGS)
            L = q.state_len
            ld = L + (L & 1)
            if "R" not in res:
                res["R"] = np.zeros((4, ld))
                res["R"][:, :L] = rng.standard_normal((4, L))
            tR = torch.from_numpy(res["R"]).cuda()
            tD = torch.zeros_like(tR)
            assert q.newton_solve(tR.data_ptr(), tD.data_ptr(), 4, ld, ld) == 0
            res[name] = tD.cpu().numpy()
            q.step(FLAGS)  # and the step after it
            ctx.sync()
            res[name + "_vars"] = q.vars()
            q.close()
        finally:
            ctx.close()
            I.debug_inject(0)
    assert np.array_equal(res["edges"], res["serial"])
    assert np.array_equal(res["edges_vars"], res["serial_vars"])
