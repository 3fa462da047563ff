"""Forward-mode sensitivities of the residual vectors on the device (ipmz_batch_data_jvp:
Optimizer.data_jvp_tensors and the raw call), through the public ABI only.

Reference (tests/data_jvp_cases.py): jc.jvp_reference, the formulation's shorthand definitions in longdouble with the
tangents as data (tests/test_oracle_data_jvp.py pins it on the CPU).  Bound: the project's bar nc.TOL = 1e-10 relative
to max(1, |ref|inf) per row, or per term of the bilinear identity.  Every test prints its worst figure before it
asserts.
"""
import ctypes

import numpy as np
import pytest

import data_jvp_cases as jc
import data_vjp_cases as dc
import newton_multi_cases as nc

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

NAN = float("nan")
S1 = jc.SHAPES[1]
SEED0 = 1000


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _dev(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _solver(c, B, ctx, name="box", steps=2, seed0=SEED0):
    """(solver, the iterates of its QPs): a single QP (B == 1: an Optimizer) or a Batch, after `steps` steps."""
    n, m, p = c
    s = I.Optimizer(n, m, p, ctx, **dc.form_kw(name)) if B == 1 else I.Batch(n, m, p, B, ctx, **dc.form_kw(name))
    s.generate(seed0)
    for _ in range(steps):
        s.step()
    return s, ([s.vars()] if B == 1 else [s.state(i) for i in range(B)])


def _devd(D, keys=None):
    return {k: _dev(a) for k, a in D.items() if keys is None or k in keys}


def _reference(name, c, vs, D, shared):
    """(B, ntan, L) reference rows."""
    q = dict(n=c[0], m=c[1], p=c[2])
    ntan = next(iter(D.values())).shape[0 if shared else 1]
    return np.stack([np.stack([jc.jvp_reference(name, q, v, jc.one(D, t, None if shared else i))
                               for t in range(ntan)]) for i, v in enumerate(vs)])


def _jvp(s, D):
    L = s.state_len
    R = s.data_jvp_tensors(D)
    assert R.shape[2] == nc.even(L)
    return _host(R)[:, :, :L]


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 3), ids=("single", "batch3"))
@pytest.mark.parametrize("name", dc.FORM_NAMES)
def test_R_against_the_reference(ctx, name, B):
    c = S1
    s, vs = _solver(c, B, ctx, name)
    zero = jc.zero_slots(name, *c)
    worst = 0.0
    for ntan in jc.NTANS:
        for shared in (False, True):
            D = jc.tangents(*c, ntan, None if shared else B)
            R = _jvp(s, _devd(D))
            ref = _reference(name, c, vs, D, shared)
            assert R.shape == ref.shape == (B, ntan, s.state_len)
            worst = max(worst, jc.row_err(R, ref))
            assert not R[:, :, zero].any(), "the slots no datum enters are exactly 0.0"
    print(f"{name} B={B}: worst row error vs the reference {worst:.3e} (bound {nc.TOL:.1e})", flush=True)
    assert worst <= nc.TOL


@pytest.mark.parametrize("c", [jc.SHAPES[0], jc.SHAPES[2]] + jc.M0_SHAPES, ids=nc.case_id)
def test_shapes(ctx, c):
    """The other shapes of the table (partial tiles, an odd tile count, m = 0, p = 0), every formulation the shape
    admits, a single QP and a batch of 3, ntan = 3."""
    worst = 0.0
    for name in (dc.FORM_NAMES if c[1] else dc.M0_FORMS):
        for B in (1, 3):
            s, vs = _solver(c, B, ctx, name)
            for shared in (False, True):
                D = jc.tangents(*c, 3, None if shared else B)
                worst = max(worst, jc.row_err(_jvp(s, _devd(D)), _reference(name, c, vs, D, shared)))
    print(f"{nc.case_id(c)}: worst row error {worst:.3e} (bound {nc.TOL:.1e})", flush=True)
    assert worst <= nc.TOL


@pytest.mark.parametrize("B", jc.BATCHES)
def test_batches(ctx, B):
    c = jc.SHAPES[0]
    s, vs = _solver(c, B, ctx)
    worst = 0.0
    for ntan in (1, 6):
        for shared in (False, True):
            D = jc.tangents(*c, ntan, None if shared else B)
            worst = max(worst, jc.row_err(_jvp(s, _devd(D)), _reference("box", c, vs, D, shared)))
    print(f"B={B}: worst row error {worst:.3e} (bound {nc.TOL:.1e})", flush=True)
    assert worst <= nc.TOL


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("shared", (False, True), ids=("per_qp", "shared"))
@pytest.mark.parametrize("name", dc.FORM_NAMES)
def test_duality_on_the_device(ctx, name, shared):
    """<W, data_jvp(D)> = sum <data_grad_tensors(W), D>, both sides the device's."""
    c, B, ntan = S1, 3, 3
    s, _ = _solver(c, B, ctx, name)
    L = s.state_len
    W = np.array(dc.cotangents(L, B))
    names = dc.present(*c)
    grads = {k: _host(t) for k, t in s.data_grad_tensors(_dev(W), shared=names if shared else ()).items()}
    D = jc.tangents(*c, ntan, None if shared else B)
    R = _jvp(s, _devd(D))
    worst = 0.0
    for t in range(ntan):
        if shared:  # one identity for the batch: the vjp's blocks are the sums over the QPs
            pairs = [(W, R[:, t], grads, jc.one(D, t))]
        else:
            pairs = [(W[i], R[i, t], {k: g[i] for k, g in grads.items()}, jc.one(D, t, i)) for i in range(B)]
        for w, r, g, d in pairs:
            gap, bound = dc.bilinear_gap(w, np.zeros_like(r), r, g, d), dc.bilinear_bound(w, np.zeros_like(r), r)
            assert bound > 0
            worst = max(worst, gap / bound)
    print(f"{name} shared={shared}: worst |<W, R> - sum <g, D>| / bound {worst:.3e}", flush=True)
    assert worst <= 1.0


# 3 ---------------------------------------------------------------------------
def _strided(a, rows_dims, shared, off, odd):
    """The tangents `a` ((B, ntan, ...) or (ntan, ...)) as a view into a NaN-filled buffer: element offset `off`, row,
    tangent and QP strides padded -- all even (the 16-byte path) or, odd, the row and tangent strides odd."""
    a = np.asarray(a)
    lead = 1 if shared else 2
    inner = a.shape[lead:]
    fix = (lambda k: k | 1) if odd else (lambda k: k + (k & 1))
    if rows_dims == 2:
        ld = fix(inner[1] + 2)
        extent = (inner[0] - 1) * ld + inner[1]
        strides = (ld, 1)
    else:
        extent = inner[0]
        strides = (1,)
    ntan = a.shape[lead - 1]
    tq = fix(extent + 2)
    sq = (ntan - 1) * tq + extent + (3 if odd else 4)
    sq = sq if odd else sq + (sq & 1)
    total = off + (1 if shared else a.shape[0]) * sq + 4
    buf = torch.full((total,), NAN, dtype=torch.float64, device="cuda")
    view = torch.as_strided(buf, a.shape, ((tq,) if shared else (sq, tq)) + strides, off)
    view.copy_(torch.from_numpy(np.array(a)).cuda())
    torch.cuda.synchronize()
    return view


def _views(D, shared, off, odd):
    return {k: _strided(a, 2 if k in dc.MATRICES else 1, shared, off, odd) for k, a in D.items()}


@pytest.mark.parametrize("shared", (False, True), ids=("per_qp", "shared"))
@pytest.mark.parametrize("c", [(48, 16, 8), (13, 5, 3), (131, 20, 3), (257, 5, 3)], ids=nc.case_id)
def test_layout_independence_bitwise(ctx, c, shared):
    B, ntan = 3, 17
    s, vs = _solver(c, B, ctx)
    D = jc.tangents(*c, ntan, None if shared else B)
    base = _jvp(s, _devd(D))
    assert jc.row_err(base, _reference("box", c, vs, D, shared)) <= nc.TOL
    # aligned, even strides with NaN padding (16-byte loads) | one element off, odd row and tangent strides
    assert _same(_jvp(s, _views(D, shared, 0, False)), base), "padded 16-byte path"
    assert _same(_jvp(s, _views(D, shared, 1, True)), base), "element path"
    assert _same(_jvp(s, _devd(D)), base), "two identical calls"
    # row t of the call = the call with that tangent alone
    for t in (0, 5, 16):
        alone = {k: (a[t:t + 1] if shared else a[:, t:t + 1]) for k, a in D.items()}
        assert _same(_jvp(s, _devd(alone))[:, 0], base[:, t]), ("tangent alone", t)
    # QP q of the batch = a batch holding QP q's iterate (per-QP tangents: a solver of one QP; shared tangents are a
    # batch's layout: a batch of two, both QP q)
    n, m, p = c
    for i in range(B):
        if shared:
            two = I.Batch(n, m, p, 2, ctx)
            two.generate(SEED0)
            two.set_state(0, vs[i])
            two.set_state(1, vs[i])
            got = _jvp(two, _devd(D))
            assert _same(got[0], base[i]) and _same(got[1], base[i]), ("QP in another batch", i)
        else:
            one = I.Optimizer(n, m, p, ctx)
            one.generate(SEED0)
            one.set_vars(vs[i])
            assert _same(_jvp(one, _devd({k: a[i:i + 1] for k, a in D.items()}))[0], base[i]), ("QP alone", i)
    print(f"{nc.case_id(c)} shared={shared}: 16-byte and element paths, single tangents, single QPs and a second call "
          "all bitwise equal; NaN padding unread", flush=True)


# 4 ---------------------------------------------------------------------------
def _everything(g):
    return [g.state(i, w) for i in range(g.batch) for w in range(4)] + [g.batch_scalars()] + \
        [g.kkt_of(i) for i in range(g.batch)]


@pytest.mark.parametrize("name", ("box", "none"))
def test_nothing_else_moves(ctx, name):
    c, B, ntan = S1, 3, 3
    a, _ = _solver(c, B, ctx, name, steps=1)
    b, _ = _solver(c, B, ctx, name, steps=1)
    L = b.state_len
    ldr, pad = nc.even(L) + 2, 4
    sR = ntan * ldr + pad
    sentinel = -123.25
    for k in range(3):
        before = _everything(b)
        buf = torch.full((B * sR,), sentinel, dtype=torch.float64, device="cuda")
        out = torch.as_strided(buf, (B, ntan, L), (sR, ldr, 1))
        shared = bool(k % 2)
        D = jc.tangents(*c, ntan, None if shared else B)
        R = b.data_jvp_tensors(_devd(D), out=out)
        assert R.data_ptr() == buf.data_ptr()
        full = _host(buf).reshape(B, sR)
        rows = full[:, :ntan * ldr].reshape(B, ntan, ldr)
        assert _same(rows[:, :, :L], _jvp(b, _devd(D))), "out= and a fresh tensor"
        assert (rows[:, :, L:] == sentinel).all() and (full[:, ntan * ldr:] == sentinel).all(), "R's padding keeps its bits"
        for x, y in zip(before, _everything(b)):
            assert np.array_equal(x, y, equal_nan=True), "the call itself"
        a.step(I.STEP_GRAPH)
        b.step(I.STEP_GRAPH)
    assert a.last_step_graph() and b.last_step_graph()
    for x, y in zip(_everything(a), _everything(b)):
        assert np.array_equal(x, y, equal_nan=True)
    print(f"{name}: iterate, scalars, kkt and graph-replayed steps bitwise those of the twin; R's padding untouched",
          flush=True)


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("shared", (False, True), ids=("per_qp", "shared"))
def test_null_blocks_are_zero_tangents(ctx, shared):
    c, B, ntan = S1, 3, 3
    s, vs = _solver(c, B, ctx)
    D = jc.tangents(*c, ntan, None if shared else B)
    all_ = _jvp(s, _devd(D))
    total = np.zeros_like(all_)
    worst = 0.0
    for k in D:
        Rk = _jvp(s, _devd(D, (k,)))
        worst = max(worst, jc.row_err(Rk, _reference("box", c, vs, {k: D[k]}, shared)))
        total += Rk
    err = jc.row_err(total, all_)
    print(f"shared={shared}: each block alone vs the reference {worst:.3e}; their sum vs all blocks {err:.3e} "
          f"(bound {nc.TOL:.1e})", flush=True)
    assert worst <= nc.TOL and err <= nc.TOL


def _raw(s, ntan, spec, R, ldr, sR):
    """The C call itself.  spec: load_tensors' name -> (address, row stride, QP stride, tangent stride)."""
    tan = I._QPDeviceTangent()
    tname = dict(Q="tQ", A="tA", C="tC", c="tc", l_x="tlx", u_x="tux", l_A="tlA", u_A="tuA", d="td")
    for name, ptr, ld, sq, rows, cols in I._BLOCKS:
        if name in spec:
            a, l, sv, tv = spec[name]
            setattr(tan.d, ptr, a)
            if ld:
                setattr(tan.d, ld, l)
            setattr(tan.d, sq, sv)
            setattr(tan, tname[ptr], tv)
    torch.cuda.synchronize()
    I._check(I.lib.ipmz_batch_data_jvp(s.h, ntan, ctypes.byref(tan), ctypes.c_void_p(R), ldr, sR), "ipmz_batch_data_jvp")
    s.ctx.sync()


def test_blocks_of_dimension_zero_are_ignored(ctx):
    c, B, ntan = (40, 0, 0), 2, 3
    n = c[0]
    s, vs = _solver(c, B, ctx, steps=1)
    L = s.state_len
    D = jc.tangents(*c, ntan, B)
    assert set(D) == {"Q", "c", "l_x", "u_x"}
    dev = _devd(D)
    ref = _jvp(s, {k: dev[k] for k in ("Q", "c")})
    ldr = nc.even(L)
    R = torch.full((B, ntan, ldr), NAN, dtype=torch.float64, device="cuda")
    junk = 0xdead0
    _raw(s, ntan, dict(Q=(dev["Q"].data_ptr(), n, ntan * n * n, n * n), c=(dev["c"].data_ptr(), 0, ntan * n, n),
                       A_ineq=(junk, 1, -5, -1), l_A_ineq=(junk, 0, 1, 0), u_A_ineq=(junk, 0, 1, 0),
                       A_eq=(junk, 0, 0, 0), b_eq=(junk, 0, -1, -1)), R.data_ptr(), ldr, ntan * ldr)
    assert _same(_host(R)[:, :, :L], ref)
    print("m = 0, p = 0: garbage A / C / l_A / u_A / d blocks ignored", flush=True)


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", jc.LOOPS, ids=[c[0] for c in jc.LOOPS])
def test_every_loop(ctx, case):
    """Every loop of csrc/jvp.hip at the smallest case that reaches it, at the initial iterate."""
    _, c, B, ntan, what = case
    s, vs = _solver(c, B, ctx, steps=0)
    L = s.state_len
    worst = 0.0
    # (the large batch: the reference of a few QPs -- the first, one past gridDim.y's reach, the last)
    picks = sorted({0, min(B - 1, jc.ROWS_GY // ntan + 1), B - 1})
    for shared in ((False, True) if B > 1 else (False,)):
        D = jc.tangents(*c, ntan, None if shared else B)
        R = _jvp(s, _devd(D))
        assert not np.isnan(R).any()
        for i in picks:
            Di = D if shared else {k: a[i:i + 1] for k, a in D.items()}
            worst = max(worst, jc.row_err(R[i:i + 1], _reference("box", c, [vs[i]], Di, shared)))
    print(f"{case[0]} ({what}): worst row error {worst:.3e} (bound {nc.TOL:.1e})", flush=True)
    assert worst <= nc.TOL


# 7 ---------------------------------------------------------------------------
def test_errors(ctx):
    n, m, p = c = S1
    B, ntan = 3, 2
    bt, _ = _solver(c, B, ctx, steps=0)
    L = bt.state_len
    ldr = nc.even(L)
    R = torch.zeros((B, ntan, ldr), dtype=torch.float64, device="cuda")
    Rp, sR = R.data_ptr(), ntan * ldr
    tq, tc = _dev(np.zeros((B, ntan, n, n))), _dev(np.zeros((B, ntan, n)))
    Q, cc = tq.data_ptr(), tc.data_ptr()
    good = dict(Q=(Q, n, ntan * n * n, n * n), c=(cc, 0, ntan * n, n))

    def invalid(g, *a):
        with pytest.raises(I.IpmzError, match="invalid argument"):
            _raw(g, *a)

    def state(g, *a):
        with pytest.raises(I.IpmzError, match="bad state"):
            _raw(g, *a)

    _raw(bt, ntan, good, Rp, ldr, sR)
    _raw(bt, 0, good, Rp, ldr, sR)                                          # ntan == 0: a no-op
    lib, tan, vp = I.lib, I._QPDeviceTangent(), ctypes.c_void_p
    assert lib.ipmz_batch_data_jvp(None, ntan, ctypes.byref(tan), vp(Rp), ldr, sR) == -1
    assert lib.ipmz_batch_data_jvp(bt.h, ntan, None, vp(Rp), ldr, sR) == -1
    assert lib.ipmz_batch_data_jvp(bt.h, ntan, ctypes.byref(tan), None, ldr, sR) == -1
    invalid(bt, -1, good, Rp, ldr, sR)                                      # ntan < 0
    invalid(bt, ntan, good, Rp, L - 1 - (L & 1), sR)                        # ldr < state_len
    invalid(bt, ntan, good, Rp, ldr + 1, sR + 2)                            # odd ldr
    invalid(bt, ntan, good, Rp, ldr, sR - 2)                                # sR < ntan * ldr
    invalid(bt, ntan, good, Rp, ldr, sR + 1)                                # odd sR
    invalid(bt, ntan, good, Rp + 8, ldr, sR)                                # R not 16-byte aligned
    invalid(bt, ntan, dict(Q=(Q, n - 1, ntan * n * n, n * n)), Rp, ldr, sR)  # row stride < n
    invalid(bt, ntan, dict(Q=(Q, n, ntan * n * n, n * n - 1)), Rp, ldr, sR)  # tangent stride below the extent
    invalid(bt, ntan, dict(Q=(Q, n, ntan * n * n - 1, n * n)), Rp, ldr, sR)  # QP stride below the tangents' extent
    invalid(bt, ntan, dict(Q=(Q, n, -n * n, n * n)), Rp, ldr, sR)            # negative strides
    invalid(bt, ntan, dict(Q=(Q, n, ntan * n * n, -1)), Rp, ldr, sR)
    invalid(bt, ntan, dict(c=(cc, 0, ntan * n, n - 1)), Rp, ldr, sR)         # vector tangent stride below its length
    invalid(bt, ntan, dict(c=(cc, 0, 2 * n - 1, n)), Rp, ldr, sR)
    invalid(bt, ntan, dict(c=(cc, 0, -1, n)), Rp, ldr, sR)
    _raw(bt, 1, dict(c=(cc, 0, n, -3)), Rp, ldr, ldr)                        # ntan == 1: the tangent stride is unused
    for kw in (dict(equality_handling=I.EQ_SLACKED_SLACKS),
               dict(equality_handling=I.EQ_NAIVE_SLACKS, inequality_handling=I.INEQ_NAIVE_SLACKS)):
        e = I.Batch(n, m, p, B, ctx, **kw)
        e.generate(SEED0)
        le = nc.even(e.state_len)
        big = torch.zeros((B, ntan, le), dtype=torch.float64, device="cuda")
        invalid(e, ntan, good, big.data_ptr(), le, ntan * le)
    fresh = I.Batch(n, m, p, B, ctx)
    state(fresh, ntan, good, Rp, ldr, sR)                                    # before a load
    q = nc.qp(n, m, p, SEED0)
    bt.load_one(0, I.Data(q["Q"], q["c"], q["lx"], q["ux"], q["A"], q["lA"], q["uA"], q["C"], q["d"]))
    state(bt, ntan, good, Rp, ldr, sR)                                       # between load_one and initialize
    bt.initialize()
    _raw(bt, ntan, good, Rp, ldr, sR)
    # single QPs: the reduction and mixed precision are refused; the QP strides and sR are ignored
    g, _ = _solver(c, 1, ctx, steps=0)
    one = dict(Q=(Q, n, -7, n * n), c=(cc, 0, 1, n))
    _raw(g, ntan, one, Rp, ldr, 1)
    g.set_reduction(I.REDUCTION_NORMAL)
    invalid(g, ntan, one, Rp, ldr, sR)
    g.set_reduction(I.REDUCTION_AUGMENTED)
    g.set_mixed_precision(True)
    invalid(g, ntan, one, Rp, ldr, sR)
    g.set_mixed_precision(False)
    _raw(g, ntan, one, Rp, ldr, sR)
    # data_jvp_tensors: the tensors agree on ntan
    D = _devd(jc.tangents(*c, 3, B))
    D["c"] = D["c"][:, :2]
    with pytest.raises(ValueError, match="tangents"):
        bt.data_jvp_tensors(D)
    print("errors: every IPMZ_ERR_INVALID / IPMZ_ERR_STATE case", flush=True)


def test_capture_needs_the_workspace_first():
    """Inside a caller's graph capture the call is enqueued like any launch, but the products' workspace cannot be
    allocated there: IPMZ_ERR_STATE until one call outside a capture has made it."""
    n, m, p = c = S1
    B, ntan = 3, 2
    st = torch.cuda.Stream()
    cx = I.Context(0, stream=st.cuda_stream)
    try:
        bt, _ = _solver(c, B, cx, steps=1)
        L = bt.state_len
        ldr = nc.even(L)
        D = _devd(jc.tangents(*c, ntan, B))
        ref_c = _jvp(bt, {"c": D["c"]})                                      # (vectors only: no workspace)
        R = torch.full((B, ntan, ldr), NAN, dtype=torch.float64, device="cuda")
        vec = dict(c=(D["c"].data_ptr(), 0, ntan * n, n))
        mat = dict(Q=(D["Q"].data_ptr(), n, ntan * n * n, n * n))

        def call(spec):
            tan = I._QPDeviceTangent()
            for name, (a, l, sv, tv) in spec.items():
                setattr(tan.d, name, a)
                if l:
                    tan.d.ldq = l
                setattr(tan.d, "s" + name, sv)
                setattr(tan, "t" + name, tv)
            return I.lib.ipmz_batch_data_jvp(bt.h, ntan, ctypes.byref(tan), ctypes.c_void_p(R.data_ptr()), ldr, ntan * ldr)

        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st, capture_error_mode="thread_local"):
            assert call(mat) == -5                                           # IPMZ_ERR_STATE
            assert b"capturing" in I.lib.ipmz_last_error()
            assert call(vec) == 0                                            # no allocation: captured
        graph.replay()
        torch.cuda.synchronize()
        assert _same(_host(R)[:, :, :L], ref_c)
        ref_q = _jvp(bt, {"Q": D["Q"]})                                      # outside: allocates
        graph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph2, stream=st, capture_error_mode="thread_local"):
            assert call(mat) == 0
        graph2.replay()
        torch.cuda.synchronize()
        assert _same(_host(R)[:, :, :L], ref_q)
        bt.close()
    finally:
        cx.close()
    print("capture: refused while the workspace is missing, captured and replayed once it exists", flush=True)
