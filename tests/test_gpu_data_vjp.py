"""The gradient with respect to the problem data on the device (ipmz_batch_data_vjp:
Optimizer.data_grad_tensors and the raw call), through the public ABI only.

References (tests/data_vjp_cases.py): for the default form the numpy transposes of nc.residuals_numpy's expressions
(tests/test_oracle_data_vjp.py pins them on the CPU); for every other served formulation the bilinear identity
<w, r(theta + D) - r(theta)> = sum <g_theta, D_theta> on the device's own residual path, which this feature leaves
untouched.  Bound: the project's bar nc.TOL = 1e-10, relative to max(1, |ref|inf), or per term of the identity.
Every test prints its worst figure before it asserts.
"""
import ctypes

import numpy as np
import pytest

import batch_form_cases as fc
import data_vjp_cases as dc
import newton_multi_cases as nc

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

NAN = float("nan")
VECTORS = tuple(k for k in dc.NAMES if k not in dc.MATRICES)


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _dev(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return t


def _host(grads):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in grads.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _single(c, ctx, eq_none=False, seed=nc.SEED, **kw):
    n, m, p = c[:3]
    kw.setdefault("equality_handling", I.EQ_NONE if eq_none else I.EQ_REGULARIZATION)
    g = I.Optimizer(n, m, p, ctx, **kw)
    g.generate(seed)
    return g


def _batch(n, m, p, B, seed0, ctx, eq_none=False, **kw):
    bt = I.Batch(n, m, p, B, ctx, equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION, **kw)
    bt.generate(seed0)
    return bt


def _dims(g):
    return dict(n=g.n, m=g.m, p=g.p)


def _raw(g, W_ptr, sW, spec):
    """The C call itself.  spec: name -> (tensor or address, element offset, row stride, QP stride)."""
    gr = I._QPDeviceGrad()
    for name, ptr, ld, sq, rows, cols in I._BLOCKS:
        if name in spec:
            t, off, l, s = spec[name]
            setattr(gr, ptr, (t if isinstance(t, int) else t.data_ptr()) + 8 * off)
            if ld:
                setattr(gr, ld, l)
            setattr(gr, sq, s)
    torch.cuda.synchronize()
    I._check(I.lib.ipmz_batch_data_vjp(g.h, ctypes.c_void_p(W_ptr), sW, ctypes.byref(gr)), "ipmz_batch_data_vjp")
    g.ctx.sync()


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
@pytest.mark.parametrize("c", nc.SHAPES, ids=nc.case_id)
def test_default_form_vs_numpy(ctx, c, eq_none):
    q = nc.qp(*c)
    g = _single(c, ctx, eq_none)
    g.step()
    g.step()
    v = g.vars()
    L = g.state_len
    w = dc.cotangents(L)[0]
    got = _host(g.data_grad_tensors(_dev(w[None])))
    ref = dc.reference(q, v, w, eq_none)
    assert set(got) == set(ref) == set(dc.present(*c))
    worst = {k: dc.rel_err(got[k][0], ref[k]) for k in ref}
    print(f"{nc.case_id(c)} eq_none={eq_none}: worst vs numpy " +
          ", ".join(f"{k} {e:.2e}" for k, e in worst.items()) + f" (bound {nc.TOL:.1e}; bitwise but A_ineq, A_eq)",
          flush=True)
    for k in ref:
        if k in ("A_ineq", "A_eq"):
            assert worst[k] <= nc.TOL, k
        else:  # a copy, a negation or one product
            assert _same(got[k][0], ref[k]), k


# 2 ---------------------------------------------------------------------------
S1 = fc.S1
FORMS = [(name, f.kw, None) for name, f in fc.FORMS.items() if name not in ("eqss", "naiveeq")] + [
    # PenaltyFunction's r_lambda_C holds mu lambda_C and Slacks' mu is the mean of (x - l) lambda_y, ...: only the
    # blocks outside those products are perturbed (the bounds l_x, u_x, l_A, u_A are inside them)
    ("pen_sl", dict(equality_handling=I.EQ_PENALTY, inequality_handling=I.INEQ_SLACKS),
     ("Q", "c", "A_ineq", "A_eq", "b_eq")),
]
ABSENT = {"vlo": ("u_x",), "vup": ("l_x",), "vnone": ("l_x", "u_x"), "alo": ("u_A_ineq",), "aup": ("l_A_ineq",)}


@pytest.mark.parametrize("name,kw,blocks", FORMS, ids=[f[0] for f in FORMS])
def test_every_served_formulation_by_the_bilinear_identity(ctx, name, kw, blocks):
    n, m, p = S1
    q = nc.qp(n, m, p)
    theta = {k: q[dc.KEYS[k]] for k in dc.NAMES}
    g = I.Optimizer(n, m, p, ctx, **kw)
    g.load_tensors(**{k: _dev(a) for k, a in theta.items()})
    g.step()
    g.step()
    v = g.vars()
    g.set_vars(v)
    r0 = g.residuals()
    L = g.state_len
    worst = 0.0
    grads = []
    for k in range(2):
        w = dc.cotangents(L, 2)[k]
        grads.append(_host(g.data_grad_tensors(_dev(w[None]))))
    for k in range(2):
        w = dc.cotangents(L, 2)[k]
        deltas = dc.random_deltas(q, 200 + k, blocks)
        moved = dc.perturbed(q, deltas)
        assert (moved["lx"] < moved["ux"]).all() and (moved["lA"] < moved["uA"]).all()
        g.load_tensors(**{kk: _dev(moved[dc.KEYS[kk]]) for kk in dc.NAMES})
        g.set_vars(v)
        r1 = g.residuals()
        gr = {kk: a[0] for kk, a in grads[k].items()}
        gap, bound = dc.bilinear_gap(w, r0, r1, gr, deltas), dc.bilinear_bound(w, r0, r1)
        assert bound > 0
        worst = max(worst, gap / bound)
        for kk in ABSENT.get(name, ()):
            assert not gr[kk].any(), (name, kk)
        for kk in gr:
            assert not np.isnan(gr[kk]).any(), kk
    print(f"{name} L={L}: worst |<w, dr> - sum <g, D>| / bound {worst:.3e}", flush=True)
    assert worst <= 1.0


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", dc.BATCH_CASES, ids=lambda c: "n%d_m%d_p%d_B%d" % c)
def test_batches(ctx, c):
    n, m, p, B = c
    seed0 = 1000
    bt = _batch(n, m, p, B, seed0, ctx)
    bt.step()
    bt.step()
    L = bt.state_len
    W = np.array(dc.cotangents(L, B))
    Wt = _dev(W)
    per = _host(bt.data_grad_tensors(Wt))
    names = dc.present(n, m, p)
    assert set(per) == set(names)
    for k in names:
        assert per[k].shape[0] == B and not np.isnan(per[k]).any(), k
    # per-QP blocks: the same QP alone in a solver of one
    one = I.Optimizer(n, m, p, ctx)
    for i in range(B):
        one.generate(seed0 + i)
        one.set_vars(bt.state(i))
        alone = _host(one.data_grad_tensors(_dev(W[i:i + 1])))
        for k in names:
            assert _same(alone[k][0], per[k][i]), (k, i)
    # shared blocks: the sum over the batch
    sh = _host(bt.data_grad_tensors(Wt, shared=names))
    worst = 0.0
    for k in names:
        ref = per[k].sum(axis=0)
        assert sh[k].shape == ref.shape
        worst = max(worst, dc.rel_err(sh[k], ref))
    print(f"n{n} m{m} p{p} B{B}: per-QP blocks bitwise the QP alone; shared vs the sum of the per-QP blocks "
          f"{worst:.3e} (bound {nc.TOL:.1e})", flush=True)
    assert worst <= nc.TOL
    again = _host(bt.data_grad_tensors(Wt, shared=names))
    mixed = _host(bt.data_grad_tensors(Wt, shared=[k for k in names if k in dc.MATRICES]))
    only_q = _host(bt.data_grad_tensors(Wt, shared=["Q"], only=["Q"]))
    for k in names:
        assert _same(again[k], sh[k]), ("two runs", k)
        assert _same(mixed[k], sh[k] if k in dc.MATRICES else per[k]), ("shared matrices with per-QP vectors", k)
    assert set(only_q) == {"Q"} and _same(only_q["Q"], sh["Q"])


# 4 ---------------------------------------------------------------------------
def _layout(g, B, Wt, sW, off, pad_ld, pad_sq, shared=False):
    """Every block at element offset `off` of a NaN-filled buffer, row stride n + pad_ld, QP stride extent + pad_sq --
    or, shared, QP stride 0: one block per buffer, summed over the batch.
    Returns ({name: (B, ...) gathered block, (...) when shared}, every buffer's padding kept its bits)."""
    d = _dims(g)
    spec, bufs, where = {}, {}, {}
    for name, ptr, ld, sq, rows, cols in I._BLOCKS:
        r, c = (None if rows is None else d[rows]), d[cols]
        if c == 0 or r == 0:
            continue
        l = c + pad_ld if r is not None else 0
        extent = (r - 1) * l + c if r is not None else c
        s = 0 if shared else extent + pad_sq
        host = np.full(off + (extent if shared else B * s) + 4, NAN)
        bufs[name] = (host, _dev(host))
        spec[name] = (bufs[name][1], off, l, s)
        where[name] = (r, c, l, s)
    _raw(g, Wt.data_ptr(), sW, spec)
    out, clean = {}, True
    for name, (host, t) in bufs.items():
        r, c, l, s = where[name]
        dv = t.cpu().numpy()
        inside = np.zeros(dv.shape, bool)
        blocks = []
        for qi in range(1 if shared else B):
            base = off + qi * s
            if r is None:
                idx = base + np.arange(c)
            else:
                idx = (base + np.arange(r)[:, None] * l + np.arange(c)[None, :])
            inside[idx.reshape(-1)] = True
            blocks.append(dv[idx])
        out[name] = blocks[0] if shared else np.stack(blocks)
        clean = clean and np.array_equal(_bits(dv[~inside]), _bits(host[~inside])) and not np.isnan(dv[inside]).any()
    return out, clean


# n = 131: the element path's c += 64 loop makes three passes and the 16-byte path's c += 128 loop a second one
# that ends on the odd column's scalar store
@pytest.mark.parametrize("c", [(48, 16, 8, 3), (13, 5, 3, 2), (131, 5, 3, 2)], ids=("n48", "n13", "n131"))
def test_layout(ctx, c):
    n, m, p, B = c
    bt = _batch(n, m, p, B, 1000, ctx)
    bt.step()
    bt.step()
    L = bt.state_len
    Wt = _dev(np.array(dc.cotangents(L, B)))
    ref = _host(bt.data_grad_tensors(Wt))
    # 16-byte path with padding: even row and QP strides, aligned pointer
    vec, clean = _layout(bt, B, Wt, L, 0, 2 + (n & 1), 4 + (n & 1))
    assert clean, "16-byte path: padding and gaps keep their bits"
    # element path: odd strides and a pointer 8 bytes off 16-byte alignment
    sca, clean2 = _layout(bt, B, Wt, L, 1, 1 + (n & 1), 3)
    assert clean2, "element path: padding and gaps keep their bits"
    for k in ref:
        assert _same(vec[k], ref[k]), ("padded 16-byte path", k)
        assert _same(sca[k], ref[k]), ("element path", k)
    # a subset of the blocks: the others are not wanted (NULL), those asked for keep their bits
    sub = _host(bt.data_grad_tensors(Wt, only=["A_ineq", "l_x"]))
    assert set(sub) == {"A_ineq", "l_x"} and all(_same(sub[k], ref[k]) for k in sub)
    print(f"layout n={n}: 16-byte path, element path and a subset all bitwise equal; padding untouched", flush=True)


@pytest.mark.parametrize("c", [(48, 16, 8, 3), (131, 5, 3, 2)], ids=("n48", "n131"))
def test_layout_shared(ctx, c):
    """Shared blocks through the raw call: QP stride 0, a row stride other than n (k_grad_shared_sum's
    dst[(t / n) * ld + t % n]) and a pointer at element offset 0 and 1 of a NaN-filled buffer."""
    n, m, p, B = c
    bt = _batch(n, m, p, B, 1000, ctx)
    bt.step()
    bt.step()
    L = bt.state_len
    Wt = _dev(np.array(dc.cotangents(L, B)))
    names = dc.present(n, m, p)
    ref = _host(bt.data_grad_tensors(Wt, shared=names))
    per = _host(bt.data_grad_tensors(Wt))
    for off in (0, 1):
        got, clean = _layout(bt, B, Wt, L, off, 3, 0, shared=True)
        assert clean, f"offset {off}: row padding, the space before the block and the tail keep their bits"
        assert set(got) == set(names)
        for k in names:
            assert _same(got[k], ref[k]), (off, k)
    worst = max(dc.rel_err(ref[k], per[k].sum(axis=0)) for k in names)  # (what was compared is the sum over the batch)
    assert worst <= nc.TOL
    print(f"shared layout n={n}: row stride n + 3 at offsets 0 and 1 bitwise the contiguous blocks; padding untouched",
          flush=True)


def test_blocks_of_dimension_zero_are_ignored(ctx):
    n, B = 40, 2
    bt = _batch(n, 0, 0, B, 1000, ctx)
    bt.step()
    L = bt.state_len
    Wt = _dev(np.array(dc.cotangents(L, B)))
    ref = _host(bt.data_grad_tensors(Wt))
    assert set(ref) == {"Q", "c", "l_x", "u_x"}
    tq, tc = _dev(np.full((B, n, n), NAN)), _dev(np.full((B, n), NAN))
    junk = 0xdead0
    _raw(bt, Wt.data_ptr(), L, dict(Q=(tq, 0, n, n * n), c=(tc, 0, 0, n), A_ineq=(junk, 0, 1, -5), l_A_ineq=(junk, 0, 0, 1),
                                    u_A_ineq=(junk, 0, 0, 1), A_eq=(junk, 0, 0, 0), b_eq=(junk, 0, 0, -1)))
    assert _same(tq.cpu().numpy(), ref["Q"]) and _same(tc.cpu().numpy(), ref["c"])
    print("m = 0, p = 0: garbage A / C / l_A / u_A / d blocks ignored", flush=True)


# 5 ---------------------------------------------------------------------------
def _everything(g):
    return [g.state(i, w) for i in range(g.batch) for w in range(4)] + [g.batch_scalars()]


@pytest.mark.parametrize("eq_none", (False, True), ids=("ldlt", "bk"))
def test_nothing_else_moves(ctx, eq_none):
    n, m, p, B, seed0 = nc.BATCHES[0]
    a, b = (_batch(n, m, p, B, seed0, ctx, eq_none) for _ in range(2))
    L = a.state_len
    Wt = _dev(np.array(dc.cotangents(L, B)))
    names = dc.present(n, m, p)
    for k in range(3):
        before = _everything(b)
        b.data_grad_tensors(Wt, shared=names if k % 2 else ())
        for x, y in zip(before, _everything(b)):
            assert np.array_equal(x, y, equal_nan=True), "the call itself"
        a.step(I.STEP_GRAPH)
        b.step(I.STEP_GRAPH)
    assert a.last_step_graph() and b.last_step_graph()
    for x, y in zip(_everything(a), _everything(b)):
        assert np.array_equal(x, y, equal_nan=True)
    # W may be the adjoint's Out buffer: row 0 of each QP's nrhs = 2 rows, sW = sO
    ldo = nc.even(L) + 2
    sO = 2 * ldo + 4
    G = np.zeros((B, sO))
    G[:, :L] = np.array(dc.cotangents(L, B))
    G[:, ldo:ldo + L] = 1.0
    tG, tO = _dev(G), _dev(np.full((B, sO), NAN))
    b.newton_adjoint_all(tG.data_ptr(), tO.data_ptr(), 2, ldo, sO, ldo, sO)
    rows = tO[:, :L].contiguous()
    ref = _host(b.data_grad_tensors(rows))
    got = _host(b.data_grad_tensors(tO))  # (B, sO) with row stride sO: the buffer itself
    for k in ref:
        assert not np.isnan(ref[k]).any() and _same(got[k], ref[k]), k
    print(f"eq_none={eq_none}: states, scalars and graph-replayed steps bitwise unchanged; W = the adjoint's Out",
          flush=True)


# 6 ---------------------------------------------------------------------------
def test_errors(ctx):
    n, m, p, B, seed0 = nc.BATCHES[0]
    bt = _batch(n, m, p, B, seed0, ctx)
    L = bt.state_len
    Wt = _dev(np.zeros((B, L)))
    W = Wt.data_ptr()
    tq, tc = _dev(np.full((B, n, n), NAN)), _dev(np.full((B, n), NAN))
    good = dict(Q=(tq, 0, n, n * n), c=(tc, 0, 0, n))

    def invalid(g, *a):
        with pytest.raises(I.IpmzError, match="invalid argument"):
            _raw(g, *a)

    def state(g, *a):
        with pytest.raises(I.IpmzError, match="bad state"):
            _raw(g, *a)

    _raw(bt, W, L, good)
    lib = I.lib
    gr = I._QPDeviceGrad()
    assert lib.ipmz_batch_data_vjp(None, ctypes.c_void_p(W), L, ctypes.byref(gr)) == -1
    assert lib.ipmz_batch_data_vjp(bt.h, None, L, ctypes.byref(gr)) == -1
    assert lib.ipmz_batch_data_vjp(bt.h, ctypes.c_void_p(W), L, None) == -1
    invalid(bt, W, L - 1, good)                                     # sW < state_len
    invalid(bt, W, L, dict(Q=(tq, 0, n - 1, n * n)))                # row stride < n
    invalid(bt, W, L, dict(Q=(tq, 0, n, n * n - 1)))                # QP stride below the extent
    invalid(bt, W, L, dict(Q=(tq, 0, n, -n * n)))                   # negative QP stride
    invalid(bt, W, L, dict(c=(tc, 0, 0, n - 1)))                    # vector QP stride below its length
    invalid(bt, W, L, dict(c=(tc, 0, 0, -1)))
    assert np.isnan(tq.cpu().numpy()).sum() == 0                    # (only the good call wrote)
    for kw in (dict(equality_handling=I.EQ_SLACKED_SLACKS),
               dict(equality_handling=I.EQ_NAIVE_SLACKS, inequality_handling=I.INEQ_NAIVE_SLACKS)):
        e = I.Batch(n, m, p, B, ctx, **kw)
        e.generate(seed0)
        big = _dev(np.zeros((B, e.state_len)))
        invalid(e, big.data_ptr(), e.state_len, good)
    fresh = I.Batch(n, m, p, B, ctx)
    state(fresh, W, L, good)                                        # before a load
    q = nc.qp(n, m, p, seed0)
    bt.load_one(0, I.Data(q["Q"], q["c"], q["lx"], q["ux"], q["A"], q["lA"], q["uA"], q["C"], q["d"]))
    state(bt, W, L, good)                                           # between load_one and initialize
    bt.initialize()
    _raw(bt, W, L, good)
    # single QPs: the reduction and mixed precision are refused as by the adjoint pair; sW is ignored
    g = _single((n, m, p), ctx)
    one = dict(Q=(tq, 0, n, 0), c=(tc, 0, 0, 0))
    _raw(g, W, 0, one)
    g.set_reduction(I.REDUCTION_NORMAL)
    invalid(g, W, L, one)
    g.set_reduction(I.REDUCTION_AUGMENTED)
    g.set_mixed_precision(True)
    invalid(g, W, L, one)
    g.set_mixed_precision(False)
    _raw(g, W, L, one)
    print("errors: every IPMZ_ERR_INVALID / IPMZ_ERR_STATE case", flush=True)


def test_capture_needs_the_shared_workspace_first():
    """Inside a caller's graph capture the call is enqueued like any launch, but the shared matrix blocks' workspace
    cannot be allocated there: IPMZ_ERR_STATE until one call outside a capture has made it."""
    n, m, p, B, seed0 = nc.BATCHES[0]
    s = torch.cuda.Stream()
    c = I.Context(0, stream=s.cuda_stream)
    try:
        bt = _batch(n, m, p, B, seed0, c)
        bt.step()
        L = bt.state_len
        Wt = _dev(np.array(dc.cotangents(L, B)))
        ref = _host(bt.data_grad_tensors(Wt, only=["c"]))["c"]                 # (per-QP vectors: no workspace yet)
        tq, tc = _dev(np.full((n, n), NAN)), _dev(np.full((B, n), NAN))
        z = torch.zeros(8, device="cuda")

        def call(spec):
            gr = I._QPDeviceGrad()
            for name, (t, ld, sq) in spec.items():
                setattr(gr, name, t.data_ptr())
                if ld:
                    gr.ldq = ld
                setattr(gr, "s" + name, sq)
            return I.lib.ipmz_batch_data_vjp(bt.h, ctypes.c_void_p(Wt.data_ptr()), L, ctypes.byref(gr))

        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            z.add_(1.0)
            assert call(dict(Q=(tq, n, 0))) == -5                              # IPMZ_ERR_STATE
            assert b"capturing" in I.lib.ipmz_last_error()
            assert call(dict(c=(tc, 0, n))) == 0                               # no allocation: captured
        graph.replay()
        torch.cuda.synchronize()
        assert z[0].item() == 1.0 and _same(tc.cpu().numpy(), ref) and np.isnan(tq.cpu().numpy()).all()
        sh = _host(bt.data_grad_tensors(Wt, shared=["Q"], only=["Q"]))["Q"]     # outside: allocates
        graph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph2, stream=s, capture_error_mode="thread_local"):
            assert call(dict(Q=(tq, n, 0))) == 0
        graph2.replay()
        torch.cuda.synchronize()
        assert _same(tq.cpu().numpy(), sh)
        bt.close()
    finally:
        c.close()
    print("capture: refused while the workspace is missing, captured and replayed once it exists", flush=True)
