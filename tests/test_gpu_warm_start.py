"""The device warm start: ipmz_batch_set_state_device (Optimizer.set_state_tensor) against the host call
ipmz_batch_set_state per QP, its interior push and its check against their numpy restatement
(tests/warm_start_cases.py), and ipmz_amd.layer.solve_qp(warm_start=).

Comparisons with the host call are bitwise: the same doubles reach the same storage and the same evaluation runs
afterwards, so there is no tolerance to choose.  Shapes: n = 48, m = 16, p = 8 for every formulation of
tests/batch_form_cases.py (the two equality-slack ones included), n = 5, m = p = 0 for the explicit bounds of the
box-only case, batches of 5.
"""
import collections
import ctypes
import functools

import numpy as np
import pytest

import batch_form_cases as fc
import data_vjp_cases as dc
import newton_multi_cases as nc
import warm_start_cases as wc

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")
layer = pytest.importorskip("ipmz_amd.layer")

NAN = float("nan")
B = wc.BATCH
CASES = [(f, wc.SHAPE) for f in fc.FORMS] + [(f, wc.BOX_SHAPE) for f in wc.BOX_FORMS]
CASE_IDS = [f if s == wc.SHAPE else f + "-boxonly" for f, s in CASES]
Ref = collections.namedtuple("Ref", "V snap nxt")


@functools.lru_cache(maxsize=None)
def shared_ctx():
    return I.Context(0)


def make(form, shape, steps=3, batch=B, seed=wc.SEED0, ctx=None):
    n, m, p = shape
    bt = I.Batch(n, m, p, batch, ctx or shared_ctx(), **fc.FORMS[form].kw)
    bt.generate(seed)
    for _ in range(steps):
        bt.step()
    return bt


def dev(a):
    t = torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared references are read-only)
    torch.cuda.synchronize()
    return t


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def snapshot(bt, batch=B):
    """All four states of every QP (iterate, affine direction, direction, residuals), then the scalar blocks."""
    return [bt.state(q, w) for q in range(batch) for w in range(4)] + [bt.batch_scalars()]


def follow(bt, steps=2, batch=B):
    out = []
    for _ in range(steps):
        bt.step()
        out += [bt.state(q, 0) for q in range(batch)]
    return out


def assert_same(got, ref, what):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert same(a, b), f"{what}: item {i} differs"


@functools.lru_cache(maxsize=None)
def base(form, shape):
    """A solver after three steps that never gets the call: its iterates (the rows the tests start from), its
    snapshot and its next two steps.  Made once per case and shared, never modified."""
    bt = make(form, shape)
    try:
        snap = snapshot(bt)
        V = bt.state_tensor().cpu().numpy()
        assert all(same(V[q], snap[4 * q]) for q in range(B))
        V.setflags(write=False)
        return Ref(V, snap, follow(bt))
    finally:
        bt.close()


def rows(form, shape):
    """The rows the warm start is given: base's iterates, perturbed and interior."""
    lay = wc.layout(form, *shape)
    W = wc.perturbed(base(form, shape).V, lay, wc.qp_bounds(shape))
    assert wc.first_offender(W, lay, 0.0, wc.qp_bounds(shape)) is None
    return lay, W


@functools.lru_cache(maxsize=None)
def host_ref(form, shape):
    """The twin set through the host call, one QP at a time: its snapshot and its next two steps."""
    _, W = rows(form, shape)
    bt = make(form, shape)
    try:
        for q in range(B):
            bt.set_state(q, W[q])
        W.setflags(write=False)
        return Ref(W, snapshot(bt), follow(bt))
    finally:
        bt.close()


def assert_qp_matches(bt, ref, q, what):
    """States 0 and 3 and the scalar block of QP q against a Ref's snapshot."""
    assert same(bt.state(q, 0), ref.snap[4 * q]), f"{what}: iterate of QP {q}"
    assert same(bt.state(q, 3), ref.snap[4 * q + 3]), f"{what}: residuals of QP {q}"
    assert same(bt.batch_scalars()[q], ref.snap[-1][q]), f"{what}: scalars of QP {q}"


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("form,shape", CASES, ids=CASE_IDS)
def test_parity_with_the_host_call(form, shape):
    ref = host_ref(form, shape)
    bt = make(form, shape)
    gen = bt._generation
    bt.set_state_tensor(dev(ref.V), check=False)
    assert bt._generation == gen + 1
    assert_same(snapshot(bt), ref.snap, "after set_state_tensor")
    assert_same(follow(bt), ref.nxt, "the next two steps")
    bt.close()


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("form,shape", CASES, ids=CASE_IDS)
def test_round_trip_keeps_the_bits(form, shape):
    bt = make(form, shape)
    V = bt.state_tensor().clone()
    bt.set_state_tensor(V)  # (checked: an iterate of the solver's own is interior)
    assert torch.equal(bt.state_tensor().view(torch.int64), V.view(torch.int64))
    for q in range(B):
        assert same(bt.state(q, 0), base(form, shape).V[q])
    bt.close()


@pytest.mark.parametrize("form", list(fc.SOLVE))
def test_converged_iterate_set_with_floor_zero_is_still_converged(form):
    n, m, p = wc.SHAPE
    bt = I.Batch(n, m, p, B, shared_ctx(), **fc.FORMS[form].kw)
    bt.generate(fc.SOLVE[form][0])
    its, conv = bt.solve_all(100)
    assert conv == B and its > 0, (its, conv)
    V = bt.state_tensor().clone()
    bt.set_state_tensor(V, floor=0.0)
    assert bt.solve_all(100) == (0, B)
    assert torch.equal(bt.state_tensor().view(torch.int64), V.view(torch.int64))
    bt.close()


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["box", "sl", "eqss", "naiveeq"])
def test_take(form):
    shape = wc.SHAPE
    ref, b0 = host_ref(form, shape), base(form, shape)
    mask = np.array([1, 0, 1, 0, 0], dtype=bool)
    W = np.array(ref.V)
    W[~mask] = NAN  # rows of QPs that are not taken are never read: the check passes
    bt = make(form, shape)
    bt.set_state_tensor(dev(W), take=dev(mask))
    for q in range(B):
        if mask[q]:
            assert_qp_matches(bt, ref, q, "taken")
        else:
            assert same(bt.state(q, 0), b0.V[q]), f"QP {q} was not taken"
    before = [bt.state(q, 0) for q in range(B)]
    bt.set_state_tensor(dev(np.full_like(W, NAN)), take=torch.zeros(B, dtype=torch.int64, device="cuda"))
    assert_same([bt.state(q, 0) for q in range(B)], before, "take all zero")
    with pytest.raises(ValueError):
        bt.set_state_tensor(dev(W), take=torch.ones(B, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        bt.set_state_tensor(dev(W), take=torch.ones(B + 1, dtype=torch.bool, device="cuda"))
    bt.close()


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["box", "eqss", "naiveeq"])
def test_padded_rows_at_an_odd_offset(form):
    """Row stride state_len + 3 with NaN between the rows, the first row 8 bytes off a 16-byte boundary."""
    shape = wc.SHAPE
    ref = host_ref(form, shape)
    L = ref.V.shape[1]
    flat = torch.full((1 + B * (L + 3),), NAN, dtype=torch.float64, device="cuda")
    view = flat[1:].as_strided((B, L + 3), (L + 3, 1))
    assert view.data_ptr() % 16 == 8
    view[:, :L] = dev(ref.V)
    bt = make(form, shape)
    bt.set_state_tensor(view)
    assert_same(snapshot(bt), ref.snap, "padded rows")
    bt.close()


@pytest.mark.parametrize("form", ["box", "eqss"])
def test_a_solver_of_one_qp(form):
    n, m, p = wc.SHAPE
    lay = wc.layout(form, n, m, p)
    pair = []
    for _ in range(2):
        o = I.Optimizer(n, m, p, shared_ctx(), **fc.FORMS[form].kw)
        o.generate(wc.SEED0)
        for _ in range(3):
            o.step()
        pair.append(o)
    a, b = pair
    V = a.state_tensor()
    assert V.shape == (1, lay.L) and same(V.cpu().numpy()[0], a.vars())
    W = wc.perturbed(V.cpu().numpy(), lay, wc.qp_bounds(wc.SHAPE, 1))
    a.set_state_tensor(dev(np.concatenate([W, np.full((1, 2), NAN)], axis=1)))  # (the stride of one row means nothing)
    b.set_vars(W[0])
    assert same(a.vars(), b.vars()) and same(a.vars(), W[0]) and same(a.residuals(), b.residuals())
    sa, sb = a.scalars(), b.scalars()
    assert all(same(np.array(sa[k]), np.array(sb[k])) for k in sa)
    a.step(), b.step()
    assert same(a.vars(), b.vars())
    a.close(), b.close()


def test_looped_grid_dimension():
    """70 000 QPs of n = 2: the QP index runs past the grid's second dimension (4096) many times over."""
    big, shape = 70000, (2, 0, 0)
    lay = wc.layout("box", *shape)
    pm = lay.kind == wc.PUSHED
    bt = make("box", shape, steps=1, batch=big, seed=3)
    twin = make("box", shape, steps=1, batch=big, seed=3)
    V = bt.state_tensor().cpu().numpy()
    W = V.copy()  # x stays where it is (inside its bounds), the slacks and multipliers move
    W[:, pm] *= 1.0 + 0.25 * np.random.default_rng(5).uniform(0.0, 1.0, (big, int(pm.sum())))
    W[::7, np.nonzero(pm)[0][0]] *= 1e-9  # (below the floor)
    take = np.arange(big) % 3 != 0
    floor = 1e-6
    bt.set_state_tensor(dev(W), take=dev(take), floor=floor)
    want = np.where(take[:, None], wc.push(W, lay, floor), V)
    got = bt.state_tensor().cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    sc = bt.batch_scalars()
    for q in (1, 4097, big - 2):
        assert take[q]
        twin.set_state(q, want[q])
        assert same(bt.state(q, 3), twin.state(q, 3)) and same(sc[q], twin.batch_scalars()[q]), q
    bad = np.array(W)
    bad[65537, lay.offsets["x"]] = NAN
    bad[big - 1, lay.L - 1] = NAN  # (not taken: 69999 % 3 == 0)
    bad[65539, lay.L - 1] = -1.0   # cured by the push
    with pytest.raises(I.IpmzError, match=r"QP 65537\b.*index %d\b" % lay.offsets["x"]):
        bt.set_state_tensor(dev(bad), take=dev(take), floor=floor)
    assert np.array_equal(bits(bt.state_tensor().cpu().numpy()), bits(want))
    bt.close(), twin.close()


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("floor", [1e-6, 1.0])
@pytest.mark.parametrize("form,shape", [c for c in CASES if c[0] != "sl"], ids=[i for i in CASE_IDS if not i.startswith("sl")])
def test_push(form, shape, floor):
    lay, W = rows(form, shape)
    W = np.array(W)
    pk = np.nonzero(lay.kind == wc.PUSHED)[0]
    if pk.size:
        W[0, pk[0]], W[1, pk[min(3, pk.size - 1)]], W[2, pk[-1]], W[4, pk[pk.size // 2]] = -1.0, 0.0, 1e-9, 0.5
    want = wc.push(W, lay, floor)
    assert not pk.size or (want != W).sum() >= 3
    keep = lay.kind != wc.PUSHED
    assert same(want[:, keep], W[:, keep])  # x, s and the free duals are never pushed
    bt = make(form, shape)
    bt.set_state_tensor(dev(W), floor=floor)  # (checked: the push cures zero and negative)
    assert np.array_equal(bits(bt.state_tensor().cpu().numpy()), bits(want))
    twin = make(form, shape)
    for q in range(B):
        twin.set_state(q, want[q])
    assert_same(snapshot(bt), snapshot(twin), "against the host call with the pushed rows")
    bt.close(), twin.close()


@pytest.mark.parametrize("shape", [wc.SHAPE, wc.BOX_SHAPE], ids=["S1", "boxonly"])
def test_push_is_refused_under_slacks(shape):
    ref = host_ref("sl", shape)
    bt = make("sl", shape)
    before = snapshot(bt)
    for check in (True, False):
        with pytest.raises(I.IpmzError, match="invalid argument.*floor > 0.*Slacks"):
            bt.set_state_tensor(dev(ref.V), floor=1e-6, check=check)
    assert_same(snapshot(bt), before, "after the refusals")
    bt.set_state_tensor(dev(ref.V), floor=0.0)
    assert_same(snapshot(bt), ref.snap, "floor 0")
    bt.close()


# 6 ---------------------------------------------------------------------------
def _poisoned(W, lay, cols, value):
    """Several (QP, index) pairs, the smallest neither first in the list nor in the first QP."""
    W = np.array(W)
    ks = sorted({int(cols[0]), int(cols[cols.size // 2]), int(cols[-1])})
    pairs = [(3, ks[0]), (1, ks[-1]), (1, ks[len(ks) // 2]), (4, ks[0])]
    for q, k in pairs:
        W[q, k] = value(q, k) if callable(value) else value
    return W


@pytest.mark.parametrize("form,shape", CASES, ids=CASE_IDS)
def test_check_names_the_first_violation_and_writes_nothing(form, shape):
    lay, W = rows(form, shape)
    bounds = wc.qp_bounds(shape)
    b0 = base(form, shape)
    classes = []
    pk = np.nonzero(lay.kind == wc.PUSHED)[0]
    if pk.size:
        classes += [("zero", pk, 0.0), ("negative", pk, -0.25), ("NaN in a pushed slot", pk, NAN)]
    fk = np.nonzero(lay.kind == wc.FREE)[0]
    if fk.size:
        classes += [("NaN in a free slot", fk, NAN)]
    xk = np.nonzero(lay.kind == wc.XBOUND)[0]
    if xk.size:
        classes += [("x on its lower bound", xk, lambda q, k: bounds["lx"][q, lay.idx[k]]),
                    ("x on its upper bound", xk, lambda q, k: bounds["ux"][q, lay.idx[k]]), ("NaN in x", xk, NAN)]
    sk = np.nonzero(lay.kind == wc.SBOUND)[0]
    if sk.size:
        classes += [("s on its upper bound", sk, lambda q, k: bounds["uA"][q, lay.idx[k]])]
    assert classes
    bt = make(form, shape)
    for what, cols, value in classes:
        bad = _poisoned(W, lay, cols, value)
        for take in (None, np.array([1, 0, 1, 1, 1], dtype=np.int32)):
            q, k = wc.first_offender(bad, lay, 0.0, bounds, take)
            assert q == (1 if take is None else 3)
            with pytest.raises(I.IpmzError, match=r"invalid argument.*QP %d\b.*index %d\b" % (q, k)) as e:
                bt.set_state_tensor(dev(bad), take=None if take is None else dev(take))
            print(f"{form} {what}: {e.value}", flush=True)
        assert_same(snapshot(bt), b0.snap, "after the refusal of " + what)
    assert_same(follow(bt), b0.nxt, "stepping after the refusals")
    bt.close()


# 7 ---------------------------------------------------------------------------
def test_refusals():
    form, shape = "box", wc.SHAPE
    n, m, p = shape
    ref = host_ref(form, shape)
    L = ref.V.shape[1]
    bt = make(form, shape)
    before = snapshot(bt)
    Vt = dev(ref.V)
    vp = ctypes.c_void_p(Vt.data_ptr())

    def call(h, src, ld, floor=0.0, flags=0):
        return I._check(I.lib.ipmz_batch_set_state_device(h, src, ld, None, floor, flags), "ipmz_batch_set_state_device")

    with pytest.raises(I.IpmzError, match="invalid argument.*null"):
        call(bt.h, None, L)
    with pytest.raises(I.IpmzError, match="invalid argument.*row stride"):
        call(bt.h, vp, L - 1)
    with pytest.raises(I.IpmzError, match="invalid argument.*row stride"):
        bt.set_state_tensor(Vt[:, :L - 1])
    for flags in (2, 3, -2):
        with pytest.raises(I.IpmzError, match="invalid argument.*flag"):
            call(bt.h, vp, L, flags=flags)
    for floor in (-1e-300, -1.0, NAN, float("inf"), -float("inf")):
        for flags in (0, I.SET_STATE_UNCHECKED):
            with pytest.raises(I.IpmzError, match="invalid argument.*floor"):
                call(bt.h, vp, L, floor=floor, flags=flags)
    for bad in (Vt.float(), Vt[0], Vt[:B - 1], ref.V, Vt.t().contiguous().t()):
        with pytest.raises(ValueError):
            bt.set_state_tensor(bad)
    assert_same(snapshot(bt), before, "after the refusals")
    bt.close()
    # before a load, and between a load and initialize
    fresh = I.Batch(n, m, p, B, shared_ctx())
    with pytest.raises(I.IpmzError, match="bad state.*load"):
        call(fresh.h, vp, L)
    fresh.generate(wc.SEED0)
    call(fresh.h, vp, L)
    q = fc.qp(shape, wc.SEED0)
    fresh.load_one(0, I.Data(**{k: q[dc.KEYS[k]] for k in dc.NAMES}))
    for flags in (0, I.SET_STATE_UNCHECKED):
        with pytest.raises(I.IpmzError, match="bad state.*load"):
            call(fresh.h, vp, L, flags=flags)
    fresh.close()


@pytest.mark.parametrize("form", ["box", "eqss"])
def test_unchecked_form_in_a_graph_capture(form):
    shape = wc.SHAPE
    ref = host_ref(form, shape)
    s = torch.cuda.Stream()
    c = I.Context(0, stream=s.cuda_stream)
    try:
        bt = make(form, shape, ctx=c)
        before = snapshot(bt)
        Vt = dev(ref.V)
        z = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            z.add_(1.0)
            with pytest.raises(I.IpmzError, match="bad state.*capturing"):
                bt.set_state_tensor(Vt)  # the checked form waits for its verdict
            bt.set_state_tensor(Vt, check=False)
        assert_same(snapshot(bt), before, "captured, not replayed yet")
        graph.replay()
        torch.cuda.synchronize()
        assert z[0].item() == 1.0
        assert_same(snapshot(bt), ref.snap, "after the replay")
        assert_same(follow(bt), ref.nxt, "the next two steps")
        bt.close()
    finally:
        c.close()


# 8 ---------------------------------------------------------------------------
def _leaf(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda().requires_grad_(True)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("form", ["box", "naive"])
def test_layer_warm_start(form):
    """solve_qp cold, then on c perturbed by a relative 1e-3 from the previous iterate with warm_floor = 1e-4.
    The warm solve's answer is judged by numpy from the data alone: the stationarity and primal-feasibility rows
    of the residual (every row but the complementarity ones) below 1e-7 in the 2-norm -- ten times the solver's own
    stop rule res < 1e-8 on the whole residual, the margin for numpy's summation order on these O(1) sums of at
    most 48 terms."""
    n, m, p = wc.SHAPE
    qs = [fc.qp(wc.SHAPE, 1000 + i) for i in range(B)]
    data = {k: np.stack([q[dc.KEYS[k]] for q in qs]) for k in dc.NAMES}
    bt = I.Batch(n, m, p, B, shared_ctx(), **fc.FORMS[form].kw)
    cold = {k: dev(a) for k, a in data.items()}
    layer.solve_qp(bt, **cold)
    prev = bt.state_tensor().clone()
    c2 = data["c"] * (1.0 + 1e-3 * np.random.default_rng(21).uniform(-1.0, 1.0, data["c"].shape))
    leaves = {k: _leaf(c2 if k == "c" else a) for k, a in data.items()}
    warm = prev.clone().requires_grad_(True)  # (it takes no gradient whatever it asks for)
    x = layer.solve_qp(bt, **leaves, warm_start=warm, warm_floor=1e-4, strict=True)
    sc = bt.batch_scalars()
    assert np.all(sc[:, I.SC["converged"]] == 1.0), sc[:, I.SC["converged"]]
    order, sz, off, L = dc.form_offsets(form, n, m, p)
    feas = np.concatenate([np.arange(off[s], off[s] + sz[s]) for s in order if s not in ("g", "h", "y", "z")])
    worst = 0.0
    for i in range(B):
        v = bt.state(i)
        assert same(x[i].detach().cpu().numpy(), v[:n])
        r = dc.residuals_form(form, dict(qs[i], c=c2[i]), v, 0.0)
        worst = max(worst, float(np.linalg.norm(r[feas])))
    print(f"{form}: worst |stationarity, primal feasibility|_2 after the warm solve {worst:.3e}", flush=True)
    assert worst < 1e-7
    # backward reads the final iterate: bit for bit solution_vjp on the same solver state with the same cotangent
    G = dev(np.random.default_rng(77).standard_normal((B, n)))
    gen = bt._generation
    grads, _ = layer.solution_vjp(bt, G[:, None, :])
    assert bt._generation == gen
    (G * x).sum().backward()
    torch.cuda.synchronize()
    assert warm.grad is None
    for k, t in leaves.items():
        assert t.grad is not None, k
        assert torch.equal(t.grad.contiguous().view(torch.int64), grads[k][:, 0].contiguous().view(torch.int64)), k
    # a set_state_tensor between forward and backward moves the iterate backward would read
    x2 = layer.solve_qp(bt, **leaves, warm_start=prev, warm_floor=1e-4)
    bt.set_state_tensor(prev, floor=1e-4)
    with pytest.raises(I.IpmzError, match="changed between forward and backward"):
        (G * x2).sum().backward()
    # the check is the layer's too: a row that is no interior iterate is refused before the solve
    poisoned = prev.clone()
    poisoned[2, 0] = NAN
    with pytest.raises(I.IpmzError, match=r"QP 2\b.*index 0\b"):
        layer.solve_qp(bt, **leaves, warm_start=poisoned, warm_floor=1e-4)
    bt.close()
