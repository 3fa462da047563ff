"""The device-resident load and read-back: ipmz_batch_load_device
(Optimizer.load_tensors) against the host load (load_one x B + initialize), and
ipmz_batch_copy_state (state_tensor) against state(q, which).

Every comparison is bitwise: the same doubles reach the same storage and the
same kernels run afterwards, so there is no tolerance to choose.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

NAN = float("nan")
SEED0 = 4200
# (n, m, p, B)
SHAPES = [
    (12, 5, 3, 3),     # n not a multiple of 8: the padding columns [n, ldn) are live
    (48, 16, 8, 3),    # the fused-step batch with the kept matrix K0
    (130, 40, 22, 3),  # rows cross a 256-thread block
    (40, 0, 0, 2),     # absent blocks, passed as None
    (300, 40, 20, 1),  # a batch of one: no K0
    (1040, 8, 4, 2),   # above IPMZ_FUSED_NMAX
]
MID = (48, 16, 8, 3)
FORMS = {
    "default": {},
    "eq_none": dict(equality_handling=I.EQ_NONE),
    "eq_penalty": dict(equality_handling=I.EQ_PENALTY),
    "ineq_slacks": dict(inequality_handling=I.INEQ_SLACKS),
    "eq_slacked_slacks": dict(equality_handling=I.EQ_SLACKED_SLACKS),
    "naive_slacks": dict(equality_handling=I.EQ_NAIVE_SLACKS, inequality_handling=I.INEQ_NAIVE_SLACKS),
}
NAMES = ("Q", "c", "l_x", "u_x", "A_ineq", "l_A_ineq", "u_A_ineq", "A_eq", "b_eq")
KEYS = dict(Q="Q", c="c", l_x="lx", u_x="ux", A_ineq="A", l_A_ineq="lA", u_A_ineq="uA", A_eq="C", b_eq="d")


def sid(s):
    return "n%d_m%d_p%d_B%d" % s


@functools.lru_cache(maxsize=None)
def shared_ctx():
    return I.Context(0)


@pytest.fixture(scope="module")
def ctx():
    return shared_ctx()


@functools.lru_cache(maxsize=None)
def host_data(shape, seed0=SEED0):
    """Data's blocks of every QP stacked along a leading batch axis (numpy, read-only)."""
    n, m, p, B = shape
    qs = [oracle.gen_qp(n, m, p, seed0 + q) for q in range(B)]
    out = {name: np.stack([q[KEYS[name]] for q in qs]) for name in NAMES}
    for a in out.values():
        a.setflags(write=False)
    return out


def present(shape, name):
    n, m, p, _ = shape
    return not ((m == 0 and name in ("A_ineq", "l_A_ineq", "u_A_ineq")) or (p == 0 and name in ("A_eq", "b_eq")))


def cuda_blocks(shape, data):
    """The blocks as contiguous CUDA tensors; absent blocks (dimension 0) as None."""
    return {k: (torch.from_numpy(np.array(v)).cuda() if present(shape, k) else None) for k, v in data.items()}


def make(ctx, shape, form):
    n, m, p, B = shape
    return I.Batch(n, m, p, B, ctx, **FORMS[form])


def host_load(g, shape, data):
    for q in range(shape[3]):
        g.load_one(q, I.Data(**{k: v[q] for k, v in data.items()}))
    g.initialize()


def snapshot(g, B):
    """What the comparisons look at: the iterate and the residuals of every QP, the scalar blocks, the KKT matrices."""
    return ([g.state(q, w) for q in range(B) for w in (0, 3)] + [g.batch_scalars()] + [g.kkt_of(q) for q in range(B)])


def stepped(g, B, steps=3):
    first = snapshot(g, B)
    for _ in range(steps):
        g.step()
    return first, snapshot(g, B)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, ref, what):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{what}: item {i} differs"


@functools.lru_cache(maxsize=None)
def host_reference(shape, form):
    """The host-loaded twin, before and after three steps: made once per (shape, formulation) and shared."""
    g = make(shared_ctx(), shape, form)
    try:
        host_load(g, shape, host_data(shape))
        return stepped(g, shape[3])
    finally:
        g.close()


def check_against_host(g, shape, form, what):
    ref0, ref3 = host_reference(shape, form)
    got0, got3 = stepped(g, shape[3])
    assert_same(got0, ref0, what + ", after the load")
    assert_same(got3, ref3, what + ", after three steps")


CASES = [(s, "default") for s in SHAPES] + [(MID, f) for f in FORMS if f != "default"]
CASE_IDS = [sid(s) + "-" + f for s, f in CASES]


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form", CASES, ids=CASE_IDS)
def test_equals_host_load(ctx, shape, form):
    g = make(ctx, shape, form)
    g.load_tensors(**cuda_blocks(shape, host_data(shape)))
    check_against_host(g, shape, form, "load_tensors")
    g.close()


@pytest.mark.parametrize("form", [dict(inequality_handling=I.INEQ_NAIVE_SLACKS), FORMS["naive_slacks"]],
                         ids=["ineq_naive", "eq_ineq_naive"])
def test_naive_slacks_residual_norm_is_the_norm_of_the_residuals(ctx, form):
    """IPMZ_SC_RES after fused steps is the 2-norm of the residual vector the solver returns.  (NaiveSlacks has
    N = n + 2m + p KKT rows but n + m + p residual elements; the fused evaluation once walked N of them, and the
    twins of test_equals_host_load disagreed in this scalar.)  Only the order of the L = state_len additions
    differs between the two sums, each addition rounding by at most 2^-53 of the running sum: L * 2^-53 < 1e-13
    relative at L <= 400, bounded here by 1e-12."""
    n, m, p, B = MID
    g = I.Batch(n, m, p, B, ctx, **form)
    g.load_tensors(**cuda_blocks(MID, host_data(MID)))
    for _ in range(3):
        g.step()
    assert g.state_len <= 400
    res = g.batch_scalars()[:, I.SC["res"]]
    for q in range(B):
        want = float(np.linalg.norm(g.state(q, 3)))
        print(f"QP {q}: res {res[q]!r}, |r|_2 {want!r}")
        assert abs(res[q] - want) <= 1e-12 * want
    g.close()


# 2 ---------------------------------------------------------------------------
def embed(a, lead, offset, row_pad, qp_pad):
    """a (B, rows, cols) or (B, cols) inside a NaN-filled flat buffer: `offset` elements in front, rows row_pad and
    QPs a further qp_pad elements apart."""
    a = np.asarray(a)
    B, cols = a.shape[0], a.shape[-1]
    if a.ndim == 3:
        ld = cols + row_pad
        sq = a.shape[1] * ld + qp_pad
        strides = (sq, ld, 1)
    else:
        sq = cols + row_pad + qp_pad
        strides = (sq, 1)
    flat = torch.full((offset + B * sq + lead,), NAN, dtype=torch.float64, device="cuda")
    view = flat[offset:].as_strided(a.shape, strides)
    view.copy_(torch.from_numpy(np.array(a)).cuda())
    return view


@pytest.mark.parametrize("offset", [1, 0], ids=["scalar_path", "vector_path"])
@pytest.mark.parametrize("shape,form", [(s, "default") for s in SHAPES] + [(MID, "eq_slacked_slacks")],
                         ids=[sid(s) + "-default" for s in SHAPES] + [sid(MID) + "-eq_slacked_slacks"])
def test_strided_blocks(ctx, shape, form, offset):
    """The data inside larger NaN-filled buffers: padding is never read (a NaN bound would be refused, a NaN entry
    would show in the states), and the element-wise copy (pointer 8 bytes off a 16-byte boundary, odd strides)
    agrees with the 16-byte one (aligned pointer, even strides, still padded)."""
    data = host_data(shape)
    blocks = {}
    for k, v in data.items():
        if not present(shape, k):
            blocks[k] = None
            continue
        # offset 1: odd row and QP strides; offset 0: both even
        row_pad = 3 if offset else 4
        n_el = v.shape[-1] * (v.shape[1] if v.ndim == 3 else 1)
        qp_pad = 5 if offset else 6
        t = embed(v, 8, offset, row_pad, qp_pad)
        assert t.data_ptr() % 16 == 8 * offset
        assert t.stride(0) > n_el and (v.ndim == 2 or t.stride(1) > v.shape[-1])
        blocks[k] = t
    g = make(ctx, shape, form)
    g.load_tensors(**blocks)
    check_against_host(g, shape, form, "strided load_tensors")
    g.close()


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["2d", "expanded"])
def test_shared_blocks(ctx, how):
    """Q, A_ineq, A_eq given once for the batch equal the same matrices repeated B times."""
    shape = MID
    n, m, p, B = shape
    data = dict(host_data(shape))
    for k in ("Q", "A_ineq", "A_eq"):
        data[k] = np.repeat(data[k][:1], B, axis=0)
    ref = make(ctx, shape, "default")
    ref.load_tensors(**cuda_blocks(shape, data))
    want = stepped(ref, B)
    ref.close()
    blocks = cuda_blocks(shape, data)
    for k in ("Q", "A_ineq", "A_eq"):
        one = blocks[k][0].clone()
        blocks[k] = one if how == "2d" else one.unsqueeze(0).expand(B, -1, -1)
    g = make(ctx, shape, "default")
    g.load_tensors(**blocks)
    got = stepped(g, B)
    g.close()
    assert_same(got[0], want[0], "shared blocks, after the load")
    assert_same(got[1], want[1], "shared blocks, after three steps")
    # and the repeated form is the host load of the repeated data
    h = make(ctx, shape, "default")
    host_load(h, shape, data)
    assert_same(stepped(h, B)[1], want[1], "repeated blocks vs the host load")
    h.close()


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "eq_slacked_slacks"])
def test_partial_reload(ctx, form):
    shape = MID
    B = shape[3]
    data = dict(host_data(shape))
    other = host_data(shape, SEED0 + 100)
    g = make(ctx, shape, form)
    g.load_tensors(**cuda_blocks(shape, data))
    g.step()
    g.step()
    c2, d2 = torch.from_numpy(np.array(other["c"])).cuda(), torch.from_numpy(np.array(other["b_eq"])).cuda()
    g.load_tensors(c=c2, b_eq=d2)
    got = stepped(g, B)
    g.close()
    data["c"], data["b_eq"] = other["c"], other["b_eq"]
    fresh = make(ctx, shape, form)
    host_load(fresh, shape, data)
    want = stepped(fresh, B)
    fresh.close()
    assert_same(got[0], want[0], "partial re-load")
    assert_same(got[1], want[1], "partial re-load, after three steps")


def test_partial_load_needs_held_blocks(ctx):
    shape = MID
    data = host_data(shape)
    c2, d2 = torch.from_numpy(np.array(data["c"])).cuda(), torch.from_numpy(np.array(data["b_eq"])).cuda()
    g = make(ctx, shape, "default")
    with pytest.raises(I.IpmzError, match="bad state.*never loaded"):
        g.load_tensors(c=c2, b_eq=d2)
    with pytest.raises(I.IpmzError, match="bad state"):
        g.step()  # still not loaded
    g.generate(77)
    g.load_tensors(c=c2, b_eq=d2)  # generate filled every block
    assert np.array_equal(g.state_tensor(0).cpu().numpy()[1], g.state(1, 0))
    g.step()
    g.close()


# 5 ---------------------------------------------------------------------------
def test_validation_refuses_and_writes_nothing(ctx):
    shape = MID
    n, m, p, B = shape
    data = host_data(shape)
    g, twin = make(ctx, shape, "default"), make(ctx, shape, "default")
    for s in (g, twin):
        s.load_tensors(**cuda_blocks(shape, data))
        s.step()
        s.step()
    other = host_data(shape, SEED0 + 100)  # what a refused load must not leave behind

    def attempt(match, **plant):
        blocks = cuda_blocks(shape, other)
        for name, edits in plant.items():
            for (q, k), v in edits:
                blocks[name][q, k] = v if v is not None else blocks[dict(l_x="u_x", l_A_ineq="u_A_ineq")[name]][q, k]
        with pytest.raises(I.IpmzError, match=match):
            g.load_tensors(**blocks)

    attempt(r"invalid argument.*QP 2: l_x < u_x violated at 5", l_x=[((2, 5), None)])  # l_x == u_x
    attempt(r"invalid argument.*QP 1: l_A <= u_A violated at 3", l_A_ineq=[((1, 3), 7.0)])  # l_A > u_A
    attempt(r"invalid argument.*QP 0: l_x < u_x violated at 7", u_x=[((0, 7), NAN)])
    # two at once: the smaller (QP, x before A, index) is the one named
    attempt(r"QP 1: l_A <= u_A violated at 3", l_x=[((2, 5), None)], l_A_ineq=[((1, 3), 7.0)])
    attempt(r"QP 1: l_x < u_x violated at 40", l_x=[((1, 40), None), ((1, 41), None)], l_A_ineq=[((1, 0), 7.0)])
    # a supplied side is checked against the side the solver holds
    with pytest.raises(I.IpmzError, match=r"invalid argument.*QP 0: l_x < u_x violated at 0"):
        g.load_tensors(l_x=torch.full((B, n), 5.0, dtype=torch.float64, device="cuda"))
    # the refused calls wrote nothing: the solver is where its twin is
    assert_same(snapshot(g, B), snapshot(twin, B), "after refused loads")
    assert_same(stepped(g, B)[1], stepped(twin, B)[1], "three steps after refused loads")
    # l_A == u_A is allowed
    blocks = cuda_blocks(shape, other)
    blocks["l_A_ineq"][0, 2] = blocks["u_A_ineq"][0, 2]
    g.load_tensors(**blocks)
    g.step()
    g.close()
    twin.close()


def _raw_load(g, d):
    return I._check(I.lib.ipmz_batch_load_device(g.h, ctypes.byref(d)), "ipmz_batch_load_device")


def test_bad_strides_are_invalid(ctx):
    shape = MID
    n, m, p, B = shape
    t = cuda_blocks(shape, host_data(shape))

    def full():
        d = I._QPDeviceData()
        d.Q, d.ldq, d.sQ = t["Q"].data_ptr(), n, n * n
        d.A, d.lda, d.sA = t["A_ineq"].data_ptr(), n, m * n
        d.C, d.ldc, d.sC = t["A_eq"].data_ptr(), n, p * n
        d.c, d.l_x, d.u_x, d.sc, d.slx, d.sux = t["c"].data_ptr(), t["l_x"].data_ptr(), t["u_x"].data_ptr(), n, n, n
        d.l_A, d.u_A, d.slA, d.suA = t["l_A_ineq"].data_ptr(), t["u_A_ineq"].data_ptr(), m, m
        d.d, d.sd = t["b_eq"].data_ptr(), p
        return d

    g = make(ctx, shape, "default")
    g.generate(3)
    before = snapshot(g, B)
    for field, value in [("ldq", n - 1), ("lda", n - 1), ("ldc", 0), ("sQ", -1), ("sc", -n), ("sd", -1), ("lda", -n),
                         ("sQ", n * n - 1), ("sA", 1), ("sux", n - 1)]:
        d = full()
        setattr(d, field, value)
        with pytest.raises(I.IpmzError, match="invalid argument"):
            _raw_load(g, d)
    with pytest.raises(I.IpmzError, match="invalid argument"):
        I._check(I.lib.ipmz_batch_load_device(g.h, None), "ipmz_batch_load_device")
    with pytest.raises(I.IpmzError, match="invalid argument"):
        I._check(I.lib.ipmz_batch_load_device(None, ctypes.byref(full())), "ipmz_batch_load_device")
    assert_same(snapshot(g, B), before, "after refused strides")
    _raw_load(g, full())  # and the untampered description loads
    ref0, _ = host_reference(shape, "default")
    assert_same(snapshot(g, B), ref0, "raw descriptor load")
    g.close()


def test_tensors_on_the_wrong_device_or_type(ctx):
    shape = MID
    blocks = cuda_blocks(shape, host_data(shape))
    g = make(ctx, shape, "default")
    with pytest.raises(ValueError, match="context is on cuda"):
        g.load_tensors(**{**blocks, "c": blocks["c"].cpu()})
    with pytest.raises(ValueError, match="float64"):
        g.load_tensors(**{**blocks, "c": blocks["c"].float()})
    g.close()


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_state_tensor_equals_state(ctx, form):
    n, m, p, B = MID
    g = make(ctx, MID, form)
    g.generate(11)
    g.step()
    g.step()
    L = g.state_len
    for which in range(4):
        t = g.state_tensor(which)
        assert t.shape == (B, L) and t.dtype == torch.float64 and t.is_cuda
        got = t.cpu().numpy()
        for q in range(B):
            assert np.array_equal(bits(got[q]), bits(g.state(q, which))), (form, which, q)
    # a wider destination keeps its tail
    big = torch.full((B, L + 6), NAN, dtype=torch.float64, device="cuda")
    r = g.state_tensor(3, out=big)
    assert r.data_ptr() == big.data_ptr() and r.shape == (B, L)
    h = big.cpu().numpy()
    assert np.isnan(h[:, L:]).all()
    for q in range(B):
        assert np.array_equal(bits(h[q, :L]), bits(g.state(q, 3)))
    x = g.solution_tensor()
    assert x.shape == (B, n) and np.array_equal(bits(x.cpu().numpy()[2]), bits(g.state(2, 0)[:n]))
    g.close()


def test_state_tensor_of_a_single_qp(ctx):
    g = I.Optimizer(48, 16, 8, ctx, equality_handling=I.EQ_SLACKED_SLACKS)
    g.generate(5)
    g.step()
    for which, ref in ((0, g.vars()), (1, g.daff()), (2, g.dir()), (3, g.residuals())):
        t = g.state_tensor(which)
        assert t.shape == (1, g.state_len) and np.array_equal(bits(t.cpu().numpy()[0]), bits(ref))
    g.close()


def test_state_tensor_errors(ctx):
    n, m, p, B = MID
    g = make(ctx, MID, "default")
    with pytest.raises(I.IpmzError, match="bad state"):
        g.state_tensor(0)  # never loaded
    g.generate(11)
    L = g.state_len
    for which in (-1, 4):
        with pytest.raises(I.IpmzError, match="invalid argument"):
            g.state_tensor(which)
    narrow = torch.full((B, L - 1), NAN, dtype=torch.float64, device="cuda")
    with pytest.raises(I.IpmzError, match="invalid argument"):
        g.state_tensor(0, out=narrow)
    assert torch.isnan(narrow).all()
    with pytest.raises(I.IpmzError, match="invalid argument"):
        I._check(I.lib.ipmz_batch_copy_state(g.h, 0, None, L), "ipmz_batch_copy_state")
    with pytest.raises(ValueError):
        g.state_tensor(0, out=torch.zeros((B, L), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        g.state_tensor(0, out=torch.zeros((B + 1, L), dtype=torch.float64, device="cuda"))
    g.close()


# 7 ---------------------------------------------------------------------------
def test_load_refused_during_graph_capture():
    shape = MID
    B = shape[3]
    s = torch.cuda.Stream()
    c = I.Context(0, stream=s.cuda_stream)
    try:
        g = make(c, shape, "default")
        g.generate(9)
        g.step()
        before = snapshot(g, B)
        blocks = cuda_blocks(shape, host_data(shape))
        z = torch.zeros(8, device="cuda")
        out = torch.zeros((B, g.state_len), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            z.add_(1.0)
            with pytest.raises(I.IpmzError, match="bad state.*capturing"):
                g.load_tensors(**blocks)
            # the read-back neither allocates nor synchronizes: it goes into the capture
            I._check(I.lib.ipmz_batch_copy_state(g.h, 0, ctypes.c_void_p(out.data_ptr()), g.state_len),
                     "ipmz_batch_copy_state")
        graph.replay()
        torch.cuda.synchronize()
        assert z[0].item() == 1.0
        assert_same(snapshot(g, B), before, "after the refused load")
        assert np.array_equal(bits(out.cpu().numpy()[1]), bits(g.state(1, 0)))
        g.load_tensors(**blocks)  # and outside the capture it works
        ref0, _ = host_reference(shape, "default")
        assert_same(snapshot(g, B), ref0, "load after the capture")
        g.close()
    finally:
        c.close()
