"""The argument checks of the nine data blocks (Q, A, C, c, l_x, u_x, l_A, u_A, d) in the three calls that take them
-- ipmz_batch_load_device, ipmz_batch_data_vjp, ipmz_batch_data_jvp -- through ctypes, on the default formulation at
(n, m, p) = (12, 5, 3): one table of strides per block, the same for every call where the calls agree.

With extent = (rows - 1) * ld + n for a matrix block (ld = n here) and the length for a vector block, tq the tangent
stride and all = (ntan - 1) * tq + extent (the load and the gradient: ntan = 1):

    row stride n - 1, -1 (matrices)                  invalid
    batch:   QP stride -1, extent - 1, all - 1       invalid;   all, 0: accepted
    ntan 2:  tangent stride extent - 1               invalid;   extent: accepted
    one QP:  QP stride -1                            invalid for the load and the gradient, ignored by the tangents
    ntan 1:  tangent stride -1                       ignored

Every refusal returns IPMZ_ERR_INVALID, names the block in ipmz_last_error, and leaves the outputs and the solver's
state bit-equal to a twin solver that never made the call.  Precedence: mixed precision enabled plus a bad stride
reports the mixed-precision refusal (gradient, tangents; the load is served with mixed precision and reports the
stride); an unloaded solver plus a bad stride reports IPMZ_ERR_STATE (gradient, tangents; the load of a new solver
checks the strides before it looks for missing blocks and reports the stride).  Blocks of dimension 0 are ignored
whatever they hold.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

N, M, P = SHAPE = (12, 5, 3)
INVALID, STATE = -1, -5
SENTINEL = -123.25
SEED = 4100
# load_tensors' name, the name the messages print, rows (None: a vector), length of a row / of the vector, fill value
# of an accepted load (bounds far apart: the bound check against the held side passes)
BLOCKS = (("Q", "Q", N, N, 1.0), ("A_ineq", "A", M, N, 1.0), ("A_eq", "C", P, N, 1.0), ("c", "c", None, N, 1.0),
          ("l_x", "l_x", None, N, -1e6), ("u_x", "u_x", None, N, 1e6), ("l_A_ineq", "l_A", None, M, -1e6),
          ("u_A_ineq", "u_A", None, M, 1e6), ("b_eq", "d", None, P, 0.0))
FIELDS = {b[0]: b[1:] for b in I._BLOCKS}  # name -> (pointer, row stride or None, QP stride, rows, cols)
CALLS = ("load", "vjp", "jvp1", "jvp2")


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


def _make(B, ctx, shape=SHAPE, generate=True):
    s = I.Optimizer(*shape, ctx) if B == 1 else I.Batch(*shape, B, ctx)
    if generate:
        s.generate(SEED)
        s.step()
    return s


def _everything(s, B):
    out = [s.state_tensor(w).cpu().numpy() for w in range(4)]
    if B == 1:
        sc = s.scalars()
        return out + [np.array([sc[k] for k in sorted(sc)]), np.asarray(s.kkt())]
    return out + [np.asarray(s.batch_scalars())] + [np.asarray(s.kkt_of(i)) for i in range(B)]


def _equal(xs, ys):
    return len(xs) == len(ys) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(xs, ys))


class Call:
    """One of the three C calls on one solver, with every buffer it needs; run(spec) -> (return code, message).
    spec: load_tensors' name -> (address, row stride, QP stride, tangent stride)."""

    def __init__(self, kind, s, B):
        self.kind, self.s, self.B = kind, s, B
        self.ntan = 2 if kind == "jvp2" else 1
        L = s.state_len
        self.ldr = L + (L & 1)
        self.W = torch.full((B, L), 0.5, dtype=torch.float64, device="cuda")
        self.R = torch.full((B, self.ntan, self.ldr), SENTINEL, dtype=torch.float64, device="cuda")

    def run(self, spec):
        lib, s = I.lib, self.s
        st = I._QPDeviceTangent() if self.kind.startswith("jvp") else \
            I._QPDeviceGrad() if self.kind == "vjp" else I._QPDeviceData()
        d = st.d if self.kind.startswith("jvp") else st
        for name, (addr, ld, sq, tq) in spec.items():
            ptr, fld, fsq = FIELDS[name][:3]
            setattr(d, ptr, addr)
            if fld:
                setattr(d, fld, ld)
            setattr(d, fsq, sq)
            if self.kind.startswith("jvp"):
                setattr(st, "t" + fsq[1:], tq)
        torch.cuda.synchronize()
        if self.kind == "load":
            rc = lib.ipmz_batch_load_device(s.h, ctypes.byref(st))
        elif self.kind == "vjp":
            rc = lib.ipmz_batch_data_vjp(s.h, ctypes.c_void_p(self.W.data_ptr()), self.W.shape[1], ctypes.byref(st))
        else:
            rc = lib.ipmz_batch_data_jvp(s.h, self.ntan, ctypes.byref(st), ctypes.c_void_p(self.R.data_ptr()), self.ldr,
                                         self.ntan * self.ldr)
        msg = lib.ipmz_last_error().decode() if rc else ""
        s.ctx.sync()
        return rc, msg


def _table(B, ntan, rows, cols, kind):
    """(what, row stride, QP stride, tangent stride, accepted) for one block, from the module's docstring."""
    ld = cols
    extent = cols if rows is None else (rows - 1) * ld + cols
    tq = extent
    al = (ntan - 1) * tq + extent
    t = [("packed strides", ld, al, tq, True)]
    if rows is not None:
        t += [("row stride n - 1", ld - 1, al, tq, False), ("row stride -1", -1, al, tq, False)]
    if B > 1:
        t += [("QP stride -1", ld, -1, tq, False), ("QP stride extent - 1", ld, extent - 1, tq, False),
              ("QP stride all - 1", ld, al - 1, tq, False), ("QP stride all", ld, al, tq, True),
              ("QP stride 0", ld, 0, tq, True)]
    else:
        t += [("QP stride -1, one QP", ld, -1, tq, kind.startswith("jvp"))]
    if ntan > 1:
        t += [("tangent stride extent - 1", ld, (ntan - 1) * (tq - 1) + extent, tq - 1, False),
              ("tangent stride extent", ld, al, tq, True)]
    elif kind.startswith("jvp"):
        t += [("tangent stride -1, ntan 1", ld, al, -1, True)]
    return t, al


@pytest.mark.parametrize("B", (1, 3), ids=("one", "batch3"))
@pytest.mark.parametrize("kind", CALLS)
def test_block_guards(ctx, kind, B):
    a, twin, acc = _make(B, ctx), _make(B, ctx), _make(B, ctx)
    ref = _everything(twin, B)
    assert _equal(_everything(a, B), ref)
    call, ok_call = Call(kind, a, B), Call(kind, acc, B)
    refused = accepted = 0
    for name, printed, rows, cols, fill in BLOCKS:
        table, al = _table(B, call.ntan, rows, cols, kind)
        buf = torch.full((B * al + 8,), SENTINEL if kind == "vjp" else fill, dtype=torch.float64, device="cuda")
        for what, ld, sq, tq, ok in table:
            if ok:
                rc, msg = ok_call.run({name: (buf.data_ptr(), ld, sq, tq)})
                assert rc == 0, (kind, B, printed, what, rc, msg)
                accepted += 1
                if kind == "vjp":
                    buf.fill_(SENTINEL)
                continue
            rc, msg = call.run({name: (buf.data_ptr(), ld, sq, tq)})
            assert rc == INVALID, (kind, B, printed, what, rc, msg)
            assert f": {printed}: " in msg, (kind, B, printed, what, msg)
            refused += 1
        # nothing written by the refused calls: the block (gradient), R (tangents), the solver's state (all)
        if kind == "vjp":
            assert (buf == SENTINEL).all().item(), (kind, B, printed)
        assert (call.R == SENTINEL).all().item(), (kind, B, printed)
        assert _equal(_everything(a, B), ref), (kind, B, printed)
    print(f"{kind} B={B}: {refused} refusals name their block and leave the twin's bits, {accepted} accepted", flush=True)
    assert refused >= 6 and accepted >= 9  # (at the least: the matrices' two row strides; every block as packed)


@pytest.mark.parametrize("kind", CALLS)
def test_error_precedence(ctx, kind):
    bad = {"Q": (16, N - 1, 0, 0)}  # (the address is never read: the call is refused)
    g = _make(1, ctx)
    g.set_mixed_precision(True)
    rc, msg = Call(kind, g, 1).run(bad)
    assert rc == INVALID
    assert (": Q: row stride" in msg) if kind == "load" else ("mixed precision" in msg), msg
    fresh = _make(3, ctx, generate=False)
    rc, msg = Call(kind, fresh, 3).run(bad)
    assert (rc == INVALID and ": Q: row stride" in msg) if kind == "load" else (rc == STATE), (rc, msg)


@pytest.mark.parametrize("shape,junk", (((N, 0, P), ("A_ineq", "l_A_ineq", "u_A_ineq")), ((N, M, 0), ("A_eq", "b_eq"))),
                         ids=("m0", "p0"))
@pytest.mark.parametrize("kind", CALLS)
def test_blocks_of_dimension_zero_are_ignored(ctx, kind, shape, junk):
    B = 3
    a, b = _make(B, ctx, shape), _make(B, ctx, shape)
    ca, cb = Call(kind, a, B), Call(kind, b, B)
    ntan = ca.ntan
    bufs = [torch.full((B * ntan * N,), SENTINEL if kind == "vjp" else 1.0, dtype=torch.float64, device="cuda")
            for _ in range(2)]
    good = [{"c": (t.data_ptr(), 0, ntan * N, N)} for t in bufs]
    garbage = {k: (0xdead0, -3, -5, -1) for k in junk}
    (rc0, m0), (rc1, m1) = ca.run(good[0]), cb.run({**good[1], **garbage})
    assert rc0 == 0 and rc1 == 0, (m0, m1)
    assert np.array_equal(bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), equal_nan=True)
    assert np.array_equal(ca.R.cpu().numpy(), cb.R.cpu().numpy(), equal_nan=True)
    assert _equal(_everything(a, B), _everything(b, B))
    if kind == "vjp":
        assert not (bufs[1] == SENTINEL).any().item()
