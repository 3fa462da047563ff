"""The data gradient for a block of cotangent rows per QP on the device (ipmz_batch_data_vjp_multi:
Optimizer.data_grad_tensors_multi and the raw call), through the public ABI only.

Reference (tests/data_vjp_cases.py): reference_form per (QP, row), numpy only, from the device's iterate and the
cotangent row alone, under the measures of tests/test_gpu_data_vjp_batch.py -- bitwise where a block is a copy, a
negation or one product, dc.rel_err <= nc.TOL for the rank-2 blocks A_ineq and A_eq, dc.shared_reference's bound for
shared blocks.  The row contract is checked bitwise against the single-row call, Optimizer.data_grad_tensors, row by
row.  Every test prints its worst figure before it asserts.
"""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import data_vjp_cases as dc
import data_vjp_multi_cases as mc
import newton_multi_cases as nc

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")
torch = pytest.importorskip("torch")

NAN = mc.NAN
INVALID, STATE = -1, -5  # include/ipmz.h IPMZ_ERR_INVALID, IPMZ_ERR_STATE


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


def _stepped(name, shape, B, ncot, seed0, ctx, steps=2):
    """The batch after `steps` steps, its iterates (B, L) on the host and its (B, ncot, L) cotangents on both sides."""
    bt = I.Batch(*shape, B, ctx, **dc.form_kw(name))
    bt.generate(seed0)
    for _ in range(steps):
        bt.step()
    L = bt.state_len
    assert L == dc.form_offsets(name, *shape)[3]
    V = bt.state_tensor(0).cpu().numpy()
    assert V.shape == (B, L) and np.isfinite(V).all()
    W = np.array(mc.cotangents(L, B, ncot))
    return bt, V, W, _dev(W)


# 1 ---------------------------------------------------------------------------
FORM_B, FORM_NCOT = 5, 3  # B = 5: one full K step of the 16x16x4 MFMA plus a tail of one
FORM_SHAPE, FORM_SHAPE_M0 = (12, 5, 3), (12, 0, 3)
FORM_CASES = [(name, FORM_SHAPE) for name in dc.FORM_NAMES] + [(name, FORM_SHAPE_M0) for name in dc.M0_FORMS]


@pytest.mark.parametrize("name,shape", FORM_CASES, ids=[f"{n}-m{s[1]}" for n, s in FORM_CASES])
def test_every_formulation_against_numpy(ctx, name, shape):
    n, m, p = shape
    B, ncot = FORM_B, FORM_NCOT
    bt, V, W, Wt = _stepped(name, shape, B, ncot, 1000, ctx)
    names = dc.present(n, m, p)
    refs = mc.references(lambda v, w: dc.reference_form(name, n, m, p, v, w), V, W)
    assert set(refs) == set(names)
    per = _host(bt.data_grad_tensors_multi(Wt))
    sh = _host(bt.data_grad_tensors_multi(Wt, shared=names))
    for k in names:
        assert per[k].shape[:2] == (B, ncot) and sh[k].shape[0] == ncot and sh[k].shape[1:] == per[k].shape[2:], k
    worst_per = mc.check_per_qp(per, refs)
    worst_sh = mc.check_shared(sh, refs)
    print(f"{name} n{n} m{m} p{p} B={B} ncot={ncot}: per-QP A_ineq / A_eq vs numpy {worst_per:.3e} (bound "
          f"{nc.TOL:.1e}), the other blocks bitwise; shared vs the longdouble sum, error / bound {worst_sh:.3e}",
          flush=True)
    assert worst_per <= nc.TOL
    assert worst_sh <= 1.0
    for k in dc.form_absent(name):
        if k in names:  # a bound the formulation lacks: exactly zero in both layouts
            assert not per[k].any() and not sh[k].any(), k


# 2 ---------------------------------------------------------------------------
SMALL, LARGE = (12, 5, 3), (130, 40, 22)  # LARGE: partial 16 x 64 tiles and an odd tile count
# B = 1: a solver of one QP; 3, 63: the K tail of the 16x16x4 MFMA; 63, 64, 65: the chunk boundary
ROW_CASES = [(SMALL, b) for b in (1, 3, dc.KCHUNK - 1, dc.KCHUNK, dc.KCHUNK + 1)] + [(LARGE, 3)]


@pytest.mark.parametrize("shape,B", ROW_CASES, ids=[f"n{s[0]}-B{b}" for s, b in ROW_CASES])
def test_every_row_has_the_bits_of_the_single_row_call(ctx, shape, B):
    """Every row of the multi call np.array_equal's (on the bit patterns) data_grad_tensors of that row alone, per QP
    and shared, for every ncot of mc.NCOTS; the rows of a smaller ncot are the leading rows of the largest."""
    n, m, p = shape
    top = max(mc.NCOTS)
    t0 = time.perf_counter()
    bt, V, W, Wt = _stepped("box", shape, B, top, 1000, ctx)
    names = dc.present(n, m, p)
    single = [(_host(bt.data_grad_tensors(Wt[:, r].contiguous())),
               _host(bt.data_grad_tensors(Wt[:, r].contiguous(), shared=names))) for r in range(top)]
    compared = 0
    for ncot in mc.NCOTS:
        Wn = Wt[:, :ncot]  # (a view: QP stride top * L, row stride L)
        per = _host(bt.data_grad_tensors_multi(Wn))
        sh = _host(bt.data_grad_tensors_multi(Wn, shared=names))
        assert set(per) == set(sh) == set(names)
        for k in names:
            assert not np.isnan(per[k]).any() and not np.isnan(sh[k]).any(), (ncot, k)
            for r in range(ncot):
                assert mc.same(per[k][:, r], single[r][0][k]), ("per QP", ncot, k, r)
                assert mc.same(sh[k][r], single[r][1][k]), ("shared", ncot, k, r)
                compared += 2
    print(f"n{n} m{m} p{p} B={B}: ncot in {mc.NCOTS}, {compared} (block, row) results bitwise those of the single-row "
          f"call, 0 differ; {time.perf_counter() - t0:.2f} s", flush=True)


# 3 ---------------------------------------------------------------------------
def _layout(bt, B, ncot, W_ptr, ldw, sW, off, shared):
    """Every block at element offset `off` of a NaN-filled buffer: row stride n + 5 (even for n = 131), cotangent-row
    stride extent + 10 rounded to even, QP stride (ncot - 1) * tq + extent + 6 rounded to even -- or, shared, 0.
    Returns ({name: (B, ncot, ...) gathered, (ncot, ...) when shared}, every buffer's padding kept its bits)."""
    spec, bufs, where = {}, {}, {}
    for name, (r, c) in mc.block_dims(bt.n, bt.m, bt.p).items():
        ld = c + 5 if r is not None else 0
        extent = (r - 1) * ld + c if r is not None else c
        tq = extent + 10 + (extent & 1)
        sq = 0 if shared else (ncot - 1) * tq + extent + 6 + (extent & 1)
        host = np.full(off + (1 if shared else B) * ((ncot - 1) * tq + extent + 6 + (extent & 1)) + 4, NAN)
        dev = _dev(host)
        bufs[name], where[name] = (host, dev), (r, c, ld, sq, tq)
        spec[name] = (dev.data_ptr() + 8 * off, ld, sq, tq)
    torch.cuda.synchronize()
    assert mc.raw(I, bt, ncot, W_ptr, ldw, sW, spec) == 0, I.lib.ipmz_last_error()
    bt.ctx.sync()
    out, clean = {}, True
    for name, (host, dev) in bufs.items():
        r, c, ld, sq, tq = where[name]
        dv = dev.cpu().numpy()
        inside = np.zeros(dv.shape, bool)
        blocks = []
        for qi in range(1 if shared else B):
            rowsq = []
            for ri in range(ncot):
                idx = mc.block_index(r, c, ld, off + qi * sq + ri * tq)
                inside[idx.reshape(-1)] = True
                rowsq.append(dv[idx])
            blocks.append(np.stack(rowsq))
        out[name] = blocks[0] if shared else np.stack(blocks)
        clean = clean and np.array_equal(mc.bits(dv[~inside]), mc.bits(host[~inside])) and not np.isnan(dv[inside]).any()
    return out, clean


def test_layout(ctx):
    """n = 131: the element path's c += 64 loop makes three passes and the 16-byte path's c += 128 loop a second one
    that ends on the odd column's scalar store.  Strides larger than the extents at element offsets 0 (16-byte
    stores: aligned, all three strides even) and 1 (element stores); W with ldw > L at an odd element offset."""
    n, m, p, B, ncot = 131, 5, 3, 2, 3
    bt, V, W, Wt = _stepped("box", (n, m, p), B, ncot, 1000, ctx)
    L = bt.state_len
    names = dc.present(n, m, p)
    ref = _host(bt.data_grad_tensors_multi(Wt))
    ref_sh = _host(bt.data_grad_tensors_multi(Wt, shared=names))
    ldw, woff = L + 3, 1
    sW = ncot * ldw + 5
    Wh = np.full(woff + B * sW + 2, -7.25)  # (a finite sentinel: W is read, never written)
    for q in range(B):
        for r in range(ncot):
            Wh[woff + q * sW + r * ldw:woff + q * sW + r * ldw + L] = W[q, r]
    Wd = _dev(Wh)
    for off in (0, 1):
        got, clean = _layout(bt, B, ncot, Wd.data_ptr() + 8 * woff, ldw, sW, off, False)
        assert clean, f"per QP, offset {off}: row padding and the space between rows and QPs keep their bits"
        got_sh, clean_sh = _layout(bt, B, ncot, Wd.data_ptr() + 8 * woff, ldw, sW, off, True)
        assert clean_sh, f"shared, offset {off}: row padding and the space between rows keep their bits"
        for k in names:
            assert mc.same(got[k], ref[k]), ("per QP", off, k)
            assert mc.same(got_sh[k], ref_sh[k]), ("shared", off, k)
    assert mc.same(Wd.cpu().numpy(), Wh), "W keeps its bits"
    print(f"layout n={n} B={B} ncot={ncot}: 16-byte and element paths at strides beyond the extents bitwise the "
          f"contiguous result, per QP and shared; padding, gaps and W untouched", flush=True)


# 4 ---------------------------------------------------------------------------
def test_pair_loop_past_the_grid(ctx):
    """B = 1025, ncot = 4: 4100 (QP, row) pairs, past dc.GRID_Y workgroups of the looped grid dimension; 17 chunks."""
    n, m, p = shape = dc.LOOP_SHAPE
    B, ncot = 1025, 4
    assert B * ncot > dc.GRID_Y
    t0 = time.perf_counter()
    bt, V, W, Wt = _stepped("box", shape, B, ncot, 1000, ctx)
    names = dc.present(n, m, p)
    refs = mc.references(lambda v, w: dc.reference_form("box", n, m, p, v, w), V, W)
    per = _host(bt.data_grad_tensors_multi(Wt))
    sh = _host(bt.data_grad_tensors_multi(Wt, shared=names))
    worst_per = mc.check_per_qp(per, refs)
    worst_sh = mc.check_shared(sh, refs)
    print(f"n{n} m{m} p{p} B={B} ncot={ncot}: per-QP A_ineq / A_eq vs numpy {worst_per:.3e} (bound {nc.TOL:.1e}), the "
          f"other blocks bitwise for every (QP, row); shared error / bound {worst_sh:.3e}; "
          f"{time.perf_counter() - t0:.2f} s", flush=True)
    assert worst_per <= nc.TOL
    assert worst_sh <= 1.0


@pytest.mark.parametrize("name", ("box", "sl"))
def test_shared_vectors_over_several_qps_per_range(ctx, name):
    """B = 257, ncot = 3: a range of k_grad_vectors_shared holds 5 QPs (a full group of four plus a tail); both
    branches (plain loads, and the Slacks forms' iterate-dependent terms)."""
    n, m, p = shape = dc.LOOP_SHAPE
    B, ncot = dc.LOOP_BATCHES[0], 3
    bt, V, W, Wt = _stepped(name, shape, B, ncot, 1000, ctx)
    vectors = tuple(k for k in dc.NAMES if k not in dc.MATRICES)
    refs = mc.references(lambda v, w: dc.reference_form(name, n, m, p, v, w), V, W)
    refs = {k: refs[k] for k in vectors}
    sh = _host(bt.data_grad_tensors_multi(Wt, shared=vectors, only=vectors))
    worst = mc.check_shared(sh, refs)
    print(f"{name} n{n} m{m} p{p} B={B} ncot={ncot}: shared vectors vs the longdouble sum, error / bound {worst:.3e}",
          flush=True)
    assert worst <= 1.0


@pytest.mark.parametrize("ncot", (2, 5))
def test_shared_sum_second_pass(ctx, ncot):
    """n = dc.BIG_N, m = p = 0, B = 2, Q shared only: rows * n exceeds k_grad_shared_sum's 2048 x 256 threads, so
    its grid-stride loop makes a second pass for each row; its grid then holds dc.GRID_Y // dc.SUM_GX = 2 rows at a
    time, so at ncot = 5 the row loop makes three passes."""
    n, B = dc.BIG_N, 2
    assert n * n > dc.SUM_GX * 256 and (ncot == 2 or ncot > 2 * (dc.GRID_Y // dc.SUM_GX))
    t0 = time.perf_counter()
    bt, V, W, Wt = _stepped("box", (n, 0, 0), B, ncot, 1000, ctx)
    refs = {"Q": np.stack([np.stack([np.outer(W[q, r, :n], V[q, :n]) for r in range(ncot)]) for q in range(B)])}
    sh = _host(bt.data_grad_tensors_multi(Wt, shared=["Q"], only=["Q"]))
    worst = mc.check_shared(sh, refs)
    print(f"n={n} B={B} ncot={ncot}: shared Q vs the longdouble sum, error / bound {worst:.3e}; "
          f"{time.perf_counter() - t0:.2f} s", flush=True)
    assert worst <= 1.0
    for r in range(ncot):
        one = _host(bt.data_grad_tensors(Wt[:, r].contiguous(), shared=["Q"], only=["Q"]))["Q"]
        assert mc.same(sh["Q"][r], one), r


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("eq_none", (False, True), ids=("ldlt", "bk"))
def test_nothing_else_moves(ctx, eq_none):
    n, m, p, B, seed0 = nc.BATCHES[0]
    ncot = 5
    kw = dict(equality_handling=I.EQ_NONE if eq_none else I.EQ_REGULARIZATION)
    a, b = I.Batch(n, m, p, B, ctx, **kw), I.Batch(n, m, p, B, ctx, **kw)
    a.generate(seed0)
    b.generate(seed0)
    L = a.state_len
    Wt = _dev(np.array(mc.cotangents(L, B, ncot)))
    names = dc.present(n, m, p)
    for k in range(3):
        before = mc.everything(b)
        b.data_grad_tensors_multi(Wt, shared=names if k % 2 else ())
        for x, y in zip(before, mc.everything(b)):
            assert np.array_equal(x, y, equal_nan=True), "the call itself"
        a.step(I.STEP_GRAPH)
        b.step(I.STEP_GRAPH)
    assert a.last_step_graph() and b.last_step_graph()
    differ = sum(not np.array_equal(x, y, equal_nan=True) for x, y in zip(mc.everything(a), mc.everything(b)))
    print(f"eq_none={eq_none}: states (4 kinds), scalars and graph-replayed steps of the twin: {differ} differ", flush=True)
    assert differ == 0


def test_dimension_zero_and_no_rows(ctx):
    """Blocks of dimension 0 are ignored whatever they hold; ncot = 0 writes nothing."""
    n, B, ncot = 40, 2, 3
    bt, V, W, Wt = _stepped("box", (n, 0, 0), B, ncot, 1000, ctx, steps=1)
    L = bt.state_len
    ref = _host(bt.data_grad_tensors_multi(Wt))
    assert set(ref) == {"Q", "c", "l_x", "u_x"}
    tq, tc = _dev(np.full((B, ncot, n, n), NAN)), _dev(np.full((B, ncot, n), NAN))
    junk = 0xdead0
    good = dict(Q=(tq.data_ptr(), n, ncot * n * n, n * n), c=(tc.data_ptr(), 0, ncot * n, n))
    spec = dict(good, A_ineq=(junk, 1, -5, -1), l_A_ineq=(junk, 0, 1, 0), u_A_ineq=(junk, 0, 1, -3), A_eq=(junk, 0, 0, 0),
                b_eq=(junk, 0, -1, 1))
    assert mc.raw(I, bt, ncot, Wt.data_ptr(), L, ncot * L, spec) == 0, I.lib.ipmz_last_error()
    bt.ctx.sync()
    assert mc.same(tq.cpu().numpy(), ref["Q"]) and mc.same(tc.cpu().numpy(), ref["c"])
    tq.fill_(NAN), tc.fill_(NAN)
    torch.cuda.synchronize()
    assert mc.raw(I, bt, 0, Wt.data_ptr(), L, L, good) == 0, I.lib.ipmz_last_error()
    bt.ctx.sync()
    assert np.isnan(tq.cpu().numpy()).all() and np.isnan(tc.cpu().numpy()).all()
    empty = bt.data_grad_tensors_multi(Wt[:, :0])
    assert empty["Q"].shape == (B, 0, n, n) and empty["c"].shape == (B, 0, n)
    print("m = 0, p = 0: garbage A / C / l_A / u_A / d blocks ignored; ncot = 0 wrote nothing", flush=True)


# 6 ---------------------------------------------------------------------------
def test_errors(ctx):
    n, m, p, B, seed0 = nc.BATCHES[0]
    ncot = 3
    bt = I.Batch(n, m, p, B, ctx)
    bt.generate(seed0)
    L = bt.state_len
    Wt = _dev(np.zeros((B, ncot, L)))
    W = Wt.data_ptr()
    tq, tc = _dev(np.full((B, ncot, n, n), NAN)), _dev(np.full((B, ncot, n), NAN))
    eQ, sQ = n * n, ncot * n * n
    good = dict(Q=(tq.data_ptr(), n, sQ, eQ), c=(tc.data_ptr(), 0, ncot * n, n))

    def rc(g, nc_, ldw, sW, spec):
        torch.cuda.synchronize()
        r = mc.raw(I, g, nc_, W, ldw, sW, spec)
        g.ctx.sync()
        return r

    assert rc(bt, ncot, L, ncot * L, good) == 0, I.lib.ipmz_last_error()
    checks = {
        "ncot < 0": rc(bt, -1, L, ncot * L, good),
        "ldw < L": rc(bt, ncot, L - 1, ncot * L, good),
        "sW < (ncot - 1) ldw + L": rc(bt, ncot, L, ncot * L - 1, good),
        "row stride < n": rc(bt, ncot, L, ncot * L, dict(Q=(tq.data_ptr(), n - 1, sQ, eQ))),
        "cotangent-row stride below the extent": rc(bt, ncot, L, ncot * L, dict(Q=(tq.data_ptr(), n, sQ, eQ - 1))),
        "vector cotangent-row stride below its length": rc(bt, ncot, L, ncot * L, dict(c=(tc.data_ptr(), 0, ncot * n, n - 1))),
        "QP stride below (ncot - 1) tX + extent": rc(bt, ncot, L, ncot * L, dict(Q=(tq.data_ptr(), n, sQ - 1, eQ))),
        "vector QP stride below (ncot - 1) tX + extent": rc(bt, ncot, L, ncot * L, dict(c=(tc.data_ptr(), 0, ncot * n - 1, n))),
        "negative QP stride": rc(bt, ncot, L, ncot * L, dict(Q=(tq.data_ptr(), n, -sQ, eQ))),
        "negative cotangent-row stride": rc(bt, ncot, L, ncot * L, dict(c=(tc.data_ptr(), 0, ncot * n, -n))),
        "negative row stride": rc(bt, ncot, L, ncot * L, dict(Q=(tq.data_ptr(), -n, sQ, eQ))),
    }
    gr = I._QPDeviceGradMulti()
    lib = I.lib
    checks["null qp"] = lib.ipmz_batch_data_vjp_multi(None, ncot, ctypes.c_void_p(W), L, ncot * L, ctypes.byref(gr))
    checks["null W"] = lib.ipmz_batch_data_vjp_multi(bt.h, ncot, None, L, ncot * L, ctypes.byref(gr))
    checks["null grad"] = lib.ipmz_batch_data_vjp_multi(bt.h, ncot, ctypes.c_void_p(W), L, ncot * L, None)
    for kw in (dict(equality_handling=I.EQ_SLACKED_SLACKS),
               dict(equality_handling=I.EQ_NAIVE_SLACKS, inequality_handling=I.INEQ_NAIVE_SLACKS)):
        e = I.Batch(n, m, p, B, ctx, **kw)
        e.generate(seed0)
        big = _dev(np.zeros((B, ncot, e.state_len)))
        torch.cuda.synchronize()
        checks[f"refused formulation {sorted(kw.values())}"] = mc.raw(I, e, ncot, big.data_ptr(), e.state_len,
                                                                     ncot * e.state_len, good)
    g = I.Optimizer(n, m, p, ctx)
    g.generate(nc.SEED)
    one = dict(Q=(tq.data_ptr(), n, 0, eQ), c=(tc.data_ptr(), 0, 0, n))
    assert rc(g, ncot, L, 0, one) == 0, I.lib.ipmz_last_error()  # (a solver of one QP ignores sW and the QP strides)
    g.set_reduction(I.REDUCTION_NORMAL)
    checks["normal-equations reduction"] = rc(g, ncot, L, 0, one)
    g.set_reduction(I.REDUCTION_AUGMENTED)
    g.set_mixed_precision(True)
    checks["mixed precision"] = rc(g, ncot, L, 0, one)
    g.set_mixed_precision(False)
    assert rc(g, ncot, L, 0, one) == 0
    print("IPMZ_ERR_INVALID cases: " + ", ".join(f"{k}: {v}" for k, v in checks.items()), flush=True)
    for k, v in checks.items():
        assert v == INVALID, (k, v)
    fresh = I.Batch(n, m, p, B, ctx)
    before_load = rc(fresh, ncot, L, ncot * L, good)
    print(f"before a load: {before_load}", flush=True)
    assert before_load == STATE
    # only the good calls wrote, and they wrote whole blocks
    assert not np.isnan(tq.cpu().numpy()).any() and not np.isnan(tc.cpu().numpy()).any()


_CAPTURE_CHILD = r"""
import ctypes, sys
import numpy as np
import torch
import ipmz_amd as I
import data_vjp_multi_cases as mc
import newton_multi_cases as nc

n, m, p, B, seed0 = nc.BATCHES[0]
ncot = 3
s = torch.cuda.Stream()
c = I.Context(0, stream=s.cuda_stream)
bt = I.Batch(n, m, p, B, c)
bt.generate(seed0)
bt.step()
L = bt.state_len
Wt = torch.from_numpy(np.array(mc.cotangents(L, B, ncot))).cuda()
W1 = Wt[:, 0].contiguous()
tq = torch.full((ncot, n, n), float("nan"), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
one = bt.data_grad_tensors(W1, shared=["Q"], only=["Q"])["Q"]          # the single row's workspace exists now
ref = bt.data_grad_tensors(W1, shared=["Q"], only=["Q"])["Q"].cpu().numpy()
torch.cuda.synchronize()
spec = dict(Q=(tq.data_ptr(), n, 0, n * n))
out = {}
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
    out["grow"] = mc.raw(I, bt, ncot, Wt.data_ptr(), L, ncot * L, spec)    # three rows' partials: it would have to grow
    out["msg"] = I.lib.ipmz_last_error().decode()
    out["fits"] = mc.raw(I, bt, 1, Wt.data_ptr(), L, ncot * L, spec)       # one row fits: captured
graph.replay()
torch.cuda.synchronize()
got = tq.cpu().numpy()
out["row0"] = bool(mc.same(got[0], ref))
out["rest_untouched"] = bool(np.isnan(got[1:]).all())
sh = bt.data_grad_tensors_multi(Wt, shared=["Q"], only=["Q"])["Q"].cpu().numpy()   # outside: grows
graph2 = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph2, stream=s, capture_error_mode="thread_local"):
    out["after"] = mc.raw(I, bt, ncot, Wt.data_ptr(), L, ncot * L, spec)
graph2.replay()
torch.cuda.synchronize()
out["replayed"] = bool(mc.same(tq.cpu().numpy(), sh))
print("RESULT", out, flush=True)
ok = out["grow"] == -5 and "capturing" in out["msg"] and out["fits"] == 0 and out["row0"] and out["rest_untouched"] \
    and out["after"] == 0 and out["replayed"]
bt.close()
c.close()
sys.exit(0 if ok else 3)
"""


def test_capture_cannot_grow_the_workspace():
    """Inside a caller's graph capture the workspace cannot grow: IPMZ_ERR_STATE for a call with more rows than any
    before it, until one such call outside a capture.  In a child process: a capture that goes wrong stays there."""
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([here, os.path.join(repo, "ipm-zoo_amd"), os.path.join(repo, "oracle"), repo,
                                         env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", _CAPTURE_CHILD], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:], flush=True)
    assert r.returncode == 0
