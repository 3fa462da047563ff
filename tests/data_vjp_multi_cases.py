"""Cotangent blocks, the raw call and the measures of the data gradient for a block of cotangent rows per QP
(ipmz_batch_data_vjp_multi: Optimizer.data_grad_tensors_multi; ipmz_amd.layer.solution_vjp / solution_jacobian),
shared by tests/test_gpu_data_vjp_multi.py and tests/test_gpu_qp_vjp_multi.py.

The reference and its measures are those of tests/data_vjp_cases.py (reference_form, shared_reference, rel_err),
applied per (QP, row); the rows come from dc.cotangents' generator with a (B, ncot, L) shape.
"""
import ctypes
import functools

import numpy as np

import data_vjp_cases as dc

RG = 4     # csrc/grad.hip RG: cotangent rows that share a strip's row-independent operands
SLAB = 16  # csrc/kernels.h IPMZ_VJP_SLAB: rows whose partials the workspace holds at a time
# one row (the single row's kernel), a partial group, the group size - 1, + 0, + 1, and the slab size - 1, + 0, + 1
# (a second slab of one row)
NCOTS = (1, 2, RG - 1, RG, RG + 1, SLAB - 1, SLAB, SLAB + 1)
TWO_PRODUCTS = ("A_ineq", "A_eq")
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def cotangents(L, B, ncot):
    """(B, ncot, L) standard-normal cotangent rows: dc.cotangents' generator."""
    w = np.random.default_rng(9700 + L).standard_normal((B, ncot, L))
    w.setflags(write=False)
    return w


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def references(fn, V, W):
    """{name: (B, ncot, ...)}: fn(iterate of QP q, row r of QP q) for every (QP, row)."""
    B, ncot = W.shape[:2]
    each = [[fn(V[q], W[q, r]) for r in range(ncot)] for q in range(B)]
    return {k: np.stack([np.stack([g[k] for g in row]) for row in each]) for k in each[0][0]}


def check_per_qp(got, refs):
    """Every (QP, row)'s block against its reference under test_gpu_data_vjp_batch.py's measures: bitwise where the
    block is a copy, a negation or one product; returns the worst dc.rel_err of the rank-2 blocks."""
    assert set(got) == set(refs)
    worst = 0.0
    for k, ref in refs.items():
        assert got[k].shape == ref.shape, k
        if k in TWO_PRODUCTS:
            for q in range(ref.shape[0]):
                for r in range(ref.shape[1]):
                    worst = max(worst, dc.rel_err(got[k][q, r], ref[q, r]))
        else:
            bad = np.argwhere(bits(got[k]) != bits(ref))
            assert bad.size == 0, (k, "first differing [QP, row, ...]", bad[0].tolist(), len(bad))
    return worst


def check_shared(got, refs):
    """Row r of every shared block against dc.shared_reference of the references' row r; returns the worst
    error / bound."""
    assert set(got) == set(refs)
    worst = 0.0
    for k, ref in refs.items():
        assert got[k].shape == ref.shape[1:], k
        for r in range(ref.shape[1]):
            want, bound = dc.shared_reference(ref[:, r])
            err = float(np.abs(got[k][r] - want).max())
            worst = max(worst, np.inf if np.isnan(err) else err / bound)
    return worst


def raw(I, g, ncot, W_ptr, ldw, sW, spec):
    """The C call itself, its return code.  spec: name -> (address, row stride, QP stride, cotangent-row stride)."""
    gr = I._QPDeviceGradMulti()
    for name, ptr, ld, sq, rows, cols in I._BLOCKS:
        if name in spec:
            addr, l, s, t = spec[name]
            setattr(gr.g, ptr, addr)
            if ld:
                setattr(gr.g, ld, l)
            setattr(gr.g, sq, s)
            setattr(gr, "t" + sq[1:], t)
    return I.lib.ipmz_batch_data_vjp_multi(g.h, ncot, ctypes.c_void_p(W_ptr), ldw, sW, ctypes.byref(gr))


def block_dims(n, m, p):
    """name -> (rows or None, columns) of the blocks a solver of these dimensions has."""
    d = dict(n=n, m=m, p=p)
    import ipmz_amd as I
    out = {}
    for name, _, _, _, rows, cols in I._BLOCKS:
        r, c = (None if rows is None else d[rows]), d[cols]
        if c and r != 0:
            out[name] = (r, c)
    return out


def block_index(r, c, ld, base):
    """The flat indices of a block's elements in its buffer."""
    if r is None:
        return base + np.arange(c)
    return base + np.arange(r)[:, None] * ld + np.arange(c)[None, :]


def everything(g):
    return [g.state(i, w) for i in range(g.batch) for w in range(4)] + [g.batch_scalars()]

