"""Cotangent rows, the independent reference and the bounds of the adjoint
Newton solve (Optimizer.newton_adjoint, Batch.newton_adjoint_all), shared by
tests/test_gpu_newton_adjoint.py (the device) and
tests/test_oracle_newton_adjoint.py (what the reference relies on, no GPU).

Shapes, batches, row counts, the dense Jacobian J and the error measure are
those of the forward call (tests/newton_multi_cases.py).  The forward call is
Dir = M R with M = -J^{-1}; the adjoint is Adj = M^T G, so the reference is
numpy.linalg.solve(J^T, -G^T)^T -- it goes through neither the augmented
system nor the forward call.
"""
import functools

import numpy as np

import newton_multi_cases as nc


@functools.lru_cache(maxsize=None)
def rows(L, B=1):
    """(B, RHS_MAX, L) standard-normal cotangent rows; a call with fewer rows uses the first ones."""
    g = np.random.default_rng(9500 + L).standard_normal((B, nc.RHS_MAX, L))
    g.setflags(write=False)
    return g


def reference_adjoint(q, vars_, G, eq_none=False):
    """numpy.linalg.solve(J^T, -G^T)^T: one cotangent with respect to r_v per row of G."""
    J = nc.full_jacobian(q, vars_, eq_none=eq_none)
    return np.linalg.solve(J.T, -np.asarray(G).T).T


def ld(a):
    return np.asarray(a, dtype=np.longdouble)


def identity_reference(D_I, G):
    """Adj_ref[r][j] = D_I[j] . G[r] in longdouble, D_I the forward call's directions of R = I_L
    (row j: the direction of the j-th unit residual, that is column j of M)."""
    return ld(G) @ ld(D_I).T


def identity_bound(D_I, G, Adj_ref):
    """Per element (r, j), from the forward bar on both sides: the forward call may be off by
    TOL max(1, |D_I[j]|inf) in every element of row j, which G[r] weighs with |G[r]|_1; the adjoint
    call gets the bar itself, TOL max(1, |Adj_ref[r]|inf)."""
    G, D_I, Adj_ref = np.asarray(G), np.asarray(D_I), np.asarray(Adj_ref, dtype=np.float64)
    a = nc.TOL * np.maximum(1.0, np.abs(Adj_ref).max(axis=1))[:, None]
    b = nc.TOL * np.abs(G).sum(axis=1)[:, None] * np.maximum(1.0, np.abs(D_I).max(axis=1))[None, :]
    return a + b


def dot_gap(G, Dir, Adj, R):
    """|<g_a, Dir(r_b)> - <Adj(g_a), r_b>| for all pairs (a, b), in longdouble, and its bound
    TOL (|g_a|_1 max(1, |Dir(r_b)|inf) + |r_b|_1 max(1, |Adj(g_a)|inf))."""
    gap = np.abs(ld(G) @ ld(Dir).T - ld(Adj) @ ld(R).T).astype(np.float64)
    G, Dir, Adj, R = (np.asarray(a, dtype=np.float64) for a in (G, Dir, Adj, R))
    bound = nc.TOL * (np.abs(G).sum(axis=1)[:, None] * np.maximum(1.0, np.abs(Dir).max(axis=1))[None, :] +
                      np.abs(R).sum(axis=1)[None, :] * np.maximum(1.0, np.abs(Adj).max(axis=1))[:, None])
    return gap, bound
