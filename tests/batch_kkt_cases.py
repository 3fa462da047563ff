"""Shapes, right-hand sides, reference and error measure of the batched
multi-right-hand-side KKT solve (Batch.kkt_solve_all), shared by
tests/test_gpu_batch_kkt_multi.py (the device) and
tests/test_oracle_batch_kkt_multi.py (what the shapes rely on, without a GPU).

Every QP of a batch is oracle.gen_qp(n, m, p, seed0 + i), as Batch.generate.
"""
import functools
import os
import re

import numpy as np

import oracle

# (n, m, p, batch, seed0): the smallest shapes at which each piece can still go wrong
SHAPES = [
    (48, 16, 8, 3, 1000),     # N = 72: one full inner block + 8 columns
    (130, 40, 22, 3, 1100),   # N = 192: three whole blocks, no ragged edge
    (256, 48, 17, 3, 1200),   # N = 321: odd; last block one column; nbi 128: a one-column second sub-block; ldb 322
    (640, 160, 32, 2, 1300),  # N = 832: the largest order whose slab fits a workgroup's LDS (nbi 64)
    (642, 160, 32, 2, 1400),  # N = 834: the first that does not: the panel chain, 4 panels
    (800, 200, 40, 2, 100),   # N = 1040: a non-fused batch, 4 panels + 16 columns
]
NBI128_ORDERS = (72, 321)       # also run on an nbi = 128 context
RHS_COUNTS = (1, 3, 16, 17, 33)  # looped: 1, 3; one full group of 16; a one-row second group; 33
RHS_MAX = max(RHS_COUNTS)
TOL = 1e-12  # |x - x_ref|_inf < TOL * max(1, |x_ref|_inf) per row
MULTI_BLOCKED, MULTI_W512, MULTI_W128 = 65536, 131072, 262144  # csrc/kernels.h IPMZ_DEBUG_MULTI_*
PANEL = 256            # include/ipmz.h IPMZ_SOLVE_MULTI_PANEL: the panel chain's default width
LDS_BYTES = 160 * 1024  # LDS a workgroup may use on an MI355X

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipm-zoo_amd", "csrc")


def case_id(c):
    return f"N{c[0] + c[1] + c[2]}"


def order(c):
    return c[0] + c[1] + c[2]


def ldb_of(N):
    """The smallest even row stride."""
    return N + (N & 1)


def trsm_constants():
    """The tile constants of csrc/trsm.hip the fused kernel's LDS follows from."""
    with open(os.path.join(CSRC, "trsm.hip")) as f:
        src = f.read()
    c = {k: int(re.search(rf"constexpr int {k} = (\d+);", src).group(1)) for k in ("TM_G", "TM_SB", "TM_BK")}
    assert re.search(r"constexpr int TM_PADN = TM_SB \+ 16;", src)
    assert re.search(r"constexpr int TM_STAGE = TM_BK \* TM_PADN;", src)
    # panel_lds_bytes: slab + T + two stage buffers
    assert ("return (size_t)(TM_G * (w + Mfma<T>::V) + TM_G * (nbi + Mfma<T>::V) + 2 * TM_STAGE) * sizeof(T);"
            in src)
    return c


def panel_lds_bytes(w, nbi, c, V=2, elem=8):
    """csrc/trsm.hip panel_lds_bytes<double>."""
    stage = c["TM_BK"] * (c["TM_SB"] + 16)
    return (c["TM_G"] * (w + V) + c["TM_G"] * (nbi + V) + 2 * stage) * elem


def fused_eligible(N, nbi, c, lds=LDS_BYTES):
    return panel_lds_bytes(-(-N // nbi) * nbi, nbi, c) <= lds


def fused_limit(nbi, c, lds=LDS_BYTES):
    """The largest N the one-launch solve serves."""
    N = nbi
    while fused_eligible(N + nbi, nbi, c, lds):
        N += nbi
    return N


@functools.lru_cache(maxsize=None)
def qp(n, m, p, seed):
    """The generated QP, made once per session and never modified."""
    return oracle.gen_qp(n, m, p, seed)


def oracles(c):
    n, m, p, B, seed0 = c
    return [oracle.OracleQP(qp(n, m, p, seed0 + i)) for i in range(B)]


@functools.lru_cache(maxsize=None)
def rhs(N, B):
    """(B, RHS_MAX, N) right-hand sides; a call with fewer rows uses the first ones.  Never modified."""
    r = np.random.default_rng(7000 + N).uniform(-1.0, 1.0, (B, RHS_MAX, N))
    r.setflags(write=False)
    return r


def sym(K):
    """The symmetric matrix from its lower triangle."""
    return K + np.tril(K, -1).T


def reference(K_lower, rows):
    """oracle.solve_ldlt of every row with the oracle's factor of sym(K_lower)."""
    L, D = oracle.ldlt(sym(K_lower))
    return np.stack([oracle.solve_ldlt(L, D, np.array(b)) for b in rows])


def row_err(X, X_ref):
    """max over rows of |x - x_ref|_inf / max(1, |x_ref|_inf); NaN counts as inf."""
    e = np.abs(X - X_ref).max(axis=-1) / np.maximum(1.0, np.abs(X_ref).max(axis=-1))
    e = np.where(np.isnan(e), np.inf, e)
    return float(e.max()) if e.size else 0.0
