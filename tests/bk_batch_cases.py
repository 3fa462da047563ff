"""Matrices, right-hand sides, reference and error measure of the batched
multi-right-hand-side Bunch-Kaufman solve (ipmz_bk_factor_batch,
ipmz_bk_prepare_solve_batch, ipmz_bk_solve_multi_batch,
ipmz_batch_kkt_solve_bk), shared by tests/test_gpu_bk_batch_multi.py (the
device) and tests/test_oracle_bk_batch_cases.py (what the batches rely on,
without a GPU).

Reference: oracle.bk_solve on oracle.bk_factor's F and ipiv, row by row --
what the device factor is bitwise.  Tolerance: the project's rule for blocked
solves, |x - x_ref|_inf < 1e-10 max(1, |x_ref|_inf) per row (DX_TOL).  On every
matrix of BATCHES a CPU LU solve (other pivoting, other summation order)
differs from the oracle by at most 3.2e-12 in that measure (the worst case is
kktz(700, 340, seed 500)): the reference alone sits 30x inside the bound.

The generated IPMZ_EQ_NONE QPs take no 2x2 pivot and no interchange at all
(their x block dominates), so constructed matrices drive the interchange
folding, the 2x2 D solves and the fallback; the QP-level tests are about
plumbing.  The two generators restate those of tests/test_gpu_bk_multi.py.
"""
import functools
import os
import re

import numpy as np

import oracle

TOL = 1e-10  # DX_TOL of tests/test_gpu_parity.py
LU_MARGIN = 3.2e-12  # the largest LU-vs-oracle difference over the matrices named here
MULTI_BLOCKED, MULTI_W512, MULTI_W128 = 65536, 131072, 262144  # csrc/kernels.h IPMZ_DEBUG_MULTI_*
RHS_COUNTS = (1, 3, 16, 17, 33)  # looped: 1, 3; one full group of 16; a one-row second group; a third group
RHS_MAX = max(RHS_COUNTS)
LDS_BYTES = 160 * 1024  # LDS a workgroup may use on an MI355X
BK_GRID_MIN = 512  # csrc/kernels.h IPMZ_BK_GRID_MIN: below it ipmz_bk_solve is the one-workgroup kernel on F

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipm-zoo_amd", "csrc")


def _indef(N, seed, zeros=0):
    rng = np.random.default_rng(seed)
    K = rng.uniform(-1, 1, (N, N))
    K = np.tril(K) + np.tril(K, -1).T
    K[np.arange(N), np.arange(N)] *= 0.05
    for z in range(zeros):
        K[N // 2 + z, :] = 0
        K[:, N // 2 + z] = 0
    return K


def _kkt_zero_block(n, m, seed):
    # [[H, B^T], [B, 0]]: the zero block forces interchanges and 2x2 pivots
    rng = np.random.default_rng(seed)
    H = rng.uniform(-1, 1, (n, n))
    H = H + H.T
    H[np.arange(n), np.arange(n)] *= 0.01  # weak diagonal: interchanges and 2x2 pivots
    B = rng.uniform(-1, 1, (m, n))
    K = np.zeros((n + m, n + m))
    K[:n, :n] = H
    K[n:, :n] = B
    K[:n, n:] = B.T
    return K


# name -> the matrices of the batch, each ("indef", N, seed, zeros) or ("kktz", n, m, seed)
BATCHES = {
    "indef72": [("indef", 72, s, 0) for s in (300, 301, 302)],     # one block + 8 columns
    "indef192": [("indef", 192, s, 0) for s in (300, 301, 302)],   # a pair across a block edge in some systems only
    "indef321": [("indef", 321, s, 0) for s in (300, 301, 302)],   # odd N; ldb = 322; a one-column last block
    "kktz832": [("kktz", 560, 272, s) for s in (500, 502)],        # largest fused order; a pair across a panel edge
    "indef834": [("indef", 834, s, 0) for s in (300, 302)],        # first order past the fused limit
    "indef1040": [("indef", 1040, s, 0) for s in (301, 302)],      # panels: 4 panels + 16 columns
}
SINGULAR = [("indef", 321, 300, 0), ("indef", 321, 301, 2), ("indef", 321, 302, 0)]  # info = [0, 161, 0]
SINGULAR_INFO = [0, 161, 0]  # oracle.bk_factor's word: the reference's 0-based info = k of the first zero column met
# The device reports 1 + that column, as ipmz_bk_factor does (tests/test_gpu_bk.py: info == info_oracle + 1).
# Column 160 of the matrix is zero too, but the 2x2 pivot at (159, 160) interchanges it away to row 274
# before the factorization reaches it: the first all-zero column it meets is 161.
SINGULAR_DEVICE_INFO = [0, 162, 0]
LU_WORST = ("kktz", 700, 340, 500)  # the matrix of the 3.2e-12 figure
FUSED_LIMIT = 832  # what BATCHES assumes; fused_limit() derives it from the source


def order(key):
    return key[1] if key[0] == "indef" else key[1] + key[2]


def ldb_of(N):
    """The smallest even row stride."""
    return N + (N & 1)


@functools.lru_cache(maxsize=None)
def system(key):
    """K, the oracle's factor of it (F, ipiv int32, info).  Made once, never modified."""
    K = _indef(*key[1:]) if key[0] == "indef" else _kkt_zero_block(*key[1:])
    F, piv, info = oracle.bk_factor(K)
    piv = piv.astype(np.int32)
    for a in (K, F, piv):
        a.setflags(write=False)
    return K, F, piv, int(info)


@functools.lru_cache(maxsize=None)
def rhs(N, B):
    """(B, RHS_MAX, N) right-hand sides, uniform(-1, 1); a call with fewer rows uses the first ones."""
    r = np.random.default_rng(9000 + N).uniform(-1.0, 1.0, (B, RHS_MAX, N))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def reference(key, q, B):
    """oracle.bk_solve of the RHS_MAX rows rhs(N, B)[q] with the oracle's factor of system(key)."""
    _, F, piv, _ = system(key)
    with np.errstate(all="ignore"):
        X = np.stack([oracle.bk_solve(F, piv, np.array(b)) for b in rhs(order(key), B)[q]])
    X.setflags(write=False)
    return X


def batch_reference(keys):
    return np.stack([reference(k, q, len(keys)) for q, k in enumerate(keys)])


def pair_starts(piv):
    out, k = [], 0
    while k < len(piv):
        if piv[k] < 0:
            out.append(k)
            k += 2
        else:
            k += 1
    return out


def interchanges(piv):
    """Pivot steps whose row is exchanged with a later one."""
    n, k = 0, 0
    while k < len(piv):
        if piv[k] < 0:
            n += -piv[k] != k + 1
            k += 2
        else:
            n += piv[k] != k
            k += 1
    return n


def row_err(X, X_ref):
    """max over rows of |x - x_ref|_inf / max(1, |x_ref|_inf); NaN counts as inf."""
    e = np.abs(X - X_ref).max(axis=-1) / np.maximum(1.0, np.abs(X_ref).max(axis=-1))
    e = np.where(np.isnan(e), np.inf, e)
    return float(e.max()) if e.size else 0.0


def trsm_constants():
    """The tile constants of csrc/trsm.hip the one-launch solve's LDS follows from."""
    with open(os.path.join(CSRC, "trsm.hip")) as f:
        src = f.read()
    c = {k: int(re.search(rf"constexpr int {k} = (\d+);", src).group(1)) for k in ("TM_G", "TM_SB", "TM_BK")}
    assert re.search(r"constexpr int TM_PADN = TM_SB \+ 16;", src)
    assert re.search(r"constexpr int TM_STAGE = TM_BK \* TM_PADN;", src)
    assert ("return (size_t)(TM_G * (w + Mfma<T>::V) + TM_G * (nbi + Mfma<T>::V) + 2 * TM_STAGE) * sizeof(T);"
            in src)
    # the Bunch-Kaufman one-launch solve is eligible as the LDL^T one with inner block TM_SB
    assert "bool bk_solve_fused_eligible(int N) { return ldlt_solve_fused_eligible(N, TM_SB); }" in src
    return c


def fused_limit(lds=LDS_BYTES):
    """The largest N the one-launch solve serves (slab + T + two stage buffers within the LDS)."""
    c = trsm_constants()
    nbi, V = c["TM_SB"], 2
    stage = c["TM_BK"] * (c["TM_SB"] + 16)

    def need(w):
        return (c["TM_G"] * (w + V) + c["TM_G"] * (nbi + V) + 2 * stage) * 8

    N = nbi
    while need(N + nbi) <= lds:
        N += nbi
    return N


def crossover():
    """BK_BATCH_MULTI_CROSSOVER of csrc/capi.cpp: the row count from which the blocked paths run."""
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        return int(re.search(r"static constexpr int BK_BATCH_MULTI_CROSSOVER = (\d+);", f.read()).group(1))
