"""Matrices and QPs that put the Bunch-Kaufman factor's pivot CHOICES under
test -- tied column maxima, the three threshold tests at equality and one ulp
off, non-finite entries, overflowing scales -- and a NumPy restatement of the
unblocked factor that records every decision it takes.  Shared by
tests/test_oracle_bk_pivot_cases.py (no GPU: the restatement equals the
oracle, every case hits what it claims), tests/test_gpu_bk_pivot_edges.py (the
device) and tests/golden/make_golden.py (the inputs of the bkp_* fixtures).

Everything here is deterministic; the seeds are the constants below.

factor_trace(K) restates LinearSolvers.cpp:76-207 with the expressions and
operand order of oracle/ipmz_oracle.cpp bk_factor (NumPy does not contract a
multiply and an add, so element by element it rounds as the oracle does; the
sign of a zero may differ where a sparse update skips x - 0).  One record per
pivot step:
  k, branch     "zero" (all-zero column), "keep1" (1x1 kept at the first
                test), "keep2" (1x1 kept at the second), "swap1" (1x1
                interchange), "2x2"
  ties          rows attaining colmax (0 when nothing compares > 0)
  row_search    imax was used
  eq1, eq2, eq3 None when the comparison was not evaluated, else whether it
                held with EQUALITY: akk == alpha colmax, akk rowmax == alpha
                colmax^2, |a(imax, imax)| == alpha rowmax
  imax, kp, kp_lt_k
  past_end      a 2x2 pivot at the last column (a NaN pivot): the reference
                indexes past the matrix -- no case here does
"""
import functools

import numpy as np

ALPHA = float.fromhex("0x1.47e0f66afed07p-1")  # (1 + sqrt(17)) / 8 as the oracle computes it at run time
BRANCHES = ("zero", "keep1", "keep2", "swap1", "2x2")


def _absmax(v):
    """The reference's strictly-greater scan from 0: (first index of the maximum, maximum, rows attaining it);
    NaN and zero never win, then (0, 0.0, 0)."""
    w = np.abs(v)
    w = np.where(w > 0, w, 0.0)
    if w.size == 0 or not (w.max() > 0):
        return 0, 0.0, 0
    m = w.max()
    return int(np.argmax(w)), float(m), int((w == m).sum())


def _rank_update(T, U, W):
    """T[i, j] -= sum_c U[c][i] * W[c][j] over the lower triangle (j <= i), each element with the reference's
    single expression; rows and columns whose factors are all exact zeros are skipped when everything is finite."""
    n = T.shape[0]
    fin = all(np.isfinite(x).all() for x in U + W)
    if fin and n > 400:
        nz = np.flatnonzero(np.any([x != 0 for x in U + W], axis=0))
        if nz.size == 0:
            return
        ix = np.ix_(nz, nz)
        U, W, sub = [x[nz] for x in U], [x[nz] for x in W], T[ix]
    else:
        ix, sub = None, T
    if len(U) == 1:
        upd = np.outer(U[0], W[0])  # f[j] * c_i
    else:
        upd = np.outer(U[0], W[0]) + np.outer(U[1], W[1])  # (u_i wk_j + v_i wk1_j)
    sub = sub - np.tril(upd)
    if ix is None:
        T[:, :] = sub
    else:
        T[ix] = sub


def factor_trace(K, fix_kp=False):
    """(F, ipiv int64, info, trace) of the reference's unblocked factor."""
    A = np.array(K, dtype=np.float64, copy=True, order="C")
    n = A.shape[0]
    ipiv = np.zeros(n, dtype=np.int64)
    info, trace, k = 0, [], 0
    with np.errstate(all="ignore"):
        while k < n:
            step, kp = 1, 0
            rec = dict(k=k, branch=None, ties=0, row_search=False, eq1=None, eq2=None, eq3=None, imax=0, kp=0,
                       kp_lt_k=False, past_end=False)
            akk = abs(A[k, k])
            i0, cmax, ties = _absmax(A[k + 1:, k])
            imax = i0 + k + 1 if cmax > 0 else 0
            rec["ties"], rec["imax"] = ties, imax
            if akk == 0.0 and cmax == 0.0:
                rec["branch"] = "zero"
                if info == 0:
                    info, kp = k, k
                elif fix_kp:
                    kp = k
            else:
                if akk >= ALPHA * cmax:
                    kp, rec["branch"] = k, "keep1"
                    rec["eq1"] = bool(akk == ALPHA * cmax)
                else:
                    rec["eq1"] = False
                    rec["row_search"] = True
                    r1 = _absmax(A[imax, k:imax])[1]  # (empty when imax < k)
                    r2 = _absmax(A[imax + 1:, imax])[1]
                    rmax = r2 if r1 < r2 else r1  # std::max
                    if akk * rmax >= ALPHA * cmax * cmax:
                        kp, rec["branch"] = k, "keep2"
                        rec["eq2"] = bool(akk * rmax == ALPHA * cmax * cmax)
                    else:
                        rec["eq2"] = False
                        kp = imax
                        if abs(A[imax, imax]) >= ALPHA * rmax:
                            rec["branch"] = "swap1"
                            rec["eq3"] = bool(abs(A[imax, imax]) == ALPHA * rmax)
                        else:
                            rec["branch"], rec["eq3"], step = "2x2", False, 2
                kk = k + step - 1
                rec["kp_lt_k"] = kp < k
                if kk >= n:
                    rec["past_end"] = True
                    trace.append(rec)
                    ipiv[k] = -kp
                    break
                if kp != kk:  # the symmetric interchange, in the reference's order
                    t = A[kp + 1:, kp].copy()
                    A[kp + 1:, kp] = A[kp + 1:, kk]
                    A[kp + 1:, kk] = t
                    if kp > kk + 1:
                        t = A[kp, kk + 1:kp].copy()
                        A[kp, kk + 1:kp] = A[kk + 1:kp, kk]
                        A[kk + 1:kp, kk] = t
                    A[kp, kp], A[kk, kk] = A[kk, kk], A[kp, kp]
                    if step == 2:
                        A[kk, k], A[kp, k] = A[kp, k], A[kk, k]
                j0 = k + step
                c0 = A[j0:, k].copy()
                if step == 1:
                    r = 1.0 / A[k, k]
                    f = r * c0
                    _rank_update(A[j0:, j0:], [c0], [f])
                    A[j0:, k] = c0 * r
                elif k < n - 1:
                    c1 = A[j0:, k + 1].copy()
                    d21 = A[k + 1, k]
                    d11 = A[k + 1, k + 1] / d21
                    d22 = A[k, k] / d21
                    t = 1.0 / (d11 * d22 - 1.0)
                    d21 = t / d21
                    wk = d21 * (d11 * c0 - c1)
                    wk1 = d21 * (d22 * c1 - c0)
                    _rank_update(A[j0:, j0:], [c0, c1], [wk, wk1])
                    A[j0:, k] = wk
                    A[j0:, k + 1] = wk1
            rec["kp"] = kp
            trace.append(rec)
            if step == 1:
                ipiv[k] = kp
            else:
                ipiv[k] = ipiv[k + 1] = -kp
            k += step
    return A, ipiv, info, trace


def tied_row_searches(trace):
    """Pivot steps that searched row imax with more than one row attaining colmax."""
    return sum(1 for r in trace if r["row_search"] and r["ties"] > 1)


# ---------------------------------------------------------------------------
# small_int: symmetric, entries in {-1, 0, 1} (span 1) or {-2 .. 2} (span 2), diagonal zero or integer.  Exact
# cancellation makes zero columns without help; ties are few after the first eliminations.
SMALL_INT = [  # (N, seed, span, zero diagonal)
    (1, 1, 1, False), (2, 2, 1, True), (2, 5, 2, False), (3, 3, 1, True), (3, 4, 2, False), (17, 17, 1, True),
    (17, 18, 2, False), (64, 64, 2, False), (65, 65, 1, True), (65, 66, 2, False), (130, 130, 1, True),
    (130, 131, 2, False), (300, 300, 1, True), (300, 301, 2, False),
]


def small_int(N, seed, span=1, zero_diag=False):
    rng = np.random.default_rng(seed)
    K = rng.integers(-span, span + 1, (N, N)).astype(np.float64)
    K = np.tril(K, -1) + np.tril(K, -1).T + np.diag(np.zeros(N) if zero_diag else np.diag(K))
    return K


# ---------------------------------------------------------------------------
# threshold: block-diagonal gadgets; each meets its first pivot step with its original values (decoupled blocks
# eliminate exactly).  colmax = 1 in every gadget; the 3x3 gadgets have rowmax = 2, the 2x2 gadgets rowmax = 1.
def _pred(x):
    return float(np.nextafter(x, 0.0))


# (name, akk, a(imax, imax), 3x3?, branch, which comparison, equality there)
GADGETS = [
    ("t1_eq", ALPHA, 3.0, False, "keep1", "eq1", True),
    ("t1_ulp", _pred(ALPHA), 0.25, False, "2x2", "eq1", False),
    ("t1_neg", -ALPHA, 3.0, False, "keep1", "eq1", True),
    ("t2_eq", ALPHA / 2, 5.0, True, "keep2", "eq2", True),
    ("t2_ulp", _pred(ALPHA / 2), 5.0, True, "swap1", "eq2", False),
    ("t3_eq", 0.125, 2 * ALPHA, True, "swap1", "eq3", True),
    ("t3_ulp", 0.125, _pred(2 * ALPHA), True, "2x2", "eq3", False),
    ("t3_neg", 0.125, -2 * ALPHA, True, "swap1", "eq3", True),
]
GADGET_ROWS = sum(3 if g[3] else 2 for g in GADGETS)  # 21


def gadget_offsets(base):
    out, o = [], base
    for g in GADGETS:
        out.append(o)
        o += 3 if g[3] else 2
    return out


def threshold(N, bases):
    """The gadget set at each base offset inside diag(10 + i) (distinct, nonzero: no zero column, no tie)."""
    K = np.diag(10.0 + np.arange(N))
    for base in bases:
        for o, (_, akk, d, three, *_rest) in zip(gadget_offsets(base), GADGETS):
            K[o, o], K[o + 1, o + 1] = akk, d
            K[o + 1, o] = K[o, o + 1] = 1.0
            if three:
                K[o + 2, o + 2] = 7.0
                K[o + 2, o + 1] = K[o + 1, o + 2] = 2.0
                K[o + 2, o] = K[o, o + 2] = 0.0
    return K


THRESHOLD_N = 1060
# sets whose gadgets straddle row 64 (t2_ulp at 63..65), row 1024 (t3_eq at 1023..1025) and the end of the matrix
THRESHOLD_BASES = (0, 64 - 9 + 2, 1024 - 12 + 1, THRESHOLD_N - GADGET_ROWS)


# ---------------------------------------------------------------------------
# spread_tie: diagonal 3 + i mod 7; pivot column k has a(k, k) = 1/8 and rows of magnitude exactly 1, mixed signs,
# far apart.  The FIRST tied row has diagonal 1/4 (< alpha rowmax: a 2x2 pivot), the others keep theirs (>= 3: a 1x1
# interchange), so any other choice among the tied rows changes ipiv.  The rows are placed so that the first one
# loses under every ordering but the smallest row index (wrong_order_winners).
SPREAD_N = 1290
SPREAD_COLUMNS = {  # k -> tied rows, ascending
    5: (647, 774, 840, 860, 927, 955, 992, 1266, 1280, 1288),
    70: (662, 752, 786, 792, 820, 852, 876, 880, 946, 990, 1284),
    200: (503, 594, 640, 665, 669, 715, 741, 980, 1000, 1004, 1245),
}


def spread_tie(ulp_column=None):
    """ulp_column = k: the first tied entry of column k one ulp below 1 (the tie broken the other way)."""
    N = SPREAD_N
    K = np.diag(3.0 + (np.arange(N) % 7))
    for k, rows in SPREAD_COLUMNS.items():
        K[k, k] = 0.125
        K[rows[0], rows[0]] = 0.25
        for t, r in enumerate(rows):
            v = -1.0 if t % 2 else 1.0
            if t == 0 and ulp_column == k:
                v = _pred(v)
            K[r, k] = K[k, r] = v
    return K


def wrong_order_winners(k, rows, groups=range(64, 321)):
    """The tied row each WRONG tie rule would pick: the lowest thread / wave of k_bk_factor's column scan (thread
    (i - k - 1) mod 1024), the largest row, and k_bk_grid's lowest owner i mod G for every G in groups (the smaller
    row among one owner's: each owner scans its rows ascending)."""
    thread = {r: (r - k - 1) % 1024 for r in rows}
    out = {"thread": min(rows, key=lambda r: (thread[r], r)), "wave": min(rows, key=lambda r: (thread[r] >> 6, r)),
           "lane": min(rows, key=lambda r: (thread[r] & 63, r)), "last": max(rows)}
    for G in groups:
        out[f"G{G}"] = min(rows, key=lambda r: (r % G, r))
    return out


# ---------------------------------------------------------------------------
# structured_qp: EqualityHandling::None QPs whose KKT matrices tie all the time: Q = I, c = +-1 alternating, C = 8 x
# incidence rows (one +8, one -8), d = 0, A three ones per row with bounds +-1, box [-1, 1].  oracle.gen_qp's layout.
# The seeds are the first ones whose KKT matrices at iterates 0-3 take at least 2 (n = 40) / 10 (n >= 300) row
# searches with a tied column maximum, stay below a condition number of 1e3, and converge within 12 iterations.
STRUCTURED = [(40, 8, 12, 12), (40, 0, 12, 12), (300, 40, 100, 13), (700, 60, 200, 14)]  # n, m, p, seed
STRUCTURED_BATCH = {40: (40, 8, 12, (16, 17, 18, 22)), 300: (300, 40, 100, (11, 12, 15, 17))}  # n -> n, m, p, seeds
STRUCTURED_MIN_TIES = {40: 2, 300: 10, 700: 10}


def structured_qp(n, m, p, seed):
    rng = np.random.default_rng(seed)
    C = np.zeros((p, n))
    for r in range(p):
        i, j = rng.choice(n, 2, replace=False)
        C[r, i], C[r, j] = 8.0, -8.0
    A = np.zeros((m, n))
    for r in range(m):
        A[r, rng.choice(n, 3, replace=False)] = 1.0
    c = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return dict(n=n, m=m, p=p, Q=np.eye(n), c=c, A=A, lA=-np.ones(m), uA=np.ones(m), C=C, d=np.zeros(p),
                lx=-np.ones(n), ux=np.ones(n))


# ---------------------------------------------------------------------------
# nonfinite
def kp_lt_k(N, arrow=False, at=5):
    """A NaN diagonal over a zero column at k = at: colmax = 0, imax = 0, no comparison holds, kp = imax = 0 < k.
    arrow: column 0 is nonzero below the diagonal (except row at, which keeps column at zero), so the backward
    interchange moves a finished column of L into the pivot column.  The interchange's loop meets the diagonal
    a(k, k) in row k, thread k - 1 of k_bk_factor: beyond the first wave from at = 65 on."""
    K = np.diag(np.arange(1.0, N + 1))
    if arrow:
        K[0, 0] = 4.0
        K[1:, 0] = K[0, 1:] = 1.0
        K[at, 0] = K[0, at] = 0.0
    K[at, at] = np.nan
    return K


KP_LT_K = {  # name -> N, arrow, at
    "kp_lt_k8": (8, False, 5), "kp_lt_k600": (600, False, 5), "kp_lt_k_arrow40": (40, True, 5),
    "kp_lt_k_arrow600": (600, True, 5), "kp_lt_k600_at300": (600, False, 300),
    "kp_lt_k_arrow600_at300": (600, True, 300),
}


def _nonfinite(N, seed, kind, jd):
    K = small_int(N, seed, 2, False)
    i, j = (N // 3, N // 2)
    if kind == "nan_pair":
        K[i, j] = K[j, i] = np.nan
    elif kind == "inf_pair":
        K[i, j] = K[j, i] = np.inf
    else:  # a NaN diagonal with a nonzero column under it
        K[jd, jd] = np.nan
        K[N - 1, jd] = K[jd, N - 1] = 2.0
    return K


# N, seed of the small_int matrix underneath, the NaN diagonal's position (NaN fills the trailing matrix and the
# rest are 2x2 pivots with kp = 0: the position makes them end on the last column, not past it)
NONFINITE = [(33, 33, 16), (65, 67, 34)]
SCALES = (600, -600, -1040)  # small_int(65, seed 66, span 2) times 2**e: alpha colmax^2 overflows / underflows


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (family, K, has non-finite entries in K or F).  Read-only."""
    out = {}
    for N, seed, span, zd in SMALL_INT:
        out[f"small_int{N}_s{seed}"] = ("small_int", small_int(N, seed, span, zd), False)
    out["threshold21"] = ("threshold", threshold(GADGET_ROWS, (0,)), False)
    out[f"threshold{THRESHOLD_N}"] = ("threshold", threshold(THRESHOLD_N, THRESHOLD_BASES), False)
    out["spread_tie"] = ("spread_tie", spread_tie(), False)
    for N, seed, jd in NONFINITE:
        for kind in ("nan_pair", "inf_pair", "nan_diag"):
            out[f"{kind}{N}"] = ("nonfinite", _nonfinite(N, seed, kind, jd), True)
    for name, args in KP_LT_K.items():
        out[name] = ("nonfinite", kp_lt_k(*args), True)
    for e in SCALES:
        out[f"scaled65_2e{e}"] = ("scaled", small_int(65, 66, 2, False) * 2.0 ** e, True)
    for _, K, _ in out.values():
        K.setflags(write=False)
    return out


def names(family=None):
    return [n for n, c in cases().items() if family is None or c[0] == family]


@functools.lru_cache(maxsize=None)
def oracle_factor(name):
    """oracle.bk_factor of the case: (F, ipiv int32, info).  Made once, read-only."""
    import oracle
    F, piv, info = oracle.bk_factor(cases()[name][1])
    piv = piv.astype(np.int32)
    F.setflags(write=False)
    piv.setflags(write=False)
    return F, piv, int(info)


@functools.lru_cache(maxsize=None)
def traced(name):
    return factor_trace(cases()[name][1])


# the fixtures of tests/golden/ (make_golden.py writes <tag>_K.bin and <tag>_b.bin, the reference the rest)
GOLDEN = {"bkp_thr21": "threshold21", "bkp_int17": "small_int17_s18", "bkp_int64": "small_int64_s64",
          "bkp_kplt8": "kp_lt_k8"}


def golden_rhs(N):
    return np.random.default_rng(7000 + N).integers(-4, 5, N).astype(np.float64)
