"""Tangents of the problem data, the independent reference and the case tables of the forward-mode sensitivities
(ipmz_batch_data_jvp: Optimizer.data_jvp_tensors; ipmz_amd.layer.solution_jvp), shared by
tests/test_gpu_data_jvp.py, tests/test_gpu_qp_jvp.py (the device) and tests/test_oracle_data_jvp.py (what the
reference relies on, no GPU).

The reference is the formulation's own "shorthand definitions" (dc.residuals_form, tests/golden/formulations.txt)
in longdouble: r is affine in the data at a fixed iterate and mu, so r(D) - r(0) -- the tangents as data minus
all-zero data -- is exactly its linear part.  Neither the device nor grad.hip's / jvp.hip's coefficients enter.
"""
import functools

import numpy as np

import data_vjp_cases as dc
import newton_multi_cases as nc

NTANS = nc.RHS_COUNTS                            # (1, 3, 17, 6)
SHAPES = [(12, 5, 3), (48, 16, 8), (130, 40, 22)]  # the last: partial M / N tiles and an odd tile count
M0_SHAPES = [(40, 0, 8), (40, 5, 0), (40, 0, 0)]   # m = 0 (dc.M0_FORMS only), p = 0, both
BATCHES = (1, 2, 3, 5, 17)                       # at SHAPES[0]: every residue of the K tail, a partial N tile
BLOCK_SHAPE = {"Q": ("n", "n"), "A_ineq": ("m", "n"), "A_eq": ("p", "n"), "c": ("n",), "l_x": ("n",), "u_x": ("n",),
               "l_A_ineq": ("m",), "u_A_ineq": ("m",), "b_eq": ("p",)}

# csrc/kernels.h, csrc/jvp.hip (tests/test_oracle_data_jvp.py reads them off the sources)
ROWS_GY = 16384   # IPMZ_JVP_ROWS_GY: gridDim.y of the launches that loop over the rows (q, t)
PAIR_COLS = 128   # columns of one pair per lane: a column tile is PAIR_COLS * pairs(n) columns
WAVES = 4         # waves of a workgroup of k_jvp_matrix: a wave takes rows w, w + 4, ... two at a time
FILL = 256        # workgroups one row (q, t) should have before the row chunk grows past 8
KSTEP = 32        # k per pass of k_jvp_shared's K loop (the chunk staged through LDS)


def pairs(n):
    """jvp_pairs: column pairs per lane of k_jvp_matrix's column tile."""
    return 1 if n <= 128 else 2 if n <= 256 else 4


def plan(n, rows):
    """qp_jvp_plan for a per-QP matrix block of `rows` rows: (column tiles, rows per chunk, chunks)."""
    ct = PAIR_COLS * pairs(n)
    nct = -(-n // ct)
    rch = 32
    while rch > 8 and -(-rows // rch) * nct < FILL:
        rch //= 2
    return nct, rch, -(-rows // rch)


# Every loop of jvp.hip with the smallest case that reaches it: (id, (n, m, p), batch, ntan, what).  One loop is out
# of reach of any shape a solver here is built for and has no case: the element loop of k_jvp_rows (max(n, m, p) >
# 256 * 2048).
LOOPS = [
    # rows per chunk 16 (ceil(n / 16) * 3 tiles >= 256): a wave's row-pair loop makes a second pass; three column
    # tiles: k_jvp_rows' loop over the tiles' row partials; A's 5 rows: one chunk
    ("pairs_nct", (1361, 5, 3), 1, 1, "k_jvp_matrix row pairs (rch 16), k_jvp_rows nct 3"),
    # rows per chunk 32 (ceil(n / 32) * 4 tiles >= 256): four passes
    ("rch32", (2017, 5, 3), 1, 1, "k_jvp_matrix row pairs (rch 32), nct 4"),
    # more rows (q, t) than gridDim.y: the row loops of k_jvp_matrix and k_jvp_rows
    ("rows_gy", (12, 5, 3), 964, 17, "batch * ntan = 16388 > IPMZ_JVP_ROWS_GY"),
    # the column tile's width changes at n = 128 | 129 and 256 | 257; m = 16 > 8 rows: two chunks of A's column
    # sums (k_jvp_rows' loop over the chunks); K = n > 32: k_jvp_shared's K loop (shared layout)
    ("np1_edge", (128, 16, 3), 2, 3, "pairs 1, last full tile"),
    ("np2_edge", (129, 16, 3), 2, 3, "pairs 2, odd n"),
    ("np2_full", (256, 16, 3), 2, 3, "pairs 2, last full tile"),
    ("np4_edge", (257, 16, 3), 2, 3, "pairs 4, odd n"),
]


@functools.lru_cache(maxsize=None)
def tangents(n, m, p, ntan, B, seed=0):
    """name -> (B, ntan, ...) standard-normal tangents of every block the shape has; B None: (ntan, ...), one set
    shared by every QP."""
    rng = np.random.default_rng(7100 + 31 * ntan + 7 * (B or 0) + seed + n)
    d = dict(n=n, m=m, p=p)
    out = {}
    for k in dc.present(n, m, p):
        shape = tuple(d[s] for s in BLOCK_SHAPE[k])
        a = rng.standard_normal(((ntan,) if B is None else (B, ntan)) + shape)
        a.setflags(write=False)
        out[k] = a
    return out


def one(D, t, q=None):
    """Tangent t (of QP q, for per-QP tangents) of every block."""
    return {k: (a[t] if q is None else a[q, t]) for k, a in D.items()}


def _data(shape_of, D):
    """The QP dict residuals_form reads, in longdouble, with the tangents as data (absent blocks: zeros)."""
    n, m, p = shape_of
    d = dict(n=n, m=m, p=p)
    out = dict(n=n, m=m, p=p)
    for k, key in dc.KEYS.items():
        shape = tuple(d[s] for s in BLOCK_SHAPE[k])
        out[key] = dc.ld(D[k]) if k in D and D[k] is not None else np.zeros(shape, dtype=np.longdouble)
    return out


def jvp_reference(name, q, v, D, mu=0.0):
    """One row of R: (d r / d data) D at the iterate v of a served formulation, D: name -> one tangent (missing:
    zero).  dc.residuals_form on longdouble copies with the tangents as data, minus the same with all-zero data,
    cast to float64.  q gives the dimensions only."""
    shape = (q["n"], q["m"], q["p"])
    vl = dc.ld(v)
    r1 = dc.residuals_form(name, _data(shape, D), vl, np.longdouble(mu))
    r0 = dc.residuals_form(name, _data(shape, {}), vl, np.longdouble(mu))
    return np.asarray(r1 - r0, dtype=np.float64)


def zero_slots(name, n, m, p):
    """Index array of the slots no datum enters: r_s, r_p and the complementarity rows of the slacked forms."""
    order, sz, off, L = dc.form_offsets(name, n, m, p)
    idx = [np.arange(off[s], off[s] + sz[s]) for s in order if s in ("s", "p", "g", "h", "y", "z")]
    return np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)


def row_err(R, ref):
    """max over rows of |R - ref|inf / max(1, |ref|inf)."""
    R, ref = np.asarray(R), np.asarray(ref)
    R, ref = R.reshape(-1, R.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return max(dc.rel_err(a, b) for a, b in zip(R, ref))
