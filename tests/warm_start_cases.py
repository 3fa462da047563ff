"""The warm start's push and check restated in numpy (ipmz_batch_set_state_device: Optimizer.set_state_tensor),
shared by tests/test_gpu_warm_start.py (the device) and tests/test_abi_warm_start.py (the self-test below, no GPU).
No GPU work here.

A row is an iterate in the reference's Newton order, what state(q) / state_tensor() return.  Its layout comes from
tests/batch_form_cases.py's formulations and oracle.newton_order / oracle.slot_size (tests/golden/formulations.txt);
the equality-slack formulations use oracle.EqSlackedOracle's order.  What the step length (ratio_elem, newton.hip)
needs of an iterate decides the class of every index:

  PUSHED  a slot kept non-negative: lambda_g, lambda_h, lambda_y, lambda_z (lambda_v, lambda_w) and, where they are
          Newton variables, g, h, y, z (v, w).  push: v < floor -> floor.  Violation: not v > 0 (so a NaN is one).
  XBOUND  x where neither g nor h is a Newton variable -- InequalityHandling::Slacks, or no inequality row at all
  SBOUND  (the box-only quirk): violation unless l_x < x < u_x; likewise s against l_A, u_A.
  FREE    everything else (x otherwise, s, lambda_A, lambda_C, p, t): only a NaN is a violation.
"""
import collections

import numpy as np

import batch_form_cases as fc
import ipmz_amd as I
import oracle

FREE, PUSHED, XBOUND, SBOUND = 0, 1, 2, 3
SHAPE = (48, 16, 8)   # n, m, p: every loop a single pass, N 72 / 88 / 96 (fc.S1)
BOX_SHAPE = (5, 0, 0)  # no inequality row: explicit bounds on x in every formulation
BOX_FORMS = ("box", "vlo", "vnone", "sl", "eqss")  # (of fc.S0_FORMS)
BATCH = 5
SEED0 = 7
_PUSHED_NAMES = {"lambda_g", "lambda_h", "lambda_v", "lambda_w", "lambda_y", "lambda_z", "g", "h", "v", "w", "y", "z"}

Layout = collections.namedtuple("Layout", "names sizes offsets kind idx L explicit")


def _flags(form):
    kw = fc.FORMS[form].kw
    ih = kw.get("inequality_handling", I.INEQ_SLACKED_SLACKS)
    eq = kw.get("equality_handling", I.EQ_REGULARIZATION)

    def bits(b):  # IPMZ_BOUNDS_* -> oracle.BOUNDS
        return {I.BOUNDS_BOTH: 3, I.BOUNDS_LOWER: 1, I.BOUNDS_UPPER: 2, I.BOUNDS_NONE: 0}[b]

    f = oracle.Form(ih == I.INEQ_SLACKS, bits(kw.get("inequality_bounds", I.BOUNDS_BOTH)),
                    bits(kw.get("variable_bounds", I.BOUNDS_BOTH)), ih == I.INEQ_NAIVE_SLACKS)
    return f, eq


def layout(form, n, m, p):
    """The caller's row of formulation `form` (a key of fc.FORMS): slot names, sizes and offsets in order, and per
    index its class and its index within the slot."""
    f, eq = _flags(form)
    if eq in (I.EQ_SLACKED_SLACKS, I.EQ_NAIVE_SLACKS):
        naive = eq == I.EQ_NAIVE_SLACKS
        sizes = collections.OrderedDict(
            x=n, lambda_A=0 if naive else m, lambda_C=0 if naive else p, s=0 if naive else m, t=0 if naive else p,
            lambda_g=m, lambda_h=m, lambda_v=p, lambda_w=p, lambda_y=n, lambda_z=n, g=m, h=m, v=p, w=p, y=n, z=n)
        rows = m + p  # the equality rows run as inequality rows
    else:
        no_p = eq in (I.EQ_NONE, I.EQ_PENALTY)
        sizes = collections.OrderedDict((s, oracle.slot_size(s, n, m, p, no_p, f))
                                        for s in oracle.newton_order(n, m, p, no_p, f))
        rows = m
    names = [s for s in sizes if sizes[s]]
    explicit = f.slacks or rows == 0
    kind, idx, offsets, off = [], [], {}, 0
    for s in names:
        k = PUSHED if s in _PUSHED_NAMES else XBOUND if explicit and s == "x" else SBOUND if explicit and s == "s" else FREE
        kind += [k] * sizes[s]
        idx += list(range(sizes[s]))
        offsets[s] = off
        off += sizes[s]
    return Layout(names, dict(sizes), offsets, np.array(kind, dtype=np.int8), np.array(idx), off, explicit)


def push(V, lay, floor):
    """The rows after the interior push: every PUSHED component below floor becomes floor; nothing else moves."""
    V = np.array(V, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        V[..., :] = np.where((lay.kind == PUSHED) & (V < floor), floor, V)
    return V


def violations(V, lay, bounds=None):
    """(B, L) bool: the components of the (already pushed) rows V the check refuses.  bounds: dict of (B, n) lx, ux
    and (B, m) lA, uA -- needed where lay.explicit."""
    V = np.asarray(V, dtype=np.float64)
    bad = np.isnan(V)
    with np.errstate(invalid="ignore"):
        bad |= (lay.kind == PUSHED) & ~(V > 0.0)
        for kind, lo, up in ((XBOUND, "lx", "ux"), (SBOUND, "lA", "uA")):
            cols = np.nonzero(lay.kind == kind)[0]
            if cols.size:
                i = lay.idx[cols]
                v = V[:, cols]
                bad[:, cols] |= ~((bounds[lo][:, i] < v) & (v < bounds[up][:, i]))
    return bad


def first_offender(V, lay, floor, bounds=None, take=None):
    """(QP, index) of the smallest violation among the taken rows after the push, or None."""
    bad = violations(push(V, lay, floor), lay, bounds)
    if take is not None:
        bad &= (np.asarray(take) != 0)[:, None]
    hits = np.argwhere(bad)  # row-major: sorted by (QP, index)
    return None if hits.size == 0 else (int(hits[0, 0]), int(hits[0, 1]))


def qp_bounds(shape, B=BATCH, seed0=SEED0):
    """The bounds of the QPs Batch.generate(seed0) makes (fc.qp), stacked; the merged rows' l_A, u_A are not needed:
    s is bounded only under InequalityHandling::Slacks, which has no equality-slack form."""
    qs = [fc.qp(tuple(shape), seed0 + i) for i in range(B)]
    return {k: np.stack([q[k] for q in qs]) for k in ("lx", "ux", "lA", "uA")}


def perturbed(V, lay, bounds, seed=11):
    """V moved deterministically and kept interior: PUSHED components scaled by 1 .. 1.25, bounded ones moved by at
    most a quarter of their distance to the nearer bound, free ones by at most 5e-4."""
    V = np.array(V, dtype=np.float64)
    u = np.random.default_rng(seed).uniform(0.0, 1.0, V.shape)
    out = V + 1e-3 * (u - 0.5)
    pm = lay.kind == PUSHED
    out[:, pm] = V[:, pm] * (1.0 + 0.25 * u[:, pm])
    for kind, lo, up in ((XBOUND, "lx", "ux"), (SBOUND, "lA", "uA")):
        cols = np.nonzero(lay.kind == kind)[0]
        if cols.size:
            i = lay.idx[cols]
            v = V[:, cols]
            room = np.minimum(v - bounds[lo][:, i], bounds[up][:, i] - v)
            out[:, cols] = v + 0.5 * (u[:, cols] - 0.5) * room
    return out


def self_test():
    """Hand-made rows through layout, push, violations and first_offender."""
    # the default formulation at n = 2, m = 1, p = 1: x2 lambda_A lambda_C s p lambda_g lambda_h lambda_y2 lambda_z2 g h y2 z2
    lay = layout("box", 2, 1, 1)
    assert lay.names == ["x", "lambda_A", "lambda_C", "s", "p", "lambda_g", "lambda_h", "lambda_y", "lambda_z", "g", "h",
                         "y", "z"]
    assert lay.L == 18 and not lay.explicit
    assert lay.kind.tolist() == [FREE] * 6 + [PUSHED] * 12
    row = np.arange(1.0, 19.0)
    V = np.stack([row, row, row])
    assert first_offender(V, lay, 0.0) is None
    V[2, 7] = 0.0      # lambda_h: zero
    V[1, 9] = -1.0     # lambda_y[1]: negative
    V[1, 3] = -5.0     # s: free, negative is fine
    V[1, 17] = np.nan  # z[1]
    V[0, 1] = -0.0     # lambda_A: free
    assert first_offender(V, lay, 0.0) == (1, 9)
    assert first_offender(V, lay, 0.0, take=[1, 0, 1]) == (2, 7)
    assert first_offender(V, lay, 0.0, take=[1, 0, 0]) is None
    assert first_offender(V, lay, 0.5) == (1, 17)  # the push cures zero and negative, not a NaN
    P = push(V, lay, 0.5)
    assert P[2, 7] == 0.5 and P[1, 9] == 0.5 and P[1, 3] == -5.0 and np.isnan(P[1, 17])
    assert np.array_equal(P[0], row * np.where(np.arange(18) == 1, -0.0, 1.0)) and np.signbit(P[0, 1])
    V[0, 0] = np.nan   # x: a NaN in a free slot
    assert first_offender(V, lay, 0.5) == (0, 0)
    # floor 0 changes nothing where no pushed component is negative (not even -0.0 <-> 0.0); a negative one becomes 0
    # and stays a violation
    P0 = push(V, lay, 0.0)
    assert np.array_equal(P0[[0, 2]], V[[0, 2]], equal_nan=True) and np.signbit(P0[0, 1])
    assert P0[1, 9] == 0.0 and first_offender(V[1:2], lay, 0.0) == (0, 9)
    # NaiveSlacks: the duals ahead of lambda_C, no s
    lay = layout("naive", 2, 1, 1)
    assert lay.names == ["x", "lambda_g", "lambda_h", "lambda_C", "p", "lambda_y", "lambda_z", "g", "h", "y", "z"]
    assert lay.kind.tolist() == [FREE] * 2 + [PUSHED] * 2 + [FREE] * 2 + [PUSHED] * 10
    # the equality-slack forms in the reference's order (oracle.EqSlackedOracle)
    lay = layout("eqss", 2, 1, 1)
    assert lay.names == ["x", "lambda_A", "lambda_C", "s", "t", "lambda_g", "lambda_h", "lambda_v", "lambda_w", "lambda_y",
                         "lambda_z", "g", "h", "v", "w", "y", "z"] and lay.L == 22 and not lay.explicit
    assert lay.kind.tolist() == [FREE] * 6 + [PUSHED] * 16
    assert layout("naiveeq", 2, 1, 1).kind.tolist() == [FREE] * 2 + [PUSHED] * 16
    # Slacks: no g, h, y, z; x and s inside explicit bounds
    lay = layout("sl", 2, 1, 1)
    assert lay.names == ["x", "lambda_A", "lambda_C", "s", "p", "lambda_g", "lambda_h", "lambda_y", "lambda_z"]
    assert lay.explicit and lay.kind.tolist() == [XBOUND] * 2 + [FREE] * 2 + [SBOUND] + [FREE] + [PUSHED] * 6
    b = dict(lx=np.array([[-1.0, -1.0]] * 2), ux=np.array([[1.0, 2.0]] * 2), lA=np.array([[0.0]] * 2), uA=np.array([[3.0]] * 2))
    V = np.array([[0.0, 1.5, 9.0, 9.0, 1.0, 9.0] + [1.0] * 6] * 2)
    assert first_offender(V, lay, 0.0, b) is None
    V[1, 4] = 3.0  # s on its upper bound
    V[1, 1] = 2.0  # x[1] on its upper bound
    assert first_offender(V, lay, 0.0, b) == (1, 1)
    V[0, 0] = -1.0  # x[0] on its lower bound
    assert first_offender(V, lay, 0.0, b) == (0, 0)
    # the box-only quirk: no inequality row -> explicit bounds in the default formulation too, and without bounds on x
    for form in BOX_FORMS:
        lay = layout(form, *BOX_SHAPE)
        assert lay.explicit and lay.kind[:5].tolist() == [XBOUND] * 5, form
    assert layout("vnone", *BOX_SHAPE).L == 5
    # perturbed stays interior
    lay = layout("sl", 2, 1, 1)
    V = np.array([[0.0, 1.5, 9.0, 9.0, 1.0, 9.0] + [1.0] * 6] * 2)
    W = perturbed(V, lay, b)
    assert first_offender(W, lay, 0.0, b) is None and not np.array_equal(W, V)
