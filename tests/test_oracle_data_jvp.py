"""What the device tests of ipmz_batch_data_jvp rely on, checked without a GPU: jvp_reference (the formulation's
shorthand definitions with the tangents as data, tests/data_jvp_cases.py) is the linear part of the residuals in the
data and the transpose of dc.reference_form, for every served formulation and all nine blocks at once; the loop
table's cases reach the loops they claim by the kernels' own constants; and the entry point exists and refuses a
null solver before it looks for a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import data_jvp_cases as jc
import data_vjp_cases as dc
import newton_multi_cases as nc

MU = 0.3  # any fixed mu: it cancels in the linear part; 0 would hide PenaltyFunction's and Slacks' mu terms
CASES = [(name, c) for name in dc.FORM_NAMES for c in jc.SHAPES + jc.M0_SHAPES if c[1] or name in dc.M0_FORMS]


def _case(name, c, seed=0):
    q = nc.qp(*c)
    L = dc.form_offsets(name, *c)[3]
    rng = np.random.default_rng(400 + seed + c[0])
    v = rng.standard_normal(L)
    D = jc.one(jc.tangents(*c, 3, None), seed % 3)
    return q, L, v, D


def _gap(name, c, v, w, ref, D, grads=None):
    grads = dc.reference_form(name, *c, v, w) if grads is None else grads
    lhs = np.sum(dc.ld(w) * dc.ld(ref))
    rhs = sum(np.sum(dc.ld(grads[k]) * dc.ld(D[k])) for k in D)
    return float(abs(lhs - rhs)), nc.TOL * float(np.sum(np.abs(w) * np.abs(ref)))


@pytest.mark.parametrize("name", dc.FORM_NAMES)
def test_reference_is_the_transpose_of_the_vjp_reference(name):
    """<w, jvp_ref(D)> = sum <reference_form(w), D>, all blocks at once."""
    worst = 0.0
    for c in jc.SHAPES[:2]:
        q, L, v, D = _case(name, c)
        assert set(D) == set(dc.present(*c))
        ref = jc.jvp_reference(name, q, v, D, MU)
        assert ref.shape == (L,) and not ref[jc.zero_slots(name, *c)].any()
        for k in range(2):
            w = dc.cotangents(L, 2)[k]
            gap, bound = _gap(name, c, v, w, ref, D)
            assert bound > 0
            worst = max(worst, gap / bound)
    print(f"{name}: worst gap / bound {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", dc.FORM_NAMES)
def test_every_block_moves_the_identity(name):
    """A reference without any one block's contribution misses the identity by far."""
    c = jc.SHAPES[1]
    q, L, v, D = _case(name, c)
    w = dc.cotangents(L)[0]
    full = jc.jvp_reference(name, q, v, D, MU)
    for k in D:
        if k in dc.form_absent(name):
            continue
        without = jc.jvp_reference(name, q, v, {kk: a for kk, a in D.items() if kk != k}, MU)
        gap, _ = _gap(name, c, v, w, without, D)
        bound = _gap(name, c, v, w, full, D)[1]
        assert gap > 1e3 * bound, (name, k, gap, bound)


@pytest.mark.parametrize("name,c", CASES, ids=[f"{n}-{nc.case_id(c)}" for n, c in CASES])
def test_reference_feasibility(name, c):
    """Affine linearity: the reference is r(theta + D) - r(theta) at generated data to 8e-16 relative; duality: the
    identity's gap is at most 5e-7 of its bound."""
    q, L, v, D = _case(name, c, 1)
    ref = jc.jvp_reference(name, q, v, D, MU)
    theta = {k: q[dc.KEYS[k]] for k in dc.present(*c)}
    vl = dc.ld(v)
    r0 = dc.residuals_form(name, jc._data(c, theta), vl, np.longdouble(MU))
    r1 = dc.residuals_form(name, jc._data(c, {k: dc.ld(theta[k]) + dc.ld(D[k]) for k in theta}), vl, np.longdouble(MU))
    lin = dc.rel_err(np.asarray(r1 - r0, dtype=np.float64), ref)
    w = dc.cotangents(L)[0]
    gap, bound = _gap(name, c, v, w, ref, D)
    print(f"{name} {nc.case_id(c)}: linearity {lin:.2e} (8e-16), duality gap / bound {gap / bound:.2e} (5e-7)")
    assert lin <= 8e-16
    assert gap <= 5e-7 * bound


def test_loop_table_matches_the_sources():
    """The loop table's cases reach the loops they claim, by the kernels' own constants."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "ipm-zoo_amd", "csrc")
    hdr, src = open(os.path.join(csrc, "kernels.h")).read(), open(os.path.join(csrc, "jvp.hip")).read()
    assert int(re.search(r"#define IPMZ_JVP_ROWS_GY (\d+)", hdr).group(1)) == jc.ROWS_GY
    assert re.search(r"constexpr int CT = (\d+) \* NP;", src).group(1) == str(jc.PAIR_COLS)
    assert int(re.search(r"constexpr int NT = (\d+);", src).group(1)) // 64 == jc.WAVES
    assert re.search(r"return n <= 128 \? 1 : n <= 256 \? 2 : 4;", src)
    assert re.search(r"mt\.rch = 32;", src) and re.search(r"mt\.rch > 8 && .* < (\d+)\)", src).group(1) == str(jc.FILL)
    assert int(re.search(r"constexpr int KC = (\d+),", src).group(1)) == jc.KSTEP
    by = {c[0]: c for c in jc.LOOPS}
    n = by["pairs_nct"][1][0]
    assert jc.plan(n, n)[:2] == (3, 16) and jc.plan(n - 1, n - 1)[1] == 8      # the smallest n with 16 rows per chunk
    assert 16 // jc.WAVES > 2                                                   # ... a wave's second pair of rows
    n = by["rch32"][1][0]
    assert jc.plan(n, n)[:2] == (4, 32) and jc.plan(n - 1, n - 1)[1] == 16
    _, c, B, ntan, _ = by["rows_gy"]
    assert B * ntan > jc.ROWS_GY >= (B - 1) * ntan and ntan == max(jc.NTANS)
    assert [jc.pairs(by[k][1][0]) for k in ("np1_edge", "np2_edge", "np2_full", "np4_edge")] == [1, 2, 2, 4]
    assert all(jc.plan(by[k][1][0], by[k][1][1])[2] == 2 for k in ("np1_edge", "np4_edge"))   # two chunks of A
    assert all(c[0] > jc.KSTEP for c in jc.SHAPES[1:]) and jc.SHAPES[2][1] > jc.KSTEP   # k_jvp_shared's K loop, both products
    # every residue of the K tail (K = n, m or p; MFMA steps of 4) and partial tiles of QPs (16 per tile, 64 per wave)
    assert {k % 4 for c in jc.SHAPES for k in c} == {0, 1, 2, 3}
    assert all(b % 16 for b in jc.BATCHES) and max(jc.BATCHES) > 16


def test_entry_point_exists_and_refuses_a_null_solver():
    I = pytest.importorskip("ipmz_amd")
    tan = I._QPDeviceTangent()
    assert I.lib.ipmz_batch_data_jvp(None, 1, ctypes.byref(tan), ctypes.c_void_p(16), 2, 2) == -1
    assert b"null" in I.lib.ipmz_last_error()
    assert ctypes.sizeof(tan) == 21 * 8 + 9 * 8
