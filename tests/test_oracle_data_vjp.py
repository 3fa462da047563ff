"""What the device tests of ipmz_batch_data_vjp rely on, checked without a GPU: the numpy reference of
tests/data_vjp_cases.py satisfies the bilinear identity against nc.residuals_numpy (so it is the transpose of the
residuals' dependence on the data, all nine blocks at once); reference_form satisfies it for every served formulation
against residuals_form, the numpy restatement of the formulation's shorthand definitions with mu a parameter, and is
dc.reference bitwise on the default form; and the entry point exists and refuses a null solver before it looks for a
device."""
import ctypes

import numpy as np
import pytest

import batch_form_cases as fc
import data_vjp_cases as dc
import newton_multi_cases as nc


@pytest.mark.parametrize("eq_none", (False, True), ids=("reg", "none"))
@pytest.mark.parametrize("c", nc.SHAPES, ids=nc.case_id)
def test_reference_satisfies_the_bilinear_identity(c, eq_none):
    q = nc.qp(*c)
    L = nc.offsets(q, eq_none)[3]
    rng = np.random.default_rng(31)
    v = rng.uniform(0.5, 2.0, L)  # any iterate: the identity does not need a feasible one
    r0 = nc.residuals_numpy(q, v, eq_none)
    worst = 0.0
    for k in range(3):
        w = dc.cotangents(L, 3)[k]
        deltas = dc.random_deltas(q, 100 + k)
        assert set(deltas) == set(dc.present(*c))
        r1 = nc.residuals_numpy(dc.perturbed(q, deltas), v, eq_none)
        grads = dc.reference(q, v, w, eq_none)
        assert set(grads) == set(deltas)
        gap, bound = dc.bilinear_gap(w, r0, r1, grads, deltas), dc.bilinear_bound(w, r0, r1)
        worst = max(worst, gap / bound)
        assert bound > 0 and gap <= bound, (k, gap, bound)
    print(f"{nc.case_id(c)} eq_none={eq_none}: worst gap / bound {worst:.3e}")


def test_every_block_moves_the_identity():
    """The identity is not satisfied by accident: a reference with any one block zeroed misses it by far."""
    c, eq_none = nc.SHAPES[1], False
    q = nc.qp(*c)
    L = nc.offsets(q, eq_none)[3]
    v = np.random.default_rng(32).uniform(0.5, 2.0, L)
    w = dc.cotangents(L)[0]
    deltas = dc.random_deltas(q, 7)
    r0, r1 = nc.residuals_numpy(q, v, eq_none), nc.residuals_numpy(dc.perturbed(q, deltas), v, eq_none)
    grads = dc.reference(q, v, w, eq_none)
    for k in grads:
        broken = dict(grads)
        broken[k] = np.zeros_like(grads[k])
        assert dc.bilinear_gap(w, r0, r1, broken, deltas) > 1e3 * dc.bilinear_bound(w, r0, r1), k


FORM_SHAPES = [(name, c) for name in dc.FORM_NAMES for c in (fc.S1, (40, 0, 0)) if c[1] or name in dc.M0_FORMS]
MU = 0.3  # the identity holds at any fixed mu; 0 would hide PenaltyFunction's and Slacks' mu terms


def _form_case(name, c, seed):
    q = nc.qp(*c)
    L = dc.form_offsets(name, *c)[3]
    v = np.random.default_rng(seed).uniform(0.5, 2.0, L)  # a random positive iterate
    return q, L, v


def test_form_table_is_every_served_formulation():
    assert set(dc.FORM_NAMES) == (set(fc.FORMS) - {"eqss", "naiveeq"}) | {"pen_sl"}
    assert set(dc.M0_FORMS) == (set(fc.S0_FORMS) - {"eqss"}) | {"pen_sl"}
    assert dc.form_absent("vnone") == ("l_x", "u_x") and dc.form_absent("alo") == ("u_A_ineq",)
    assert dc.form_absent("box") == dc.form_absent("pen_sl") == ()


@pytest.mark.parametrize("name,c", FORM_SHAPES, ids=[f"{n}-{nc.case_id(c)}" for n, c in FORM_SHAPES])
def test_reference_form_satisfies_the_bilinear_identity(name, c):
    """reference_form is the transpose of residuals_form's dependence on the data, all blocks at once."""
    q, L, v = _form_case(name, c, 33)
    r0 = dc.residuals_form(name, q, v, MU)
    assert r0.shape == (L,)
    worst = 0.0
    for k in range(3):
        w = dc.cotangents(L, 3)[k]
        deltas = dc.random_deltas(q, 300 + k)
        r1 = dc.residuals_form(name, dc.perturbed(q, deltas), v, MU)
        grads = dc.reference_form(name, *c, v, w)
        assert set(grads) == set(deltas) == set(dc.present(*c))
        for kk in dc.form_absent(name):
            assert kk not in grads or not grads[kk].any(), kk
        gap, bound = dc.bilinear_gap(w, r0, r1, grads, deltas), dc.bilinear_bound(w, r0, r1)
        worst = max(worst, gap / bound)
        assert bound > 0 and gap <= bound, (k, gap, bound)
    print(f"{name} {nc.case_id(c)}: worst gap / bound {worst:.3e}")


@pytest.mark.parametrize("name", dc.FORM_NAMES)
def test_every_block_of_every_form_moves_the_identity(name):
    """A reference_form with any one block zeroed (of those the formulation has) misses the identity by far."""
    c = fc.S1
    q, L, v = _form_case(name, c, 34)
    w = dc.cotangents(L)[0]
    deltas = dc.random_deltas(q, 8)
    r0, r1 = dc.residuals_form(name, q, v, MU), dc.residuals_form(name, dc.perturbed(q, deltas), v, MU)
    grads = dc.reference_form(name, *c, v, w)
    bound = dc.bilinear_bound(w, r0, r1)
    assert dc.bilinear_gap(w, r0, r1, grads, deltas) <= bound
    for k in grads:
        if k in dc.form_absent(name):
            continue
        broken = dict(grads)
        broken[k] = np.zeros_like(grads[k])
        assert dc.bilinear_gap(w, r0, r1, broken, deltas) > 1e3 * bound, k


@pytest.mark.parametrize("name,eq_none", (("box", False), ("none", True)))
@pytest.mark.parametrize("c", nc.SHAPES, ids=nc.case_id)
def test_reference_form_is_the_default_reference_bitwise(c, name, eq_none):
    q, L, v = _form_case(name, c, 35)
    assert L == nc.offsets(q, eq_none)[3]
    w = dc.cotangents(L)[0]
    a, b = dc.reference_form(name, *c, v, w), dc.reference(q, v, w, eq_none)
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k
    # ... and residuals_form restates nc.residuals_numpy at mu = 0
    assert np.array_equal(dc.residuals_form(name, q, v, 0.0), nc.residuals_numpy(q, v, eq_none))


def test_loop_cases_reach_the_loops():
    """The batches of dc.LOOP_BATCHES against the limits of grad.hip's grids (block_grid, data_terms.h) as the
    sources state them."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ipm-zoo_amd", "csrc")
    txt, grid = open(os.path.join(csrc, "grad.hip")).read(), open(os.path.join(csrc, "data_terms.h")).read()
    gx, gy = re.search(r"gx > (\d+) \? \1 : gx;\s*int64_t gy = (\d+) / gx;", grid).groups()
    assert (int(gx), int(gy)) == (dc.SUM_GX, dc.GRID_Y)
    assert "block_grid(" in txt and re.search(r"constexpr int GRID_NT = 256;", grid) and "NT == GRID_NT" in txt
    assert re.search(r"constexpr int NT = 256;", txt) and re.search(r"constexpr int VS = 64,", txt)
    n = dc.LOOP_SHAPE[0]
    assert max(dc.LOOP_BATCHES) > dc.GRID_Y // -(-n // 4) and max(dc.LOOP_BATCHES) > dc.GRID_Y
    assert -(-257 // 64) == 5 and 257 in dc.LOOP_BATCHES          # a full group of four plus a tail
    assert dc.BIG_N ** 2 > dc.SUM_GX * 256 >= 724 ** 2


def test_null_solver_is_invalid_without_a_device():
    import ipmz_amd as I
    grad = I._QPDeviceGrad()
    w = (ctypes.c_double * 4)()
    rc = I.lib.ipmz_batch_data_vjp(None, ctypes.cast(w, ctypes.c_void_p), 4, ctypes.byref(grad))
    assert rc == -1, rc  # IPMZ_ERR_INVALID
    assert b"null" in I.lib.ipmz_last_error()
    assert "ipmz_batch_data_vjp" in I.EXPORTS


def test_chunk_size_matches_the_sources():
    """The batches that straddle the K chunk of the shared matrix blocks use the kernels' own chunk size."""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(here, "..", "ipm-zoo_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"#define IPMZ_VJP_KCHUNK (\d+)", txt).group(1)) == dc.KCHUNK
    assert {dc.KCHUNK - 1, dc.KCHUNK, dc.KCHUNK + 1} <= {c[3] for c in dc.BATCH_CASES}


def test_the_data_blocks_are_described_once():
    """The nine blocks, the dual A^T multiplies and the grid of the data calls each have one statement: the spellings
    of the copies that csrc/kernels.h DATA_BLOCKS and csrc/data_terms.h replaced occur nowhere."""
    import glob
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ipm-zoo_amd")
    src = {os.path.basename(f): open(f).read() for f in glob.glob(os.path.join(root, "csrc", "*"))}
    everything = "\n".join(src.values())
    for old in ("QpIoData", "QpGradOut", "QpTanIn", "grad_grid", "io_grid", "jvp_dual", "grad_vec_ok", "IPMZ_GRAD_",
                "IPMZ_JVP_MATRIX", "IPMZ_JVP_SHARED"):
        assert old not in everything, old
    table = re.findall(r"DATA_BLOCKS\[DB_COUNT\] = \{(.*?)\};", src["kernels.h"], re.S)
    assert len(table) == 1 and everything.count("DATA_BLOCKS[DB_COUNT] = {") == 1
    rows = re.findall(r'\{"(\w+)", (true|false), ([012]), HELD_\w+\}', table[0])
    assert [r[0] for r in rows] == ["Q", "A", "C", "c", "l_x", "u_x", "l_A", "u_A", "d"]
    assert [r[1:] for r in rows] == [("true", "0"), ("true", "1"), ("true", "2"), ("false", "0"), ("false", "0"),
                                     ("false", "0"), ("false", "1"), ("false", "1"), ("false", "2")]
    assert "blocks[9]" not in src["qp.cpp"]
    assert len(re.findall(r"double a_dual\(", everything)) == 1
    assert everything.count("q.v[LH][i] + (-q.v[LG][i])") == 1
    assert "_tangent_block" not in open(os.path.join(root, "ipmz_amd", "__init__.py")).read()
