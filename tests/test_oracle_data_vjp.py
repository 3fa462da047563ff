"""What the device tests of ipmz_batch_data_vjp rely on, checked without a GPU: the numpy reference of
tests/data_vjp_cases.py satisfies the bilinear identity against nc.residuals_numpy (so it is the transpose of the
residuals' dependence on the data, all nine blocks at once), and the entry point exists and refuses a null solver
before it looks for a device."""
import ctypes

import numpy as np
import pytest

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
