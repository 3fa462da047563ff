"""What tests/test_gpu_batch_kkt_multi.py relies on, checked without a GPU:

  * the reference is good to far less than the device bound: for every QP of
    every shape, at the initial iterate and after two oracle iterations, the
    oracle's LDL^T solve and numpy.linalg.solve of the oracle's KKT matrix agree
    to < 1e-13 in the tests' measure (the device bound is 1e-12);
  * the raggedness each shape is there for: blocks, sub-blocks, panels, the
    even row stride;
  * which shapes the one-launch (fused) solve serves: the limits 832 (nbi 64)
    and 768 (nbi 128) against 160 KiB, from the tile constants read out of
    csrc/trsm.hip, and the crossover the looped right-hand-side counts assume.
"""
import os
import re

import numpy as np
import pytest

import batch_kkt_cases as kc
import oracle

REF_TOL = 1e-13


@pytest.mark.parametrize("c", kc.SHAPES, ids=kc.case_id)
def test_two_cpu_solves_agree(c):
    N, B = kc.order(c), c[3]
    rows = kc.rhs(N, B)[:, :3]
    worst = 0.0
    for q, o in enumerate(kc.oracles(c)):
        for it in range(2):
            K = np.array(o.kkt())
            assert K.shape == (N, N) and np.array_equal(K, K.T)
            X = kc.reference(np.tril(K), rows[q])
            worst = max(worst, kc.row_err(X, np.linalg.solve(K, rows[q].T).T))
            if it == 0:
                assert o.iterate()[0] == 0 and o.iterate()[0] == 0  # no QP converges before the second comparison
    print(f"N{N}: oracle LDL^T solve vs numpy.linalg.solve {worst:.3e} (bound {REF_TOL:.1e})", flush=True)
    assert worst < REF_TOL


def test_shapes_reach_what_they_name():
    N = [kc.order(c) for c in kc.SHAPES]
    assert N == [72, 192, 321, 832, 834, 1040]
    assert all(c[3] >= 2 for c in kc.SHAPES)

    def blocks(n, nb):
        return [min(nb, n - j) for j in range(0, n, nb)]

    assert blocks(72, 64) == [64, 8] and blocks(72, 128) == [72]
    assert blocks(192, 64) == [64, 64, 64]
    assert blocks(321, 64) == [64] * 5 + [1] and 321 % 2 == 1 and kc.ldb_of(321) == 322
    assert blocks(321, 128) == [128, 128, 65] and blocks(65, 64) == [64, 1]  # nbi 128: a one-column second sub-block
    assert blocks(832, 64) == [64] * 13
    assert blocks(834, kc.PANEL) == [256, 256, 256, 66]   # 4 panels
    assert blocks(1040, kc.PANEL) == [256, 256, 256, 256, 16]  # 4 panels + 16 columns
    assert set(kc.NBI128_ORDERS) <= set(N)
    # right-hand-side groups of 16: one full, a one-row second, two + one row
    c = kc.trsm_constants()
    assert c["TM_G"] == 16 and [-(-r // 16) for r in kc.RHS_COUNTS] == [1, 1, 1, 2, 3] and 17 % 16 == 1


def test_fused_limits_follow_from_the_kernel_constants():
    c = kc.trsm_constants()
    assert kc.fused_limit(64, c) == 832 and kc.fused_limit(128, c) == 768
    assert kc.panel_lds_bytes(832, 64, c) == 156160 <= kc.LDS_BYTES < kc.panel_lds_bytes(896, 64, c)
    assert kc.panel_lds_bytes(768, 128, c) == 156160 <= kc.LDS_BYTES < kc.panel_lds_bytes(896, 128, c)
    fused = [kc.order(s) for s in kc.SHAPES if kc.fused_eligible(kc.order(s), 64, c)]
    assert fused == [72, 192, 321, 832]  # 834 rounds up to 896 columns: the first that does not fit
    assert all(kc.fused_eligible(N, 128, c) for N in kc.NBI128_ORDERS)
    # the limit is computed from the device's LDS, never a literal order
    with open(os.path.join(kc.CSRC, "trsm.hip")) as f:
        src = f.read()
    assert "hipDeviceAttributeMaxSharedMemoryPerBlock" in src
    body = src[src.index("bool ldlt_solve_fused_eligible"):]
    assert "832" not in body and "768" not in body


def test_looped_counts_are_below_the_crossover():
    with open(os.path.join(kc.CSRC, "qp.cpp")) as f:
        cross = int(re.search(r"static constexpr int BATCH_MULTI_CROSSOVER = (\d+);", f.read()).group(1))
    looped = [r for r in kc.RHS_COUNTS if r < cross]
    assert 1 in looped and 3 in looped and all(r >= cross for r in kc.RHS_COUNTS if r >= 16)
