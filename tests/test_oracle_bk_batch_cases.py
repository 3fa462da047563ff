"""What tests/test_gpu_bk_batch_multi.py relies on, checked on the CPU oracle:
the pivot facts of every batch of tests/bk_batch_cases.py (so a later change
to a generator cannot hollow out the GPU tests), the margin of the reference
inside the tolerance, the source constants the routes follow from, and that
the generated EqualityHandling::None QPs exercise no pivoting at all.
"""
import numpy as np
import pytest

import bk_batch_cases as C
import oracle


def _facts(key):
    _, _, piv, info = C.system(key)
    return C.pair_starts(piv), C.interchanges(piv), info


def test_one_block_plus_eight_columns_with_a_pattern_per_system():
    facts = [_facts(k) for k in C.BATCHES["indef72"]]
    assert [len(f[0]) for f in facts] == [15, 24, 13]
    assert [f[1] for f in facts] == [36, 28, 24]
    assert all(f[2] == 0 for f in facts)


def test_a_pair_across_a_block_edge_in_some_systems_only():
    starts = [_facts(k)[0] for k in C.BATCHES["indef192"]]
    assert [63 in s for s in starts] == [True, False, True]
    assert not any(k % 64 == 63 for k in starts[1])


def test_odd_order_with_a_pair_ending_in_the_one_column_last_block():
    keys = C.BATCHES["indef321"]
    assert all(C.order(k) == 321 for k in keys) and C.ldb_of(321) == 322
    starts = _facts(keys[1])[0]
    assert 63 in starts and 319 in starts  # rows 319 | 320: the second one is the whole last block


def test_fused_limit_and_the_orders_around_it():
    assert C.fused_limit() == C.FUSED_LIMIT == 832
    assert [C.order(k) for k in C.BATCHES["kktz832"]] == [832, 832]   # the largest eligible order
    assert [C.order(k) for k in C.BATCHES["indef834"]] == [834, 834]  # the first even order past it
    s500, s502 = (_facts(k)[0] for k in C.BATCHES["kktz832"])
    assert 511 in s500 and 255 in s502  # a pair across a 256-column panel boundary
    s300, s302 = (_facts(k)[0] for k in C.BATCHES["indef834"])
    assert 255 in s302 and 767 in s302
    assert not any(k % 256 == 255 for k in s300)


def test_panel_batch_has_pairs_at_panel_edges():
    s301, s302 = (_facts(k)[0] for k in C.BATCHES["indef1040"])
    assert 255 in s301 and 511 in s302
    assert C.order(C.BATCHES["indef1040"][0]) == 4 * 256 + 16


def test_every_regular_matrix_pivots_and_factors():
    for keys in C.BATCHES.values():
        for k in keys:
            starts, inter, info = _facts(k)
            assert info == 0 and starts and inter, k


def test_singular_batch_info_words():
    assert [_facts(k)[2] for k in C.SINGULAR] == C.SINGULAR_INFO == [0, 161, 0]
    assert C.SINGULAR_DEVICE_INFO == [i + 1 if i else 0 for i in C.SINGULAR_INFO]
    piv = C.system(C.SINGULAR[1])[2]
    assert piv[159] == piv[160] == -274 and piv[161] == 161  # column 160 leaves before it is met; 161 is met
    # the singular system's reference has the same non-finite entries in every row
    X = C.reference(C.SINGULAR[1], 1, 3)
    assert not np.isfinite(X).all()
    assert (np.isfinite(X) == np.isfinite(X[0])).all()


def test_row_counts_and_crossover():
    x = C.crossover()
    assert 2 <= x <= 16  # 1 row is looped, 16 rows (one full group) are blocked
    assert C.RHS_COUNTS == (1, 3, 16, 17, 33)
    assert max(r for r in C.RHS_COUNTS if r < x) >= 1 and min(r for r in C.RHS_COUNTS if r >= x) == 16


def test_reference_sits_30x_inside_the_tolerance():
    """An LU solve (other pivoting, other summation order) against the oracle on every matrix named."""
    worst, at = 0.0, None
    named = [k for keys in C.BATCHES.values() for k in keys] + [C.SINGULAR[0], C.SINGULAR[2], C.LU_WORST]
    for key in dict.fromkeys(named):
        K = C.system(key)[0]
        B = C.rhs(C.order(key), 1)[0]
        X = C.reference(key, 0, 1)
        e = C.row_err(np.linalg.solve(K, B.T).T, X)
        if e > worst:
            worst, at = e, key
    print(f"LU vs oracle: {worst:.3e} at {at}")
    assert at == C.LU_WORST
    assert worst <= C.LU_MARGIN and C.LU_MARGIN * 30 <= C.TOL, (worst, at)


@pytest.mark.parametrize("n,m,p", [(48, 16, 8), (100, 20, 8), (130, 40, 22), (256, 48, 17), (640, 160, 32),
                                   (642, 160, 32), (800, 200, 40)])
def test_generated_eq_none_qps_take_no_pair_and_no_interchange(n, m, p):
    # The x block of a generated QP's KKT matrix dominates every column, so
    # Bunch-Kaufman accepts each diagonal entry as a 1x1 pivot in place:
    # ipiv[k] == k everywhere.  A test through QPs alone would run none of the
    # interchange folding, none of the 2x2 D solves and no fallback -- the
    # QP-level GPU tests are about plumbing (assembly, factor storage, strides,
    # states), the constructed matrices above about the arithmetic.
    o = oracle.OracleQP(oracle.gen_qp(n, m, p, 1000), eq_none=True)
    for it in range(2):
        _, piv, info = oracle.bk_factor(o.kkt())
        assert info == 0
        assert np.array_equal(piv, np.arange(n + m + p)), it
        if it == 0:
            o.iterate()
