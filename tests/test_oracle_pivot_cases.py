"""The generators of pivot_cases.py against the CPU oracle (no GPU): the
conditions test_gpu_pivot_edges.py relies on hold for the inputs themselves,
so a GPU failure there is the kernels', not the inputs'."""
import numpy as np
import pytest

import oracle
import pivot_cases as pc

ALL_CONFIGS = pc.ORACLE_CONFIGS + pc.EXACT_ONLY_CONFIGS
_ids = lambda c: f"N{c[0]}-nbo{c[1][0]}-nbi{c[1][1]}"  # noqa: E731


@pytest.mark.parametrize("cfg", ALL_CONFIGS, ids=_ids)
def test_positions_cover_every_edge(cfg):
    N, blocking = cfg
    nbo, nbi = pc.resolve_blocking(N, blocking)
    pos = pc.positions(N, nbo, nbi)
    want = [p for p in (0, 15, 16, 63, 64, 127, 128, nbo - 1, nbo, N - 1) if p < N]
    assert set(want) <= set(pos) and all(0 <= p < N for p in pos)
    last0 = (N - 1) // nbi * nbi
    assert any(last0 < p < N - 1 for p in pos)  # one index inside the last ragged inner block
    pairs = pc.pair_positions(N, nbo)
    assert {15, 63, 127, N - 2} <= set(pairs) and (nbo - 1 in pairs or nbo >= N)


@pytest.mark.parametrize("cfg", ALL_CONFIGS, ids=_ids)
def test_int_factor_exactness_condition(cfg):
    """A B 128 < 2^53 (pivot_cases.exactness_product), K is the integer matrix
    (L0 D0) L0^T exactly, and rows have at most 4 entries of +-1."""
    N, blocking = cfg
    pos = pc.positions(N, *pc.resolve_blocking(N, blocking))
    K, L0, D0, L_exp, D_exp = pc.int_factor(N, 11 * N, pos)
    A, B, prod = pc.exactness_product(L0, D0)
    assert prod < 2.0 ** 53, (A, B, prod)
    assert np.array_equal(K, K.T) and np.array_equal(K, np.rint(K))
    if N <= 2560:
        assert np.array_equal(K, (L0 * D0) @ L0.T)
    off = np.tril(L0, -1)
    assert np.array_equal(np.triu(L0), np.eye(N)) and set(np.unique(off)) <= {-1.0, 0.0, 1.0}
    assert (np.abs(off).sum(axis=1) <= 4).all()
    assert set(np.unique(D0)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and np.array_equal(np.flatnonzero(D0 == 0), pos)
    assert np.array_equal(np.diag(K)[[0]], D0[[0]])
    assert np.count_nonzero(np.diag(K)[pos[1:]]) > 0  # zero pivots that appear only after the updates


@pytest.mark.parametrize("N", [200, 300, 700, 1000, 1408])
def test_oracle_reproduces_int_factor(N):
    pos = pc.positions(N, 256, 64)
    K, L0, D0, L_exp, D_exp = pc.int_factor(N, 11 * N, pos)
    L, D = oracle.ldlt(K)
    assert np.array_equal(D, D_exp) and np.array_equal(np.tril(L, -1), L_exp)
    Lb, Db = oracle.ldlt_blocked(K)
    assert np.array_equal(Db, D_exp) and np.array_equal(np.tril(Lb, -1), L_exp)


def _right_looking(K, rule):
    """A right-looking LDL^T in numpy (another elimination order than the
    oracle's).  rule "updated": the reference's zero test, on the updated
    pivot; "input": the zero test misapplied to the input diagonal entry."""
    A = np.array(K, dtype=np.float64)
    N = A.shape[0]
    L, D = np.eye(N), np.zeros(N)
    with np.errstate(all="ignore"):
        for i in range(N):
            d = A[i, i]
            if (d if rule == "updated" else K[i, i]) == 0.0:
                d = 1e-8
            D[i] = d
            w = A[i + 1:, i].copy()
            L[i + 1:, i] = w / d
            A[i + 1:, i + 1:] -= np.outer(L[i + 1:, i], w)
    return L, D


def test_cases_tell_a_misplaced_zero_test():
    """The integer factor is exact in a second elimination order, and both it
    and the saddle matrix fail their GPU assertions for a factor that tests the
    input diagonal entry in place of the updated pivot."""
    N = 200
    pos = pc.positions(N, 256, 64)
    K, L0, D0, L_exp, D_exp = pc.int_factor(N, 11 * N, pos)
    L, D = _right_looking(K, "updated")
    assert np.array_equal(D, D_exp) and np.array_equal(np.tril(L, -1), L_exp)
    L, D = _right_looking(K, "input")
    assert not np.array_equal(D, D_exp)
    n, mp = 150, 50
    Ks = pc.saddle(n, mp, n + mp)
    L, D = _right_looking(Ks, "updated")
    assert (D[n:] < 0).all() and not (D == 1e-8).any()
    L, D = _right_looking(Ks, "input")
    assert (D == 1e-8).any()


def _deleted_factor(K, gone):
    keep = np.setdiff1d(np.arange(K.shape[0]), gone)
    L, D = oracle.ldlt(K[np.ix_(keep, keep)])
    return keep, L, D


@pytest.mark.parametrize("cfg", pc.ORACLE_CONFIGS, ids=_ids)
def test_zero_rows_decouple(cfg):
    """D[j] == 1e-8, L[j+1:, j] == 0, and every other entry is, bit for bit,
    the factor of the matrix with those rows and columns deleted."""
    N, blocking = cfg
    pos = pc.positions(N, *pc.resolve_blocking(N, blocking))
    K = pc.zero_rows(pc.qd(N, N), pos)
    assert np.count_nonzero(np.diag(pc.qd(N, N))) == N
    L, D = oracle.ldlt(K)
    assert np.array_equal(D[pos], np.full(len(pos), 1e-8))
    for j in pos:
        assert not L[j + 1:, j].any() and not L[j, :j].any()
    keep, Lk, Dk = _deleted_factor(K, pos)
    assert np.array_equal(D[keep], Dk) and np.array_equal(L[np.ix_(keep, keep)], Lk)
    b = np.random.default_rng(1).uniform(-1, 1, N)
    b[pos] = 1.0
    assert np.array_equal(oracle.solve_ldlt(L, D, b)[pos], np.full(len(pos), 1e8))


@pytest.mark.parametrize("cfg", pc.ORACLE_CONFIGS, ids=_ids)
def test_pairs_give_1e8_multiplier(cfg):
    N, blocking = cfg
    pairs = pc.pair_positions(N, pc.resolve_blocking(N, blocking)[0])
    js = np.array(pairs)
    K = pc.embed_pairs(pc.qd(N, N), pairs)
    L, D = oracle.ldlt(K)
    assert np.array_equal(D[js], np.full(len(js), 1e-8))
    assert np.array_equal(L[js + 1, js], np.full(len(js), 1e8))
    assert np.allclose(D[js + 1], 2 - 1e8, rtol=1e-15, atol=0)
    sp = np.concatenate([js, js + 1])
    keep, Lk, Dk = _deleted_factor(K, sp)
    assert np.array_equal(D[keep], Dk) and np.array_equal(L[np.ix_(keep, keep)], Lk)
    # the well-conditioned right-hand side: x[j+1] = 1 / (2 - 1e8), x[j] = -1e8 x[j+1]
    b = np.random.default_rng(2).uniform(-1, 1, N)
    b[js], b[js + 1] = 0.0, 1.0
    x = oracle.solve_ldlt(L, D, b)
    assert np.allclose(x[js + 1], 1 / (2 - 1e8), rtol=1e-14, atol=0)
    assert np.allclose(x[js], -1e8 / (2 - 1e8), rtol=1e-14, atol=0)


@pytest.mark.parametrize("n,mp", [(150, 50), (450, 250)])
def test_saddle_fills_in(n, mp):
    K = pc.saddle(n, mp, n + mp)
    assert not np.diag(K)[n:].any()
    L, D = oracle.ldlt(K)
    assert (D[:n] > 0).all() and (D[n:] < 0).all() and not (D == 1e-8).any()
    assert np.linalg.cond(K) < 1e3  # well conditioned: an fp32 factor refines it in a few corrections


@pytest.mark.parametrize("cfg", pc.ORACLE_CONFIGS, ids=_ids)
def test_rows_before_first_nonfinite_pivot_are_clean(cfg):
    N, blocking = cfg
    nbo, nbi = pc.resolve_blocking(N, blocking)
    K = pc.qd(N, N)
    L0, D0 = oracle.ldlt(K)
    cases = pc.contaminations(N, nbo)
    assert len(cases) >= 6
    for label, i, j, val in cases:
        with np.errstate(all="ignore"):
            L, D = oracle.ldlt(pc.contaminate(K, i, j, val))
        assert np.isfinite(D[:i]).all() and not np.isfinite(D[i]), label
        assert np.array_equal(D[:i], D0[:i]) and np.array_equal(L[:i], L0[:i]), label


def test_normal_sign_pattern():
    """Case 5's S test: with K[n+q, n+q] = +10 the pivots are > 0 on H, < 0 on
    [n, n+q) and > 0 at n + q; contaminations inside H stay inside H."""
    n, mp = 150, 50
    K = pc.aug(n, mp, n + mp)
    for q in (0, mp - 1):
        D = oracle.ldlt(pc.contaminate(K, n + q, n + q, 10.0))[1]
        assert (D[:n] > 0).all() and (D[n:n + q] < 0).all() and D[n + q] > 0
    D = oracle.ldlt(K)[1]
    assert (D[:n] > 0).all() and (D[n:] < 0).all()
    for label, i, j, val in pc.contaminations(n + mp, 256, limit=n):
        assert j <= i < n, label
