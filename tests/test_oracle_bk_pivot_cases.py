"""What tests/test_gpu_bk_pivot_edges.py relies on, without a GPU: the
recording restatement of tests/bk_pivot_cases.py equals the oracle's
Bunch-Kaufman factor on every case, and every case hits what it claims (read
from the restatement's decision trace: conditions on the inputs, not
measurements).  The oracle itself is pinned to the reference on tied data by
the bkp_* fixtures (tests/test_oracle_golden.py)."""
import numpy as np
import pytest

import bk_pivot_cases as C
import oracle


def _same_factor(K, nonfinite):
    F, piv, info, trace = C.factor_trace(K)
    Fo, po, io = oracle.bk_factor(K)
    assert not any(r["past_end"] for r in trace)  # (the reference would index past the matrix)
    if not nonfinite:
        assert np.isfinite(Fo).all()
    assert np.array_equal(np.isnan(np.tril(F)), np.isnan(np.tril(Fo)))
    assert np.array_equal(np.tril(F), np.tril(Fo), equal_nan=nonfinite)
    assert np.array_equal(np.triu(F, 1), np.triu(Fo, 1), equal_nan=nonfinite)
    assert np.array_equal(piv, po) and info == io
    return trace


@pytest.mark.parametrize("name", C.names())
def test_restatement_equals_oracle(name):
    family, K, nonfinite = C.cases()[name]
    F, piv, info, trace = C.traced(name)
    Fo, po, io = C.oracle_factor(name)
    assert not any(r["past_end"] for r in trace), name
    if not nonfinite:
        assert np.isfinite(Fo).all()
    assert np.array_equal(np.isnan(F), np.isnan(Fo))
    assert np.array_equal(F, Fo, equal_nan=nonfinite)
    assert np.array_equal(piv, po) and info == io
    steps = sum(2 if r["branch"] == "2x2" else 1 for r in trace)
    assert steps == K.shape[0]


def test_small_int_hits_every_branch():
    seen, infos, ties = set(), [], 0
    for name in C.names("small_int"):
        trace = C.traced(name)[3]
        seen |= {r["branch"] for r in trace}
        infos.append(C.traced(name)[2])
        ties += C.tied_row_searches(trace)
    assert seen == set(C.BRANCHES)
    assert any(infos)  # a zero column past column 0, by exact cancellation
    assert C.traced("small_int3_s3")[2] == 2
    assert ties >= 10
    assert sorted({C.cases()[n][1].shape[0] for n in C.names("small_int")}) == [1, 2, 3, 17, 64, 65, 130, 300]


def test_alpha_is_the_oracles():
    assert C.ALPHA == (1.0 + np.sqrt(17.0)) / 8.0


@pytest.mark.parametrize("name,bases", [("threshold21", (0,)), (f"threshold{C.THRESHOLD_N}", C.THRESHOLD_BASES)])
def test_threshold_gadgets(name, bases):
    K = C.cases()[name][1]
    trace = {r["k"]: r for r in C.traced(name)[3]}
    for base in bases:
        for o, (gname, akk, d, three, branch, which, equal) in zip(C.gadget_offsets(base), C.GADGETS):
            r = trace[o]  # the gadget's first step meets its original values
            assert K[o, o] == akk and K[o + 1, o + 1] == d
            assert r["branch"] == branch, (base, gname, r)
            assert r[which] is equal, (base, gname, r)  # evaluated, and with / without equality
            assert r["imax"] == o + 1 and r["ties"] == 1 and r["row_search"] == (branch != "keep1")
    assert sum(bool(r[e]) for r in trace.values() for e in ("eq1", "eq2", "eq3")) == 5 * len(bases)
    assert C.traced(name)[2] == 0 and not any(r["branch"] == "zero" for r in trace.values())
    # the one-ulp misses are one ulp away
    assert np.nextafter(C.GADGETS[1][1], 1.0) == C.ALPHA and np.nextafter(C.GADGETS[4][1], 1.0) == C.ALPHA / 2
    assert np.nextafter(C.GADGETS[6][2], 4.0) == 2 * C.ALPHA


def test_threshold_gadgets_straddle_the_edges():
    N = C.THRESHOLD_N
    assert N > 512  # IPMZ_BK_GRID_MIN
    spans = [(o, o + (3 if g[3] else 2) - 1) for base in C.THRESHOLD_BASES
             for o, g in zip(C.gadget_offsets(base), C.GADGETS)]
    assert all(a0 > b1 for (a0, _), (_, b1) in zip(spans[1:], spans[:-1]))  # no overlap
    for edge in (64, 1024):
        assert any(lo < edge <= hi for lo, hi in spans), edge
    assert spans[-1][1] == N - 1


@pytest.mark.parametrize("k", sorted(C.SPREAD_COLUMNS))
def test_spread_tie_columns(k):
    rows = C.SPREAD_COLUMNS[k]
    K = C.cases()["spread_tie"][1]
    assert C.SPREAD_N >= 1200 and len(rows) >= 8 and list(rows) == sorted(rows)
    assert (np.abs(K[list(rows), k]) == 1.0).all() and {-1.0, 1.0} == set(K[list(rows), k])
    assert np.count_nonzero(K[:, k]) == len(rows) + 1
    r = next(r for r in C.traced("spread_tie")[3] if r["k"] == k)
    assert r["ties"] == len(rows) and r["row_search"] and r["imax"] == rows[0] and r["branch"] == "2x2"
    piv = C.traced("spread_tie")[1]
    assert piv[k] == piv[k + 1] == -rows[0]
    # the first tied row wins under no other ordering than the smallest row index
    wrong = C.wrong_order_winners(k, rows)
    assert len(wrong) == 4 + 257
    assert all(w != rows[0] for w in wrong.values()), [n for n, w in wrong.items() if w == rows[0]]
    # and any other winner changes ipiv: the first entry one ulp lower hands the tie to the second row
    Kp = C.spread_tie(ulp_column=k)
    assert np.count_nonzero(Kp != K) == 2
    tp = _same_factor(Kp, False)
    rp = next(r for r in tp if r["k"] == k)
    assert rp["imax"] == rows[1] and rp["branch"] == "swap1" and rp["ties"] == len(rows) - 1
    pivp = oracle.bk_factor(Kp)[1]
    assert pivp[k] == rows[1] and pivp[k + 1] == k + 1


ALL_QPS = list(C.STRUCTURED) + [(n, m, p, s) for n, m, p, ss in C.STRUCTURED_BATCH.values() for s in ss]


@pytest.mark.parametrize("n,m,p,seed", ALL_QPS, ids=[f"n{c[0]}m{c[1]}s{c[3]}" for c in ALL_QPS])
def test_structured_qp_ties(n, m, p, seed):
    qp = C.structured_qp(n, m, p, seed)
    assert np.array_equal(qp["Q"], np.eye(n)) and set(np.unique(qp["C"])) == {-8.0, 0.0, 8.0}
    assert (np.abs(qp["C"]).sum(axis=1) == 16.0).all() and (qp["A"].sum(axis=1) == 3.0).all()
    o = oracle.OracleQP(qp, eq_none=True)
    for it in range(4):
        trace = _same_factor(o.kkt(), False)
        assert C.tied_row_searches(trace) >= C.STRUCTURED_MIN_TIES[n], (it, C.tied_row_searches(trace))
        done, _ = o.iterate()
        assert not done
    for it in range(4, 13):
        done, _ = o.iterate()
        if done:
            break
    assert done == 1


def test_single_structured_qp_reaches_the_grid_factor():
    n, m, p, _ = C.STRUCTURED[-1]
    assert n + m + p == 960 > 512  # IPMZ_BK_GRID_MIN


@pytest.mark.parametrize("name", C.names("nonfinite"))
def test_nonfinite_cases(name):
    K = C.cases()[name][1]
    F, piv, info, trace = C.traced(name)
    assert not np.isfinite(K).all() and not np.isfinite(F).all()
    if name.startswith("nan_pair") or name.startswith("inf_pair"):
        N = K.shape[0]
        i, j = N // 3, N // 2
        assert not np.isfinite(K[j, i]) and not np.isfinite(K[i, j]) and (~np.isfinite(K)).sum() == 2
        assert np.isnan(K[j, i]) == name.startswith("nan_pair")
    if name.startswith("nan_diag"):
        j = int(np.flatnonzero(np.isnan(np.diag(K)))[0])
        assert (~np.isfinite(K)).sum() == 1 and np.count_nonzero(K[j + 1:, j]) > 0
    if name.startswith("kp_lt_k"):
        N, arrow, at = C.KP_LT_K[name]
        r = next(r for r in trace if r["k"] == at)
        assert r["kp_lt_k"] and r["kp"] == 0 and r["imax"] == 0 and r["ties"] == 0 and r["branch"] == "swap1"
        assert piv[at] == 0 and np.isnan(F[at, 0])
        if arrow:  # a finished, nonzero column of L moves into the pivot column
            assert np.count_nonzero(F[at + 1:, at]) == N - at - 1
    # NaN never wins a search: every row searched holds a finite, positive column maximum
    for r in trace:
        assert r["imax"] == 0 or r["ties"] >= 1


def test_kp_lt_k_small_is_the_issue_case():
    F, piv, info = C.oracle_factor("kp_lt_k8")
    assert list(piv) == [0, 1, 2, 3, 4, 0, 6, 7] and info == 0
    assert {at for _, _, at in C.KP_LT_K.values()} == {5, 300}  # the first wave of k_bk_factor, and past it
    assert any(r["kp_lt_k"] for n in ("nan_pair33", "nan_diag65", "scaled65_2e-1040") for r in C.traced(n)[3])


def test_scaled_cases():
    base = C.oracle_factor("small_int65_s66")[1]
    for e in C.SCALES:
        F, piv, info = C.oracle_factor(f"scaled65_2e{e}")
        assert not np.array_equal(piv, base), e  # alpha colmax^2 overflows / underflows: other pivots
    assert not np.isfinite(C.oracle_factor("scaled65_2e-1040")[0]).all()
    K = C.cases()["scaled65_2e-1040"][1]
    assert 0 < np.abs(K[K != 0]).max() < np.finfo(np.float64).tiny  # subnormal
