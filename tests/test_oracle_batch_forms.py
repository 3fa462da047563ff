"""The conditions tests/test_gpu_batch_forms.py relies on, checked on the CPU:

  * no comparison is skipped: for every (path, formulation, QP, step) of
    tests/batch_form_cases.py the oracle's iterate() returns done == 0 (for
    k0-w8 over the first 257 seeds: 256 compute units + 1);
  * the freeze / restart seeds converge after the tabled oracle iterations,
    every triple holds two distinct counts (some QP freezes while another
    steps) and the largest count plus one is below the restart test's 12 steps;
  * every path row lands on the kernel set it names: fused_phases,
    fused_solves, uses_k0 and the K0 allocation rule of csrc/qp.cpp and the
    wave-count rule of qp_fused_solves restated in Python, the restated source
    lines asserted present verbatim, the KKT order of every (row, formulation)
    put through them;
  * ipmz_batch_create refuses none of the table's combinations (create_solver's
    rules restated);
  * the shapes with more equality rows than variables (the update's third
    loop bound) hold exactly the formulations whose KKT matrix stays well
    conditioned there.
"""
import functools
import os
import re

import pytest

import batch_form_cases as fc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipm-zoo_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---------------------------------------------------------------------------
# 1. the paths, against the sources
def test_constants_match_the_sources():
    kernels, newton = _src("kernels.h"), _src("newton.hip")
    assert int(re.search(r"#define IPMZ_FUSED_NMAX (\d+)", kernels).group(1)) == fc.FUSED_NMAX
    assert int(re.search(r"#define IPMZ_SMALL_NMAX (\d+)", kernels).group(1)) == fc.SMALL_NMAX
    assert int(re.search(r"IPMZ_DEBUG_NO_K0 = (\d+)", kernels).group(1)) == fc.DEBUG_NO_K0
    assert int(re.search(r"IPMZ_DEBUG_NO_FUSED_SOLVES = (\d+)", kernels).group(1)) == fc.DEBUG_NO_FUSED_SOLVES
    assert f"inline bool fused_solves_ok(int N, int64_t ld) {{ return N <= {fc.FUSED_SOLVES_NMAX} && !(ld & 1); }}" in kernels
    assert "enum { KMODE_K = 0, KMODE_K0_DIAG = 1, KMODE_K0_OFFDIAG = 2 };" in kernels
    assert f"constexpr int FT = {fc.FT};  // 8 waves" in newton
    # k_fused_pre's copy units and the per-formulation bounds the fused bodies restate by hand
    assert f"const int nch = (N + {fc.PRE_UNIT - 1}) / {fc.PRE_UNIT}, units = kmode == KMODE_K0_DIAG ? 0 : N * nch;" in newton
    assert "const int N = q.N, n = q.n, m = q.m, nm = q.n + q.mk;" in newton
    assert "const int N = q.N, nm = q.n + q.m;" in newton
    assert "const int rows = nm + (q.eqpen ? q.p : 0);" in newton
    assert "const int mx = max(n, max(m, p));" in newton
    assert "for (int64_t t = tid; t < q.state_len; t += FT) restart_elem(q, t);" in newton
    assert "for (int t = tid; t < nr; t += FT) residual_elem<true>(q, t, 0.0, res2, comp, fa, fb);" in newton


def test_restated_dispatch_lines_are_the_sources():
    qp, newton, ldlt = _src("qp.cpp"), _src("newton.hip"), _src("ldlt.hip")
    for line in (
        "bool fused_phases(const ipmz_qp* s) { return s->B > 1 && s->N <= IPMZ_FUSED_NMAX; }",
        "  return fused_phases(s) && path_of(s) == Path::LdltBatch && s->ctx->nbi == 64 && fused_solves_ok(s->N, s->ldk) &&\n"
        "         !(debug_inject_mask() & IPMZ_DEBUG_NO_FUSED_SOLVES);",
        "  return s->K0 && s->ctx->nbi == 64 && s->N <= IPMZ_SMALL_NMAX && !(debug_inject_mask() & IPMZ_DEBUG_NO_K0);",
        "  if (B > 1 && N <= IPMZ_FUSED_NMAX && !s->eqnone) {\n    int64_t sK0 = 0;\n    s->K0 = dev_array(",
        "  if (s->eqnone) return s->B > 1 ? Path::BkBatch :",
        "  return s->B == 1 ? Path::Ldlt : Path::LdltBatch;",
        "  s->ldk = round_up(s->N, 64);",
        "  const bool fused = fused_phases(s);",
        "    HIP_OK(qp_fused_pre(qb, restart ? 1 : 0, s->eqnone ? nullptr : s->binfo, st, uses_k0(s) ? KMODE_K0_DIAG : KMODE_K));",
        "  if (s->K0) HIP_OK(qp_fused_pre(s->qb, 0, nullptr, st, KMODE_K0_OFFDIAG));",
        "    if (fused_solves(s)) {",
        "      HIP_OK(qp_fused_mid(qb, st));",
        "      HIP_OK(qp_fused_post(qb, freeze, st));",
    ):
        assert line in qp, line
    assert "  if (qb.B <= device_cus())\n    hipLaunchKernelGGL(k_fused_solves<16>," in newton
    assert "  else\n    hipLaunchKernelGGL(k_fused_solves<8>," in newton
    assert "  if (nbi == 64 && N <= IPMZ_SMALL_NMAX) return ldlt_factor_small_batched(" in ldlt


def dispatch(N, B, nbi, mask, eqnone, cus=fc.CUS):
    """qp.cpp's run_step / initialize decisions for a batch (mixed precision
    and the normal equations are single-QP settings)."""
    fused_phases = B > 1 and N <= fc.FUSED_NMAX
    k0_alloc = B > 1 and N <= fc.FUSED_NMAX and not eqnone
    ldlt_batch = not eqnone and B > 1  # path_of
    ldk = -(-N // 64) * 64
    fused_solves = (fused_phases and ldlt_batch and nbi == 64 and N <= fc.FUSED_SOLVES_NMAX and not ldk & 1
                    and not mask & fc.DEBUG_NO_FUSED_SOLVES)
    uses_k0 = k0_alloc and nbi == 64 and N <= fc.SMALL_NMAX and not mask & fc.DEBUG_NO_K0
    return dict(
        phases="fused" if fused_phases else "nonfused",
        initialize="KMODE_K0_OFFDIAG" if k0_alloc else None,
        pre=("KMODE_K0_DIAG" if uses_k0 else "KMODE_K") if fused_phases else None,
        factor="bk" if eqnone else "small" if nbi == 64 and N <= fc.SMALL_NMAX else "chain",
        factor_reads_k0=bool(fused_phases and uses_k0 and not eqnone),
        solves=(("k_fused_solves<16>" if B <= cus else "k_fused_solves<8>") if fused_solves else
                "separate" if fused_phases else None),
    )


# what each path row reaches, for the LDL^T formulations and for "none" (Bunch-Kaufman: no K0, no fused solve)
def _want(phases, initialize, pre, factor, k0, solves):
    return dict(phases=phases, initialize=initialize, pre=pre, factor=factor, factor_reads_k0=k0, solves=solves)


_K0_16 = _want("fused", "KMODE_K0_OFFDIAG", "KMODE_K0_DIAG", "small", True, "k_fused_solves<16>")
_BK_FUSED = _want("fused", None, "KMODE_K", "bk", False, "separate")
REACHES = {
    "k0-w16-S1": (_K0_16, _BK_FUSED),
    "k0-w16-S2": (_K0_16, _BK_FUSED),
    "k0-w16-S0": (_K0_16, _BK_FUSED),
    "k0-w8": (dict(_K0_16, solves="k_fused_solves<8>"), _BK_FUSED),
    "separate": (dict(_K0_16, solves="separate"), _BK_FUSED),
    "no-k0": (dict(_K0_16, pre="KMODE_K", factor_reads_k0=False), _BK_FUSED),
    "nbi128": (_want("fused", "KMODE_K0_OFFDIAG", "KMODE_K", "chain", False, "separate"), _BK_FUSED),
    "nonfused": (_want("nonfused", None, None, "chain", False, None), _want("nonfused", None, None, "bk", False, None)),
    "k0-w16-SP": (_K0_16, None),
    "nonfused-SPL": (_want("nonfused", None, None, "chain", False, None), None),
}


@pytest.mark.parametrize("pid,form", fc.CASES, ids=fc.CASE_IDS)
def test_path_row_reaches_what_it_names(pid, form):
    path = fc.PATHS[pid]
    n, m, p = path.shape
    N = fc.kkt_order(form, path.shape)
    assert N == {"naive": n + 2 * m + p, "naiveeq": n + 2 * (m + p)}.get(form, n + m + p)
    B = fc.batch_of(path)
    assert B > 1
    got = dispatch(N, B, 128 if path.ctx == "nbi128" else 64, path.mask, form == "none")
    assert got == REACHES[pid][form == "none"], (pid, form, N)
    if path.shape == fc.S1:  # every loop a single pass
        assert N <= fc.FT and n <= fc.PRE_UNIT
    if path.shape == fc.S2:  # the 512-thread loops stride, rows hold several copy units, still fused
        assert fc.FT < N <= fc.FUSED_NMAX and n > fc.PRE_UNIT
    if path.shape == fc.SL:
        assert N > fc.FUSED_NMAX
    if path.shape == fc.S0:
        assert m == 0 and form in fc.S0_FORMS
    if path.shape in (fc.SP, fc.SPL):  # the update's third bound
        assert p > max(n, m) and form in fc.SP_FORMS
        assert (N <= fc.FT) if path.shape == fc.SP else (N > fc.FUSED_NMAX)


def test_table_shape():
    assert list(fc.FORMS) == ["box", "vlo", "vup", "vnone", "alo", "aup", "sl", "naive", "pen", "none", "eqss", "naiveeq"]
    assert list(fc.PATHS) == list(REACHES)
    assert len(fc.CASES) == 7 * 12 + 8 + 2 * 3
    assert [fc.kkt_order(f, fc.S1) for f in ("box", "naive", "naiveeq")] == [72, 88, 96]
    assert [fc.kkt_order(f, fc.S2) for f in ("box", "naive", "naiveeq")] == [760, 900, 960]
    assert [fc.kkt_order(f, fc.SL) for f in ("box", "naive", "naiveeq")] == [1040, 1240, 1280]
    assert fc.PATHS["k0-w8"].B is None and fc.batch_of(fc.PATHS["k0-w8"]) == 257


# ---------------------------------------------------------------------------
# 2. ipmz_batch_create refuses none of the combinations
def refusal(n, m, p, B, kw, N):
    """create_solver's checks (csrc/qp.cpp), in its order; None: accepted."""
    import ipmz_amd as I
    eh, ih = kw.get("equality_handling", 0), kw.get("inequality_handling", 0)
    ib, vb = kw.get("inequality_bounds", 0), kw.get("variable_bounds", 0)
    if n <= 0 or m < 0 or p < 0 or B <= 0:
        return "dimensions"
    if eh == I.EQ_NONE and B > 1 and N > 4096:
        return "EqualityHandling::None in batches"
    if ih == I.INEQ_NAIVE_SLACKS and m > 0 and ib != I.BOUNDS_BOTH:
        return "InequalityHandling::NaiveSlacks: both inequality bounds"
    if eh == I.EQ_NAIVE_SLACKS and (ih != I.INEQ_NAIVE_SLACKS or ib != I.BOUNDS_BOTH):
        return "EqualityHandling::NaiveSlacks"
    if eh == I.EQ_SLACKED_SLACKS and (ih != I.INEQ_SLACKED_SLACKS or ib != I.BOUNDS_BOTH):
        return "EqualityHandling::SlackedSlacks"
    if m > 0 and ib == I.BOUNDS_NONE:
        return "inequality rows need a lower or an upper bound"
    if ih == I.INEQ_SLACKS and ((m > 0 and ib != I.BOUNDS_BOTH) or vb != I.BOUNDS_BOTH):
        return "InequalityHandling::Slacks is built on both bounds"
    return None


def test_no_tabled_combination_is_refused():
    qp = _src("qp.cpp")
    for line in (
        "  if (cfg->equality_handling == IPMZ_EQ_NONE && B > 1 && cfg->n + mk + cfg->p > IPMZ_BK_NMAX)",
        "  if (ih == IPMZ_INEQ_NAIVE_SLACKS && cfg->m > 0 && ib != IPMZ_BOUNDS_BOTH)",
        "  if (cfg->equality_handling == IPMZ_EQ_NAIVE_SLACKS && (ih != IPMZ_INEQ_NAIVE_SLACKS || ib != IPMZ_BOUNDS_BOTH))",
        "  if (cfg->equality_handling == IPMZ_EQ_SLACKED_SLACKS && (ih != IPMZ_INEQ_SLACKED_SLACKS || ib != IPMZ_BOUNDS_BOTH))",
        "  if (cfg->m > 0 && ib == IPMZ_BOUNDS_NONE)",
        "  if (ih == IPMZ_INEQ_SLACKS && ((cfg->m > 0 && ib != IPMZ_BOUNDS_BOTH) || vb != IPMZ_BOUNDS_BOTH))",
    ):
        assert line in qp, line
    assert "#define IPMZ_BK_NMAX 4096" in _src("kernels.h")
    refused = {}
    for pid, form in fc.CASES:
        path = fc.PATHS[pid]
        why = refusal(*path.shape, fc.batch_of(path), fc.FORMS[form].kw, fc.kkt_order(form, path.shape))
        if why:
            refused[pid, form] = why
    assert refused == fc.REFUSED == {}
    # the one-sided inequality bounds S0 (m = 0) leaves out are not a refusal either: there is nothing to bound
    assert set(fc.FORMS) - set(fc.S0_FORMS) == {"alo", "aup", "naive", "naiveeq"}


def test_more_equality_rows_than_variables_conditioning():
    """Why SP / SPL hold three formulations: the 2-norm condition number of the
    initial KKT matrix at SP, below 1e2 for them and above 1e8 for the others
    (bounds of 1e-9 on a direction need cond x 2^-53 well below that)."""
    import numpy as np
    for form in fc.FORMS:
        K = np.tril(fc.oracles(form, fc.SP, 1, fc.seed0(fc.SP, form))[0].kkt())
        cond = np.linalg.cond(K + np.tril(K, -1).T)
        assert (cond < 1e2) if form in fc.SP_FORMS else (cond > 1e8), (form, cond)


# ---------------------------------------------------------------------------
# 3. the convergence windows
@functools.lru_cache(maxsize=None)
def _converged_in_window(form, shape, B, seed, steps):
    """(QP, step) at which iterate() reports a converged iterate: none wanted.
    One call more than the window's steps: the iterate the last step leaves
    is not converged either (the GPU test asserts converged == 0 after every
    step)."""
    bad = []
    for i, o in enumerate(fc.oracles(form, shape, B, seed)):
        for it in range(steps + 1):
            if o.iterate()[0] != 0:
                bad.append((i, it))
    return tuple(bad)


@pytest.mark.parametrize("pid,form", fc.CASES, ids=fc.CASE_IDS)
def test_window_has_no_converged_qp(pid, form):
    path = fc.PATHS[pid]
    B = fc.batch_of(path)  # k0-w8: the first 257 seeds
    assert _converged_in_window(form, path.shape, B, fc.seed0(path.shape, form), path.steps) == ()


def _count(o):
    """iterate() returns done != 0 (and leaves the iterate alone) once the
    iterate it is given has converged: the number of Newton steps before that."""
    k = 0
    while k < 50 and o.iterate()[0] == 0:
        k += 1
    return k


def test_solve_table_lists_every_converging_formulation():
    assert list(fc.SOLVE) == [f for f in fc.FORMS if f != "sl"]
    assert fc.SOLVE_SHAPE == fc.PATHS["k0-w16-S1"].shape and fc.SOLVE_B == fc.PATHS["k0-w16-S1"].B
    assert {f: s for f, (s, _) in fc.SOLVE.items() if s != 7} == {"vnone": 1224}
    # Slacks (the reference's corrector defect) does not converge
    assert [_count(o) for o in fc.oracles("sl", fc.SOLVE_SHAPE, fc.SOLVE_B, 7)] == [50] * fc.SOLVE_B


@pytest.mark.parametrize("form", list(fc.SOLVE))
def test_solve_seeds_iteration_counts(form):
    seed, iters = fc.SOLVE[form]
    counts = tuple(_count(o) for o in fc.oracles(form, fc.SOLVE_SHAPE, fc.SOLVE_B, seed))
    assert counts == iters
    assert len(set(counts)) >= 2  # some QP freezes while another steps
    # the restart test's 12 steps: every QP converges, restarts and steps on
    assert max(counts) + 1 < fc.RESTART_STEPS


def test_vnone_counts_at_the_common_seeds():
    """Why vnone has a seed0 of its own: no two of seeds 7 .. 9 differ."""
    assert [_count(o) for o in fc.oracles("vnone", fc.SOLVE_SHAPE, fc.SOLVE_B, 7)] == [5, 5, 5]
