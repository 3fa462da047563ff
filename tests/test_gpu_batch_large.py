"""Batched Newton steps past the fused-kernel limits: batches with KKT order
N > 1024 (IPMZ_FUSED_NMAX) and batches on a context whose inner block is 128,
through the public ABI only, every QP against its own oracle run.

What a batch runs there that no other test launches with more than one QP:
  * the non-fused step with gridDim.y = B (run_step's else branch: k_assemble,
    k_rhs, k_backsub, k_ratio_part, k_mu_aff_part / final, k_corrector,
    k_update, k_restart_copy / scal and the evaluation);
  * the batched kernel-chain factor (ldlt_factor_batched -> factor_panel /
    panel_update with BatchStrides): ldlt_diag64_blk_kernel or
    ldlt_diag_kernel<double, 128> with B workgroups, the EPI_PANEL TRSM with
    its five strides, and every strip and trailing update on gemm.h's
    register-staged fp64 engine (a batch skips gemm64.h's kernels);
  * the batched solves outside the fused launch: trsv_small_kernel<16> at
    1024 < N <= 4096, trsv_batched_kernel<64> above, trsv_batched_kernel<128>
    on an nbi = 128 context;
  * nbi = 128 batches at small N: KMODE_K assembly in the fused pre phase and
    qp_fused_mid / qp_fused_post as separate launches around the solves.

The shapes are tests/batch_large_cases.py's; tests/test_oracle_batch_large.py
checks on the CPU that no QP converges inside a compared window and that each
shape has the blocking it is meant to reach (asserted here against the
context as well).  Not reached: the 128 x 128 strip instance (strips of more
than 8192 rows; one oracle iteration at that order costs minutes) and batches
of more than 256 QPs at N > 1024.

Bounds (BASELINE.json north star, test_gpu_parity.py): the initial iterate
bitwise; f, res, mu within 1e-12 relative; alpha_aff, mu_aff, sigma, alpha
and every block of both directions within 1e-9 relative;
||dx_gpu - dx_cpu||_inf < 1e-10.  After every step each QP is reset to its
oracle's iterate.  Every case prints its worst figures before asserting them.
(The bounds and the comparison helpers live in tests/batch_compare.py, shared
with tests/test_gpu_batch_forms.py -- whose loop does not reset the batch: the
reset re-evaluates every QP with the non-fused qp_evaluate.)
"""
import numpy as np
import pytest

import batch_large_cases as bc
import oracle
from batch_compare import DX_TOL, STATE_KEYS, Worst, _compare_step, _rel
from golden_io import load, trace

pytestmark = pytest.mark.gpu
I = pytest.importorskip("ipmz_amd")


@pytest.fixture(scope="module")
def ctx():
    return I.Context(0)


@pytest.fixture(scope="module")
def ctx128():
    """A context of its own with nbi = 128: the blocking is set before any
    Batch is sized for it and never changed."""
    c = I.Context(0, nbi=128)
    yield c
    c.close()


def _steps_vs_oracle(bt, orcs, steps, w):
    """test_batch_steps_vs_oracle's loop with every bound of the parity tests."""
    for i, o in enumerate(orcs):
        assert np.array_equal(bt.state(i, 0), o.vars()), i  # generator + initial iterate: bitwise
    for it in range(steps):
        sc0 = bt.batch_scalars()
        recs = []
        for i, o in enumerate(orcs):
            done, rec = o.iterate()
            assert done == 0, (it, i)  # (test_oracle_batch_large.py: never inside these windows)
            recs.append(rec)
        bt.step()
        sc = bt.batch_scalars()
        for i, o in enumerate(orcs):
            for k in STATE_KEYS:  # the evaluation of the iterate the step started from
                w.add("f/res/mu rel", _rel(sc0[i, I.SC[k]], recs[i][k]), (it, i, k))
            _compare_step(w, o, recs[i], sc[i], bt.state(i, 1), bt.state(i, 2), (it, i))
            bt.set_state(i, o.vars())


# ---------------------------------------------------------------------------
# 1. non-fused batched steps, default context (nbi = 64)
@pytest.mark.parametrize("case", bc.NONFUSED, ids=lambda c: f"N{sum(c[:3])}")
def test_nonfused_batch_steps_vs_oracle(ctx, case):
    """N = 1040, 1030 (m = 0), 1050 (p = 0), 2048 (nbo 384) and 4200 (nbo 512,
    the 128 x 128 trailing and 64 x 128 strip instances, trsv_batched_kernel<64>).

    The 1e-10 bound on dx at N = 4200 comes from the single-QP Optimizer
    (the panel path, other kernels than the batch's) stepped from the same
    iterate on seed 500: where it meets 1e-10 against the oracle the batch must
    too; otherwise the batch's bound is four times its error (a factor 2 for
    the summation order of gemm.h's tiles, one for run-to-run placement of the
    maximum).  Measured on an MI355X: the single-QP Optimizer 3.442e-15, the
    batch 3.164e-15 -- the bound is 1e-10 (worst over the other four cases:
    dx 2.6e-15, direction blocks 5.4e-15, scalars 1.1e-15, f / res / mu
    3.2e-15 relative)."""
    n, m, p, B, seed0, steps, nbo = case
    N = n + m + p
    assert ctx.blocking(N) == (nbo, 64)
    assert B > 1 and N > bc.FUSED_NMAX
    orcs = bc.oracles(n, m, p, B, seed0)
    bounds = {}
    if N > 4096:
        g = I.Optimizer(n, m, p, ctx)
        g.generate(seed0)
        ref = oracle.OracleQP(bc.qp(n, m, p, seed0))
        assert np.array_equal(g.vars(), ref.vars())
        ref.iterate()
        g.step()
        single = max(np.abs(g.daff()[:n] - ref.daff()[:n]).max(), np.abs(g.dir()[:n] - ref.dir()[:n]).max())
        g.close()
        del ref
        bounds["|dx - dx_cpu|"] = DX_TOL if single < DX_TOL else 4.0 * single
        print(f"N={N}: single-QP Optimizer |dx - dx_cpu| {single:.3e} -> batch bound {bounds['|dx - dx_cpu|']:.3e}",
              flush=True)
    bt = I.Batch(n, m, p, B, ctx)
    bt.generate(seed0)
    w = Worst(f"nonfused N={N} B={B}", bounds)
    _steps_vs_oracle(bt, orcs, steps, w)
    bt.close()
    w.check()


# ---------------------------------------------------------------------------
# 2. freeze, restart and solve_all through the non-fused kernels
def _solve_oracles():
    n, m, p = bc.SOLVE_SHAPE
    return bc.oracles(n, m, p, len(bc.SOLVE_SEEDS), bc.SOLVE_SEEDS[0])


def test_nonfused_solve_all_and_freeze(ctx):
    """solve_all on seeds 100..102 (8, 10 and 8 oracle iterations): all three
    converge after 10 steps with every x within 1e-7 of its oracle's
    (test_batch_solve_all_matches_single's bound); a second batch stepped by
    hand converges QP by QP after the oracle's counts, QPs 0 and 2 keep their
    iterate and its evaluation bitwise over the two steps QP 1 still takes
    (freeze = 1 in k_update), and ends bitwise where solve_all did."""
    n, m, p = bc.SOLVE_SHAPE
    B = len(bc.SOLVE_SEEDS)
    orcs = _solve_oracles()
    for o in orcs:
        while o.iterate()[0] == 0:
            pass
    bt = I.Batch(n, m, p, B, ctx)
    bt.generate(bc.SOLVE_SEEDS[0])
    its, nconv = bt.solve_all(100)
    assert (its, nconv) == (max(bc.SOLVE_ITERS), B)
    worst = max(np.abs(bt.state(i, 0)[:n] - o.vars()[:n]).max() for i, o in enumerate(orcs))
    print(f"solve_all: worst |x - x_cpu| {worst:.3e} (bound 1e-7)", flush=True)
    assert worst < 1e-7

    hb = I.Batch(n, m, p, B, ctx)
    hb.generate(bc.SOLVE_SEEDS[0])
    first = [None] * B  # steps taken when QP i first reports converged
    frozen = {}
    keep = [I.SC[k] for k in STATE_KEYS + ("converged",)]
    for it in range(1, max(bc.SOLVE_ITERS) + 1):
        hb.step()
        sc = hb.batch_scalars()
        for i in range(B):
            if sc[i, I.SC["converged"]] != 0.0 and first[i] is None:
                first[i] = it
                frozen[i] = (hb.state(i, 0), sc[i, keep].copy())
            elif first[i] is not None:
                assert np.array_equal(hb.state(i, 0), frozen[i][0]), (it, i)
                assert np.array_equal(sc[i, keep], frozen[i][1]), (it, i)
    assert tuple(first) == bc.SOLVE_ITERS
    for i in range(B):
        assert np.array_equal(hb.state(i, 0), bt.state(i, 0)), i
    bt.close()
    hb.close()


def test_nonfused_restart_vs_oracle(ctx):
    """STEP_RESTART_IF_CONVERGED for 12 steps (k_restart_copy / k_restart_scal
    with gridDim.y = 3): each step against the oracle from the pre-step
    iterate, or from the initial one when the QP had converged before the
    step; every QP restarts at least once."""
    n, m, p = bc.SOLVE_SHAPE
    B = len(bc.SOLVE_SEEDS)
    orcs = _solve_oracles()
    init = [o.vars() for o in orcs]
    bt = I.Batch(n, m, p, B, ctx)
    bt.generate(bc.SOLVE_SEEDS[0])
    w = Worst("nonfused restart N=1040 B=3")
    restarts = [0] * B
    for it in range(12):
        pre = [bt.state(i, 0) for i in range(B)]
        conv = bt.batch_scalars()[:, I.SC["converged"]].copy()
        bt.step(I.STEP_RESTART_IF_CONVERGED)
        sc = bt.batch_scalars()
        for i, o in enumerate(orcs):
            if conv[i]:
                restarts[i] += 1
            o.set_vars(init[i] if conv[i] else pre[i])
            done, rec = o.iterate()
            assert done == 0, (it, i)
            _compare_step(w, o, rec, sc[i], bt.state(i, 1), bt.state(i, 2), (it, i))
        assert np.array_equal(sc[:, I.SC["restarts"]], np.array(restarts, dtype=float)), it
    bt.close()
    w.check()
    assert min(restarts) >= 1, restarts


# ---------------------------------------------------------------------------
# 3. graph replay and determinism of the non-fused batched step
def _snapshot(bt):
    return bt.batch_scalars(), [[bt.state(i, w) for w in range(3)] for i in range(bt.batch)]


def _assert_same(a, b, label):
    assert np.array_equal(a[0], b[0]), label
    for i, (sa, sb) in enumerate(zip(a[1], b[1])):
        for w in range(3):
            assert np.array_equal(sa[w], sb[w]), (label, i, w)


def test_nonfused_graph_replay_bitwise(ctx):
    """RESTART | GRAPH against the eager step, 4 steps: scalars, iterate and
    both directions bitwise, the graph replayed from the second step on (the
    step is single-stream: its captured graph has no parallel branches)."""
    n, m, p = bc.SOLVE_SHAPE
    gb, eb = I.Batch(n, m, p, 2, ctx), I.Batch(n, m, p, 2, ctx)
    gb.generate(100)
    eb.generate(100)
    for it in range(4):
        gb.step(I.STEP_RESTART_IF_CONVERGED | I.STEP_GRAPH)
        eb.step(I.STEP_RESTART_IF_CONVERGED)
        if it >= 1:
            assert gb.last_step_graph(), it
        assert not eb.last_step_graph(), it
        _assert_same(_snapshot(gb), _snapshot(eb), it)
    gb.close()
    eb.close()


def test_nonfused_eager_steps_run_to_run_bitwise(ctx):
    """Two batches from the same seed, 3 eager steps each: bitwise (each
    element of C is written by one launch in a fixed k order)."""
    n, m, p = bc.SOLVE_SHAPE
    a, b = I.Batch(n, m, p, 2, ctx), I.Batch(n, m, p, 2, ctx)
    a.generate(100)
    b.generate(100)
    for it in range(3):
        a.step()
        b.step()
        _assert_same(_snapshot(a), _snapshot(b), it)
    a.close()
    b.close()


# ---------------------------------------------------------------------------
# 4. batches on an nbi = 128 context
@pytest.mark.parametrize("case", bc.NBI128, ids=lambda c: f"N{sum(c[:3])}-seed{c[4]}")
def test_nbi128_batch_steps_vs_oracle(ctx128, case):
    """One ragged block (N = 65), exactly one (128), one plus a row (129),
    128 + 128 + 64 (320; QP 0 also against the reference's c4_it* golden
    vectors, as test_batch_c4_golden), equality rows (128) and the non-fused
    phases together with the 128 chain (1040)."""
    n, m, p, B, seed0, steps = case
    N = n + m + p
    assert ctx128.blocking(N) == (256, 128)
    bt = I.Batch(n, m, p, B, ctx128)
    bt.generate(seed0)
    w = Worst(f"nbi128 N={N} B={B}")
    _steps_vs_oracle(bt, bc.oracles(n, m, p, B, seed0), steps, w)
    if (n, m, p, seed0) == (256, 64, 0, 0):
        names, rows, _ = trace("c4")
        for it in range(len(rows)):
            bt.set_state(0, load(f"c4_it{it}_vars.bin"))
            bt.step()
            for which, tag in ((1, "daff"), (2, "d")):
                ref = load(f"c4_it{it}_{tag}.bin")
                got = bt.state(0, which)
                w.add("|dx - dx_cpu|", np.abs(got[:n] - ref[:n]).max(), ("golden", it, tag))
                w.add("direction blocks rel", np.abs(got - ref).max() / max(1.0, np.abs(ref).max()), ("golden", it, tag))
    bt.close()
    w.check()
