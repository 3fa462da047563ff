"""The conditions tests/test_gpu_batch_large.py relies on, checked on the CPU:

  * no comparison is skipped: for every (shape, seed, step) of its two tables
    the oracle's iterate() returns done == 0 (no QP converges inside the
    compared window);
  * the freeze / restart shapes converge after 8, 10 and 8 oracle iterations
    (the freeze test relies on the counts differing);
  * the blocking each case is meant to reach -- a pure-Python restatement of
    nbo_for (csrc/capi.h) -- and the panel, trailing-order and strip-row
    figures that follow from it, against the dispatch thresholds read from the
    kernel sources.
"""
import os
import re

import pytest

import batch_large_cases as bc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipm-zoo_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_thresholds_match_the_sources():
    kernels, trsv, ldlt, capi = _src("kernels.h"), _src("trsv_small.h"), _src("ldlt.hip"), _src("capi.h")
    assert int(re.search(r"#define IPMZ_FUSED_NMAX (\d+)", kernels).group(1)) == bc.FUSED_NMAX
    assert int(re.search(r"#define IPMZ_SMALL_NMAX (\d+)", kernels).group(1)) == bc.SMALL_NMAX
    assert int(re.search(r"#define IPMZ_TRAIL_SMALL_M (\d+)", kernels).group(1)) == bc.TRAIL_SMALL_M
    assert int(re.search(r"constexpr int TRSV_SMALL_NMAX = (\d+);", trsv).group(1)) == bc.TRSV_SMALL_NMAX
    # the strip instances of gemm_nt_sub_t, in the order it tries them
    strips = re.findall(r"if \(M <= (\d+)\) return launch_gemm<(\d+), (\d+), EPI_SUB_STRIP", ldlt)
    assert strips == [(str(bc.STRIP_64_M), "64", "64"), (str(bc.STRIP_128_M), "64", "128")]
    # nbo_for's rule
    assert "if (ctx->nbi != 64 || N < 2048) return 256;" in capi
    assert "return N <= 4096 ? 384 : 512;" in capi


def test_nbo_rule():
    assert [bc.nbo_for(N) for N in (1, 2047, 2048, 4096, 4097, 20000)] == [256, 256, 384, 384, 512, 512]
    assert [bc.nbo_for(N, nbi=128) for N in (65, 2048, 4200)] == [256, 256, 256]
    assert bc.nbo_for(4200, nbo=128) == 128


def test_nonfused_table_reaches_what_it_names():
    by_N = {}
    for n, m, p, B, seed0, steps, nbo in bc.NONFUSED:
        N = n + m + p
        assert B > 1 and N > bc.FUSED_NMAX, N  # run_step's else branch, and the kernel-chain factor
        assert bc.nbo_for(N) == nbo, N
        by_N[N] = (n, m, p, nbo)
    assert sorted(by_N) == [1030, 1040, 1050, 2048, 4200]
    # 1040: the smallest tabled N past 1024; five outer panels, the last 16 rows; 17 inner blocks, the last ragged
    assert -(-1040 // 256) == 5 and 1040 - 4 * 256 == 16
    assert -(-1040 // 64) == 17 and 1040 % 64 == 16
    assert by_N[1030][1] == 0 and by_N[1050][2] == 0  # m = 0, p = 0
    # 2048: a multiple of 64, not of its nbo
    assert by_N[2048][3] == 384 and 2048 % 64 == 0 and 2048 % 384 != 0
    # the solves: trsv_small_kernel up to 4096, trsv_batched_kernel<64> above
    assert all(N <= bc.TRSV_SMALL_NMAX for N in by_N if N != 4200) and 4200 > bc.TRSV_SMALL_NMAX
    # 4200: the first trailing update (below the first outer panel) and the first strip (below the first
    # inner block) run the large instances; no strip reaches the 128 x 128 one
    nbo = by_N[4200][3]
    assert nbo == 512
    assert 4200 - nbo == 3688 > bc.TRAIL_SMALL_M
    assert bc.STRIP_64_M < 4200 - 64 == 4136 <= bc.STRIP_128_M
    # ... while every other case stays on the 64 x 64 instances
    for N, (_, _, _, nbo) in by_N.items():
        if N != 4200:
            assert N - nbo <= bc.TRAIL_SMALL_M and N - 64 <= bc.STRIP_64_M, N


def test_nbi128_table_block_counts():
    blocks = {}
    for n, m, p, B, seed0, steps in bc.NBI128:
        N = n + m + p
        assert B > 1 and bc.nbo_for(N, nbi=128) == 256
        blocks.setdefault(N, [min(128, N - j) for j in range(0, N, 128)])
    assert blocks[65] == [65]
    assert blocks[128] == [128]
    assert blocks[129] == [128, 1]
    assert blocks[320] == [128, 128, 64]
    assert blocks[1040] == [128] * 8 + [16]
    assert sum(1 for c in bc.NBI128 if c[2] > 0 and sum(c[:3]) == 128) == 1  # equality rows at exactly one block
    assert all(N <= bc.FUSED_NMAX for N in blocks if N != 1040) and 1040 > bc.FUSED_NMAX


def _not_done_for(n, m, p, B, seed0, steps):
    for i, o in enumerate(bc.oracles(n, m, p, B, seed0)):
        for it in range(steps):
            done, _ = o.iterate()
            assert done == 0, (n, m, p, seed0 + i, it)


@pytest.mark.parametrize("case", bc.NONFUSED, ids=lambda c: f"N{sum(c[:3])}")
def test_nonfused_window_has_no_converged_qp(case):
    n, m, p, B, seed0, steps, _ = case
    _not_done_for(n, m, p, B, seed0, steps)


@pytest.mark.parametrize("case", bc.NBI128, ids=lambda c: f"N{sum(c[:3])}-seed{c[4]}")
def test_nbi128_window_has_no_converged_qp(case):
    _not_done_for(*case)


def test_solve_seeds_iteration_counts():
    """iterate() returns done != 0 (and leaves the iterate alone) once the
    iterate it is given has converged: the number of Newton steps before that."""
    n, m, p = bc.SOLVE_SHAPE
    counts = []
    for o in bc.oracles(n, m, p, len(bc.SOLVE_SEEDS), bc.SOLVE_SEEDS[0]):
        k = 0
        while k < 50 and o.iterate()[0] == 0:
            k += 1
        counts.append(k)
    assert tuple(counts) == bc.SOLVE_ITERS
    assert counts[1] > counts[0] == counts[2]  # QPs 0 and 2 freeze while QP 1 goes on
    # the restart test's 12 steps: every QP converges, restarts and steps on
    assert max(counts) + 1 < 12
    # ... and the graph test's 4 steps see no restart
    assert min(counts) > 4
