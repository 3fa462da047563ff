"""Shapes of the batched Newton steps past the fused-kernel limits, shared by
tests/test_gpu_batch_large.py (the steps on the device) and
tests/test_oracle_batch_large.py (the conditions the shapes rely on, checked
without a GPU).

Every QP of a batch is oracle.gen_qp(n, m, p, seed0 + i), as Batch.generate.
"""
import functools

import oracle

# csrc/kernels.h, csrc/trsv_small.h (test_oracle_batch_large.py checks them against the sources)
FUSED_NMAX = 1024       # IPMZ_FUSED_NMAX: B > 1 and N <= this -> the per-QP k_fused_* phases
SMALL_NMAX = 1024       # IPMZ_SMALL_NMAX: nbi 64 and N <= this -> the one-workgroup factors of small.hip
TRSV_SMALL_NMAX = 4096  # nbi 64 and N <= this -> trsv_small_kernel, above it trsv_batched_kernel<64>
TRAIL_SMALL_M = 3072    # IPMZ_TRAIL_SMALL_M: trailing order above this -> the 128 x 128 EPI_SUB instance
STRIP_64_M = 4096       # ldlt.hip gemm_nt_sub_t: strip rows above this -> the 64 x 128 strip instance,
STRIP_128_M = 8192      # above this the 128 x 128 one (out of reach at test cost)

# (n, m, p, B, seed0, steps, nbo) on the default context (nbi 64)
NONFUSED = [
    (800, 200, 40, 3, 100, 3, 256),
    (1000, 0, 30, 2, 200, 2, 256),
    (900, 150, 0, 2, 300, 2, 256),
    (1500, 400, 148, 2, 400, 2, 384),
    (3300, 700, 200, 2, 500, 1, 512),
]
# (n, m, p, B, seed0, steps) on a context with nbi 128 (nbo 256 at every N)
NBI128 = [
    (52, 13, 0, 2, 4052, 3),
    (100, 28, 0, 3, 4100, 3),
    (103, 26, 0, 3, 4103, 3),
    (256, 64, 0, 4, 0, 3),
    (96, 24, 8, 3, 7, 3),
    (800, 200, 40, 2, 100, 2),
]
# freeze / restart / solve_all / graph replay: seeds and the oracle's iterations to convergence
SOLVE_SHAPE = (800, 200, 40)
SOLVE_SEEDS = (100, 101, 102)
SOLVE_ITERS = (8, 10, 8)


def nbo_for(N, nbo=0, nbi=64):
    """Outer panel width of an order-N factor (csrc/capi.h nbo_for)."""
    if nbo:
        return nbo
    if nbi != 64 or N < 2048:
        return 256
    return 384 if N <= 4096 else 512


@functools.lru_cache(maxsize=None)
def _qp_cached(n, m, p, seed):
    return oracle.gen_qp(n, m, p, seed)


def qp(n, m, p, seed):
    """The generated QP, never modified; the shapes several tests share are
    made once per session (the N = 4200 ones, 87 MB each, are not kept)."""
    return _qp_cached(n, m, p, seed) if n <= 1500 else oracle.gen_qp(n, m, p, seed)


def oracles(n, m, p, B, seed0):
    """Fresh oracle runs (at the initial iterate) of the B QPs of a batch."""
    return [oracle.OracleQP(qp(n, m, p, seed0 + i)) for i in range(B)]
