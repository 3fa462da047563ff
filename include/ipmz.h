/*
 * ipmz.h -- C ABI of libipmz, the MI355X (gfx950) implementation of
 * ipm-zoo's numerical interior-point Newton step.
 *
 * Drop-in boundary.  The reference has no FFI: its hot path
 * is a set of C++ free functions plus one class, all called from Optimizer.
 * Each entry point below replaces one of them:
 *
 *   ipmz_ldlt_decomposition     <- LinearSolvers::ldlt_decomposition
 *                                  (include/NumericalOptimization/LinearSolvers.h:11,
 *                                   src/NumericalOptimization/LinearSolvers.cpp:14-42)
 *   ipmz_overwriting_solve_ldlt <- LinearSolvers::overwriting_solve_ldlt
 *                                  (LinearSolvers.h:16-17, LinearSolvers.cpp:44-74)
 *   ipmz_ldlt_factor / _solve   <- the same pair on device-resident K (no copies)
 *   ipmz_ldlt_solve_multi, ipmz_overwriting_solve_ldlt_multi, ipmz_qp_kkt_solve
 *                               <- no reference counterpart (the reference solves one
 *                                  vector at a time): overwriting_solve_ldlt for a block
 *                                  of right-hand sides, one per row, as a blocked
 *                                  triangular solve that reads L once per sweep
 *   ipmz_mixed_solve_multi, ipmz_qp_kkt_solve_mixed, ipmz_sym_residual_multi
 *                               <- no reference counterpart either: the same block of
 *                                  right-hand sides through the fp32 factor (blocked fp32
 *                                  solve) with fp64 refinement and a per-row stop test;
 *                                  the refinement's residual R = B - X K on its own
 *   ipmz_bk_prepare_solve, ipmz_bk_solve_multi, ipmz_overwriting_solve_bunch_kaufman_multi,
 *   ipmz_qp_kkt_solve_bk, ipmz_normal_solve_multi
 *                               <- no reference counterpart: overwriting_solve_bunch_kaufman
 *                                  and the normal-equations solve for a block of right-hand
 *                                  sides, on the same blocked triangular solve
 *   ipmz_batch_get_kkt, ipmz_batch_kkt_solve
 *                               <- no reference counterpart: the KKT matrix of any QP of
 *                                  a batch, and ipmz_qp_kkt_solve for every QP of a batch at
 *                                  once (one launch per batch where a QP's right-hand sides
 *                                  fit a workgroup's LDS)
 *   ipmz_bk_factor_batch, ipmz_bk_prepare_solve_batch, ipmz_bk_solve_multi_batch,
 *   ipmz_batch_kkt_solve_bk
 *                               <- no reference counterpart: the one-workgroup
 *                                  Bunch-Kaufman factor and the prepared multi-right-hand-side
 *                                  solve for a batch of systems of one order (N <= 4096) on
 *                                  caller-owned storage, and ipmz_qp_kkt_solve_bk for every
 *                                  QP of an IPMZ_EQ_NONE batch at once
 *   ipmz_batch_load_device, ipmz_batch_copy_state
 *                               <- no reference counterpart: build_environment for a whole
 *                                  batch from device memory (strided blocks, shared or per
 *                                  QP, validated and copied by kernels), and the state of
 *                                  every QP in the reference's Newton order to device memory
 *   ipmz_batch_set_state_device
 *                               <- no reference counterpart: the iterate of a whole batch
 *                                  set from such rows in device memory (a warm start),
 *                                  pushed into the interior and checked by kernels
 *   ipmz_batch_solve_ex, ipmz_batch_can_skip_converged
 *                               <- the loop of Optimizer::solve_quasi_definite_ for a whole
 *                                  batch with the reference's per-QP stop (Optimizer.cpp:
 *                                  133-135) kept on the device: a converged QP takes no part
 *                                  in any launch of a step (IPMZ_STEP_SKIP_CONVERGED), and
 *                                  the host looks at the device every few steps only
 *   ipmz_qp_create + ipmz_qp_load_host
 *                               <- NumericalOptimization::build_environment
 *                                  (EnvironmentBuilder.h:19-20, EnvironmentBuilder.cpp:7-76)
 *                                  + Optimizer::Optimizer (Optimizer.h:15-18)
 *   ipmz_qp_step                <- one body of Optimizer::solve_quasi_definite_
 *                                  (Optimizer.cpp:127-219): assembly
 *                                  (get_as_matrix_, :387-391), factor, two
 *                                  compute_search_direction_ (:344-380), two
 *                                  get_max_step_ (:270-342), update (:222-231)
 *   ipmz_qp_solve               <- Optimizer::solve (Optimizer.h:20, Optimizer.cpp:63-73)
 *   ipmz_qp_newton_solve_multi, ipmz_batch_newton_solve_multi
 *                               <- the multi-row form of Optimizer::compute_search_direction_
 *                                  (:344-380) with get_max_step_ (:270-342): full residual
 *                                  vectors r_v of the Newton system in, full Newton
 *                                  directions and their maximum steps out, any number of
 *                                  rows from one factor, for a QP or every QP of a batch
 *   ipmz_qp_newton_adjoint_multi, ipmz_batch_newton_adjoint_multi
 *                               <- no reference counterpart: the transpose of the map above
 *                                  (J^T out = -g), cotangents of directions in, cotangents
 *                                  with respect to the residual vectors out, from the same
 *                                  factor and blocked solves
 *   ipmz_batch_data_vjp         <- no reference counterpart: that cotangent contracted with
 *                                  d r_v / d (Q, c, A, l_A, u_A, C, d, l_x, u_x), the gradient
 *                                  with respect to the problem data in the strided blocks
 *                                  ipmz_batch_load_device reads (per QP, or summed over the
 *                                  batch for shared blocks)
 *   ipmz_batch_data_vjp_multi   <- the same for a block of cotangent rows per QP (the adjoint
 *                                  pair's nrhs rows): reverse-mode Jacobians in one call
 *   ipmz_batch_data_jvp         <- no reference counterpart: the forward-mode counterpart,
 *                                  tangents of the data (ntan per QP, or one set shared by
 *                                  the batch) to the residual rows d r_v / d data applied to
 *                                  them, the input of ipmz_*_newton_solve_multi
 *   ipmz_batch_center           <- no reference counterpart: Newton iterations from a solved
 *                                  iterate onto the central path at a fixed barrier parameter
 *                                  kappa (r(z; mu = kappa) = 0), where the derivative calls
 *                                  above are exact at any active set
 *
 * Conventions
 *   - Plain pointers and sizes only.  "device" pointers are HIP device
 *     memory on the context's device, "host" pointers are ordinary memory.
 *   - Dense matrices are row-major.  K is symmetric; only its lower triangle
 *     (i >= j) is read, and the factor overwrites the strict lower triangle
 *     with L (unit diagonal implicit) -- row-major lower == the reference's
 *     L[i][j], i > j.
 *   - Return value: 0 success; > 0 = 1-based index of the first non-finite
 *     pivot (the factorization still completes, as the reference's does);
 *     < 0 = error (IPMZ_ERR_*), message via ipmz_last_error().  The zero-pivot
 *     rule of the reference (an exactly-zero pivot becomes 1e-8,
 *     LinearSolvers.cpp:26-28) is not an error, as in the reference.
 *   - All device work is enqueued on the context's stream; functions whose
 *     outputs are host memory synchronize it.
 *   - There is no CPU fallback: without a usable gfx950 device every entry
 *     point that computes returns IPMZ_ERR_NO_DEVICE.
 */
#ifndef IPMZ_H
#define IPMZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPMZ_OK 0
#define IPMZ_ERR_INVALID (-1)
#define IPMZ_ERR_HIP (-2)
#define IPMZ_ERR_NOMEM (-3)
#define IPMZ_ERR_NO_DEVICE (-4)
#define IPMZ_ERR_STATE (-5)

/* Canonical Newton-variable slots.  The reference's Newton-variable order
 * (get_newton_system, SlackedSlacks + Regularization) is this order with the
 * absent blocks dropped; state vectors are concatenated in it. */
enum ipmz_slot {
  IPMZ_SLOT_X = 0, IPMZ_SLOT_LAMBDA_A, IPMZ_SLOT_LAMBDA_C, IPMZ_SLOT_S, IPMZ_SLOT_P,
  IPMZ_SLOT_LAMBDA_G, IPMZ_SLOT_LAMBDA_H, IPMZ_SLOT_LAMBDA_Y, IPMZ_SLOT_LAMBDA_Z,
  IPMZ_SLOT_G, IPMZ_SLOT_H, IPMZ_SLOT_Y, IPMZ_SLOT_Z, IPMZ_NSLOT
};

/* Per-iteration scalars (device block of IPMZ_SC_COUNT doubles). */
enum ipmz_scalar {
  IPMZ_SC_F = 0,        /* objective 0.5 x'Qx + c'x of the current iterate   */
  IPMZ_SC_RES,          /* ||full rhs at mu = 0||_2 (get_residual_norm_)      */
  IPMZ_SC_MU,           /* mean |complementarity| (get_mu_)                   */
  IPMZ_SC_ALPHA_AFF,    /* last step: affine step length                      */
  IPMZ_SC_MU_AFF,       /* last step: mu at the affine trial point            */
  IPMZ_SC_SIGMA,        /* last step: (mu_aff / mu)^3                         */
  IPMZ_SC_ALPHA,        /* last step: corrector step length (before 0.995)    */
  IPMZ_SC_CONVERGED,    /* 1.0 when res < 1e-8 and mu < 1e-8                  */
  IPMZ_SC_MU_NEW,       /* last step: sigma * mu                              */
  IPMZ_SC_RESTARTS,     /* benchmark restarts taken                           */
  IPMZ_SC_IR_RATIO_AFF, /* mixed precision: ||r||/||b|| reached, affine solve */
  IPMZ_SC_IR_ITERS_AFF, /*   refinement corrections, affine solve             */
  IPMZ_SC_IR_RATIO,     /*   the same for the corrector solve                 */
  IPMZ_SC_IR_ITERS,
  IPMZ_SC_STEPS = 14,   /* steps with IPMZ_STEP_SKIP_CONVERGED this QP took part in */
  IPMZ_SC_COUNT = 16
};

typedef struct ipmz_ctx ipmz_ctx;
typedef struct ipmz_qp ipmz_qp;

/* ---- context ---------------------------------------------------------- */
int ipmz_ctx_create(ipmz_ctx** out, int device);
/* Destroying a context that solvers (ipmz_qp_create / ipmz_batch_create)
 * still use only marks it: it is freed when the last of them is destroyed
 * (so a garbage collector may finalize the two in either order; the calls
 * are thread-safe with respect to each other).  A marked context first
 * drains an external stream set with ipmz_ctx_set_stream and then runs its
 * remaining solvers on its own stream; creating a solver on it returns
 * IPMZ_ERR_STATE. */
int ipmz_ctx_destroy(ipmz_ctx* ctx);
/* Enqueue on an external HIP stream, e.g. torch.cuda.current_stream().cuda_stream.
 * NULL selects the HIP null (legacy default) stream -- what PyTorch's
 * default stream is -- NOT the context's own stream. */
int ipmz_ctx_set_stream(ipmz_ctx* ctx, void* hip_stream);
/* Go back to the context's own (non-blocking) stream. */
int ipmz_ctx_reset_stream(ipmz_ctx* ctx);
int ipmz_ctx_sync(ipmz_ctx* ctx);
const char* ipmz_last_error(void);
/* Test hook: while bit 1 (solve) / bit 2 (outer-panel factor) is set, the
 * persistent kernels launched drop their first cross-workgroup hand-off, so
 * their consumers hit the 0.5 s spin limit -- the path by which a stuck
 * hand-off surfaces as IPMZ_ERR_HIP from ipmz_ldlt_factor, ipmz_ctx_sync,
 * ipmz_qp_scalars, ipmz_qp_solve (sticky error words, cleared when a
 * factorization starts).  Bit 4 is not a fault: IPMZ_STEP_GRAPH then
 * captures steps whose factor forks onto the look-ahead streams as well.
 * 0 (default) for normal operation. */
int ipmz_debug_inject(int mask);
/* Blocking of the factorization: outer panel nbo (multiple of nbi, <= 512;
 * 0 = by matrix order: with nbi 64, 512 for N > 4096, 384 for 2048 <= N <= 4096,
 * else 256), inner
 * diagonal block nbi (64 or 128).  Defaults 0 / 64.  Workspace sizes depend
 * on it: query them after setting the blocking. */
int ipmz_ctx_set_blocking(ipmz_ctx* ctx, int nbo, int nbi);
/* The blocking an order-N factor uses with this context (nbo resolved when
 * the context's is 0 = by matrix order). */
int ipmz_ctx_get_blocking(ipmz_ctx* ctx, int N, int* nbo, int* nbi);

/* ---- LinearSolvers on device memory ------------------------------------ */
/* Workspace for factor + solve of order N (bytes). */
int64_t ipmz_ldlt_workspace_bytes(ipmz_ctx* ctx, int N);
/* In-place LDL^T of the lower triangle of K (device, row-major, ld >= N,
 * ld even).  D: device, N doubles.  ws: device workspace; it keeps the
 * inverted diagonal blocks that ipmz_ldlt_solve consumes. */
int ipmz_ldlt_factor(ipmz_ctx* ctx, int N, double* K, int64_t ld, double* D, void* ws, int64_t ws_bytes);
/* b <- K^{-1} b with the factor left by ipmz_ldlt_factor (device b); asynchronous.
 * ws must stay allocated until the next ipmz_ctx_sync, which reports a
 * hand-off timeout of this solve (its sticky error words) as IPMZ_ERR_HIP. */
int ipmz_ldlt_solve(ipmz_ctx* ctx, int N, const double* K, int64_t ld, const double* D, const void* ws, double* b);
/* Rebuild the solve workspace from an explicit unit-lower L (device). */
int ipmz_ldlt_prepare_solve(ipmz_ctx* ctx, int N, const double* L, int64_t ld, void* ws, int64_t ws_bytes);
/* B (device): nrhs rows of length N, row r = right-hand side r, stride ldb >= N (even).
 * Every row <- K^{-1} row with the factor left by ipmz_ldlt_factor /
 * ipmz_ldlt_prepare_solve; asynchronous, in place, no allocation.  K's ld must
 * be even too, K (N rows of ld elements) and B 16-byte aligned; B[r][N .. ldb)
 * is never written.
 * nrhs == 1 is ipmz_ldlt_solve (bitwise); from a crossover nrhs on the rows
 * are solved together, blocked over column panels of IPMZ_SOLVE_MULTI_PANEL
 * columns on fp64 MFMA (L read once per sweep; stream-ordered launches, no
 * cross-workgroup waiting, deterministic), below it one after the other.
 * ws as for ipmz_ldlt_solve.  The multi-right-hand-side form of
 * ipmz_mixed_solve is ipmz_mixed_solve_multi, those of ipmz_normal_solve and
 * ipmz_bk_solve are ipmz_normal_solve_multi and ipmz_bk_solve_multi (all below). */
#define IPMZ_SOLVE_MULTI_PANEL 256
int ipmz_ldlt_solve_multi(ipmz_ctx* ctx, int N, const double* K, int64_t ld, const double* D, const void* ws,
                          double* B, int64_t ldb, int nrhs);

/* ---- mixed precision (config C5): fp32 factor + fp64 refinement -----------
 * No reference counterpart (the reference is fp64 throughout,
 * LinearSolvers.cpp:14-74); the result is the fp64 solution of the same
 * system to the requested tolerance.  K: device, lower triangle, row-major,
 * fp64 (left intact: the refinement residual r = b - K x uses it).  The
 * factor is of S K S, S = diag(|K_ii|^-1/2), stored in fp32 in ws. */
int64_t ipmz_mixed_workspace_bytes(ipmz_ctx* ctx, int N);
int ipmz_mixed_factor(ipmz_ctx* ctx, int N, const double* K, int64_t ld, void* ws, int64_t ws_bytes);
/* b (device) <- K^{-1} b, refined until ||b - K x||_inf <= tol ||b||_inf or
 * max_refine corrections; stat (host, may be NULL): {ratio reached,
 * corrections applied}. */
int ipmz_mixed_solve(ipmz_ctx* ctx, int N, const double* K, int64_t ld, void* ws, double* b, double tol,
                     int max_refine, double* stat);
/* The same solve for nrhs right-hand sides, the rows of B (device, stride ldb
 * >= N, even; K's ld even too, K and B 16-byte aligned; B[r][N .. ldb) is
 * never written, K is left intact).  Per pass: one blocked fp32 solve of all
 * rows (fp32 MFMA, column panels as ipmz_ldlt_solve_multi), x += correction,
 * the fp64 residual of all rows (ipmz_sym_residual_multi's kernel) and the
 * stop test of ipmz_mixed_solve PER ROW.  A row that met tol is frozen: its
 * solution and its stat {ratio reached, corrections applied} are those of the
 * pass where it stopped, so a row's result does not depend on which other rows
 * are in the call.  Passes run until every row stopped or max_refine
 * corrections are applied.  Deterministic (stream-ordered launches, no
 * atomics).  The host reads the stop word after every pass: the call BLOCKS,
 * and returns IPMZ_ERR_STATE while the context's stream is capturing a
 * hipGraph.  nrhs == 1 is ipmz_mixed_solve (bitwise, stat included; mws
 * unused); below a crossover nrhs the rows go through it one by one.
 * ws: the workspace ipmz_mixed_factor filled; mws: extra device workspace of
 * ipmz_mixed_multi_workspace_bytes(N, nrhs) bytes (x, the fp32 right-hand
 * sides, per-row state), required for nrhs >= 2: too small is
 * IPMZ_ERR_INVALID.  stat (host, may be NULL): nrhs x 2 doubles. */
int64_t ipmz_mixed_multi_workspace_bytes(ipmz_ctx* ctx, int N, int nrhs);
int ipmz_mixed_solve_multi(ipmz_ctx* ctx, int N, const double* K, int64_t ld, void* ws, double* B, int64_t ldb,
                           int nrhs, double tol, int max_refine, void* mws, int64_t mws_bytes, double* stat);
/* R = B - X K for nrhs rows (device, asynchronous), K symmetric with only its
 * lower triangle read, on fp64 MFMA; every element is summed in a fixed order
 * (deterministic).  ld, ldx, ldb, ldr >= N and even, all four matrices 16-byte
 * aligned; R may alias B. */
int ipmz_sym_residual_multi(ipmz_ctx* ctx, int N, const double* K, int64_t ld, const double* X, int64_t ldx,
                            const double* B, int64_t ldb, double* R, int64_t ldr, int nrhs);

/* ---- normal-equations reduction (config C2) ------------------------------
 * The reference derives it symbolically (get_normal_equations,
 * SymbolicOptimization.cpp:465-478; built at Optimizer.cpp:39-40) but never
 * evaluates it.  For the augmented K = [[H, B^T], [B, -E]] (device, lower
 * triangle, order n + mp, H SPD, E > 0 diagonal): Cholesky of H (as L D L^T,
 * D > 0), L21 = B L^{-T} D^{-1}, S = E + L21 D L21^T = E + B H^{-1} B^T,
 * Cholesky of S -- run as the x-first blocked LDL^T of K, one pipelined
 * factor (normal.hip).  K's lower triangle is overwritten by [L_H; L21, L_S].
 * D: device, n + mp doubles (pivots of H, then of -S).  Returns > 0 (1-based
 * augmented index) when H or S is not positive definite. */
int64_t ipmz_normal_workspace_bytes(ipmz_ctx* ctx, int n, int mp);
int ipmz_normal_factor(ipmz_ctx* ctx, int n, int mp, double* K, int64_t ld, double* D, void* ws, int64_t ws_bytes);
/* b = [r0; r1] (device) <- [x; l]:  l = S^{-1} (B H^{-1} r0 - r1),
 * x = H^{-1} (r0 - B^T l). */
int ipmz_normal_solve(ipmz_ctx* ctx, int n, int mp, const double* K, int64_t ld, const double* D, void* ws, double* b);
/* every row of B (device, nrhs rows, stride ldb >= n + mp) <- the
 * ipmz_normal_solve of that row: ipmz_ldlt_solve_multi on the factor
 * ipmz_normal_factor left (same crossover, kernels and alignment rules: ld and
 * ldb even, K and B 16-byte aligned; nrhs == 1 is ipmz_normal_solve, bitwise). */
int ipmz_normal_solve_multi(ipmz_ctx* ctx, int n, int mp, const double* K, int64_t ld, const double* D, void* ws,
                            double* B, int64_t ldb, int nrhs);

/* ---- Bunch-Kaufman (symmetric indefinite) ---------
 * LinearSolvers::symmetric_indefinite_factorization (LinearSolvers.h:23-26,
 * LinearSolvers.cpp:76-207) and overwriting_solve_bunch_kaufman
 * (LinearSolvers.h:28-31, :209-318); never called by the reference's
 * Optimizer (solve_indefinite_ is ASSERT(false), Optimizer.cpp:75).
 * Device: A row-major (lower triangle factored in place), any N; ipiv:
 * device int[N] in the reference's convention (>= 0: 1x1 pivot with that
 * interchange; < 0: -kp on both rows of a 2x2 pivot).  fix_kp = 0 keeps the
 * reference's kp = 0 for a second all-zero column (LinearSolvers.cpp:111-116),
 * 1 records kp = k.  Returns 0, or 1 + the first all-zero column. */
int ipmz_bk_factor(ipmz_ctx* ctx, int N, double* A, int64_t ld, int* ipiv, int fix_kp);
/* Same, with the kernel chosen: IPMZ_BK_AUTO (the whole-device factor from
 * N = 512 up), IPMZ_BK_WORKGROUP (one workgroup, N <= 4096), IPMZ_BK_GRID
 * (every CU, a grid barrier per pivot step).  Both are bitwise the reference. */
#define IPMZ_BK_AUTO 0
#define IPMZ_BK_WORKGROUP 1
#define IPMZ_BK_GRID 2
int ipmz_bk_factor_ex(ipmz_ctx* ctx, int N, double* A, int64_t ld, int* ipiv, int fix_kp, int algo);
/* b <- A^{-1} b from ipmz_bk_factor's F and ipiv, in the reference's order
 * (overwriting_solve_bunch_kaufman, LinearSolvers.cpp:209-318).  From
 * N = 512 it reads a transposed copy of F made on the context's stream
 * (N * N doubles, stream-ordered allocation freed after the solve). */
int ipmz_bk_solve(ipmz_ctx* ctx, int N, const double* F, int64_t ld, const int* ipiv, double* b);
/* The same solve prepared once per factor and applied to a block of
 * right-hand sides (no reference counterpart).  A^{-1} = P^T L'^{-T} D^{-1}
 * L'^{-1} P with L' unit lower (every later interchange folded into L's
 * columns), D block diagonal and P one permutation.
 * workspace of a prepared Bunch-Kaufman solve of order N (bytes) */
int64_t ipmz_bk_solve_workspace_bytes(ipmz_ctx* ctx, int N);
/* once per factor: from ipmz_bk_factor's F and ipiv (device; F is only read) build in ws the
 * transposed factor, L' (leading dimension round_up(N, 64)), the inverted 64-column diagonal
 * blocks, the persistent solve's operators and the interchange bookkeeping.  Asynchronous. */
int ipmz_bk_prepare_solve(ipmz_ctx* ctx, int N, const double* F, int64_t ld, const int* ipiv,
                          void* ws, int64_t ws_bytes);
/* every row of B (device, nrhs rows, stride ldb >= N, even, 16-byte aligned) <- A^{-1} row;
 * in place, asynchronous, no allocation; B[r][N .. ldb) is never written.  F, ld, ipiv as given
 * to ipmz_bk_prepare_solve and unchanged since.  Below a crossover nrhs the rows go one by one
 * through the launches of ipmz_bk_solve (every such row, nrhs == 1 included, is bitwise the
 * ipmz_bk_solve of that row); from it on together: row permutation, blocked forward sweep on
 * L' (fp64 MFMA, column panels as ipmz_ldlt_solve_multi), the D solve in the reference's
 * arithmetic, blocked backward sweep, inverse permutation -- stream-ordered launches, no
 * cross-workgroup waiting, deterministic, a row's result independent of its neighbours.  A
 * factor the reference solves in its own interleaved order only (a singular one with its
 * kp = 0 defect, or N > 16384) runs those sweeps instead, one workgroup per row, chosen on
 * the device.  ws must stay allocated until the next ipmz_ctx_sync, which reports a hand-off
 * timeout of the looped solves as IPMZ_ERR_HIP. */
int ipmz_bk_solve_multi(ipmz_ctx* ctx, int N, const double* F, int64_t ld, const int* ipiv,
                        const void* ws, double* B, int64_t ldb, int nrhs);
/* ---- batches of Bunch-Kaufman systems of one order (no reference counterpart) ----
 * `batch` matrices of order N (<= IPMZ_BK_NMAX = 4096), matrix q at A + q*sA (device, row-major,
 * ld >= N, sA >= (N-1)*ld + N), its pivots at ipiv + q*sP (sP >= N): the step's batched
 * one-workgroup factor on caller storage, one launch.  Every matrix is bitwise
 * ipmz_bk_factor_ex(..., IPMZ_BK_WORKGROUP) of that matrix.  info (host, batch ints, may be
 * NULL): per matrix ipmz_bk_factor's word, 0 or 1 + the first all-zero column the
 * factorization met.  Returns the smallest non-zero info, else IPMZ_OK; synchronizes.  batch <= 65535; N == 0 and batch == 0 are no-ops. */
#define IPMZ_BK_NMAX 4096
int ipmz_bk_factor_batch(ipmz_ctx* ctx, int N, int batch, double* A, int64_t ld, int64_t sA,
                         int* ipiv, int64_t sP, int fix_kp, int* info);
/* workspace of the prepared solves of a batch (bytes): per system the transposed factor and L'
 * (about 16 N^2 bytes together), the inverted 64-column diagonal blocks and the interchange
 * bookkeeping with the system's own fallback flag */
int64_t ipmz_bk_batch_solve_workspace_bytes(ipmz_ctx* ctx, int N, int batch);
/* ipmz_bk_prepare_solve for every matrix of the batch, in a number of launches that does not
 * grow with `batch` (six); sA even.  The interchange bookkeeping always uses 64-column diagonal blocks,
 * whatever ipmz_ctx_set_blocking says.  A workspace that is too small is IPMZ_ERR_INVALID.
 * Asynchronous. */
int ipmz_bk_prepare_solve_batch(ipmz_ctx* ctx, int N, int batch, const double* F, int64_t ld, int64_t sA,
                                const int* ipiv, int64_t sP, void* ws, int64_t ws_bytes);
/* rows r < nrhs at B + q*sB + r*ldb <- A_q^{-1} row; in place, asynchronous, no allocation.
 * ldb >= N and even, sB >= nrhs*ldb and even, sA even, B 16-byte aligned, nrhs >= 0; B[q][r][N .. ldb)
 * and everything between nrhs*ldb and sB is never written; N, batch or nrhs == 0 is a no-op.
 * Below a crossover nrhs the rows go one by one through the step's batched single-vector solve
 * (one launch per row serving all systems: k rows are bitwise k calls with one row, and for
 * N < 512 bitwise ipmz_bk_solve of that system); from it on together, as ipmz_bk_solve_multi
 * with the system on a grid dimension of every launch: row permutation, blocked forward sweep
 * on L', the D solve in the reference's arithmetic, blocked backward sweep, inverse
 * permutation.  A system the reference solves in its own interleaved order only (a singular
 * one) runs those sweeps instead, one workgroup per (system, row), chosen on the device per
 * system: the other systems of the batch stay on the blocked path.  Stream-ordered launches
 * only, no cross-workgroup waiting, no atomics: a row's result does not depend on the other
 * rows, a system's not on the other systems of the batch (given the same path), and equal
 * inputs give equal bits. */
int ipmz_bk_solve_multi_batch(ipmz_ctx* ctx, int N, int batch, const double* F, int64_t ld, int64_t sA,
                              const int* ipiv, int64_t sP, const void* ws,
                              double* B, int64_t ldb, int64_t sB, int nrhs);

/* Host signatures of the reference (value semantics, reference pivoting
 * including its kp = 0 defect): F = A with the lower triangle factored. */
int ipmz_symmetric_indefinite_factorization(ipmz_ctx* ctx, int N, const double* A, double* F, int* ipiv);
int ipmz_overwriting_solve_bunch_kaufman(ipmz_ctx* ctx, int N, const double* F, const int* ipiv, double* b);
/* The same for nrhs right-hand sides (ipmz_bk_prepare_solve + ipmz_bk_solve_multi):
 * B host, nrhs x N row-major, every row overwritten with its solution. */
int ipmz_overwriting_solve_bunch_kaufman_multi(ipmz_ctx* ctx, int N, const double* F, const int* ipiv,
                                               double* B, int nrhs);

/* ---- LinearSolvers with the reference's host signatures ------------------ */
/* A: host N x N row-major (lower triangle read).  L: host N x N, written
 * full (zeros above, ones on the diagonal); D: host N. */
int ipmz_ldlt_decomposition(ipmz_ctx* ctx, int N, const double* A, double* L, double* D);
/* L: host N x N unit lower; D: host N; b: host N, overwritten with the
 * solution.  N == 0 is a no-op (LinearSolvers.cpp:46-48). */
int ipmz_overwriting_solve_ldlt(ipmz_ctx* ctx, int N, const double* L, const double* D, double* b);
/* The same for nrhs right-hand sides: B host, nrhs x N row-major, every row
 * overwritten with its solution.  N == 0 or nrhs == 0 is a no-op. */
int ipmz_overwriting_solve_ldlt_multi(ipmz_ctx* ctx, int N, const double* L, const double* D, double* B, int nrhs);

/* ---- the Newton-step solver --------------------------------------------- */
/* Settings::EqualityHandling (SymbolicOptimization.h:28-64) */
#define IPMZ_EQ_REGULARIZATION 0 /* (lambda_C, lambda_C) block -delta^2, slack p: LDL^T   */
#define IPMZ_EQ_NONE 1           /* zero (lambda_C, lambda_C) block, no p: the reference's
                                    "indefinite" case (Optimizer.cpp:63-75), factored with
                                    Bunch-Kaufman (LinearSolvers.cpp:76-318): any N for a
                                    single QP (the whole-device factor from N = 512), N <= 4096
                                    per QP in batches (one workgroup per QP) */
#define IPMZ_EQ_PENALTY 2        /* PenaltyFunction: -mu (lambda_C, lambda_C) block (mu I,
                                    mu = the iterate's environment mu), no p: LDL^T */
#define IPMZ_EQ_PENALTY_EXTRA_DUAL 3 /* PenaltyFunctionWithExtraDual: the reference derives
                                        PenaltyFunction's optimality conditions through it
                                        (SymbolicOptimization.cpp:364-366) -- the same Newton
                                        system (tests/golden/formulations.txt), solved alike */
#define IPMZ_EQ_SLACKED_SLACKS 4 /* equality SlackedSlacks: t with slacks v = t - d, w = d - t
                                    (l = u = d), their duals lambda_v, lambda_w; the KKT
                                    (lambda_C, lambda_C) block -((V^-1 L_v) + (W^-1 L_w))^-1.
                                    With InequalityHandling::SlackedSlacks and both
                                    inequality bounds; the reference's evaluator asserts
                                    on its zero blocks (Evaluation.cpp:57-60) */
#define IPMZ_EQ_NAIVE_SLACKS 5   /* equality NaiveSlacks: C x - v = d, C x + w = d with duals
                                    lambda_v, lambda_w as KKT rows (SymbolicOptimization.cpp:
                                    163-171; N = n + 2m + 2p).  With InequalityHandling::
                                    NaiveSlacks and both inequality bounds: the rows run as
                                    NaiveSlacks inequality rows with l = u = d */
/* Settings::InequalityHandling (SymbolicOptimization.h:28-64) */
#define IPMZ_INEQ_SLACKED_SLACKS 0 /* s with slacks g = s - l_A, h = u_A - s (and y, z
                                      for x): the reference default                  */
#define IPMZ_INEQ_SLACKS 1         /* no g/h/y/z: complementarity on (s - l_A) lambda_g
                                      etc.; the reference's corrector substitutes
                                      dX_aff for X in (X - L_x),
                                      reproduced.  Bounds must be IPMZ_BOUNDS_BOTH
                                      (inequality bounds: when m > 0). */
#define IPMZ_INEQ_NAIVE_SLACKS 2   /* no s: l_A + g = A x, A x + h = u_A with duals lambda_g,
                                      lambda_h as KKT rows (N = n + 2m + p); the reference's
                                      evaluator asserts on its zero block, Evaluation.cpp:
                                      57-60.  Both inequality bounds; not with the
                                      normal-equations reduction. */
/* Settings::Bounds for inequality_bounds / variable_bounds */
#define IPMZ_BOUNDS_BOTH 0
#define IPMZ_BOUNDS_LOWER 1
#define IPMZ_BOUNDS_UPPER 2
#define IPMZ_BOUNDS_NONE 3 /* variable bounds only; inequalities need a bound when m > 0 */
typedef struct ipmz_qp_config {
  int n;         /* primal dimension                                  */
  int m;         /* inequality rows  l_A <= A x <= u_A                 */
  int p;         /* equality rows C x = d                              */
  double delta;  /* regularization (EnvironmentBuilder.cpp:48: 1e-4)  */
  int equality_handling;   /* IPMZ_EQ_* (0 = Regularization)          */
  int inequality_handling; /* IPMZ_INEQ_* (0 = SlackedSlacks)         */
  int inequality_bounds;   /* IPMZ_BOUNDS_* (0 = Both)                */
  int variable_bounds;     /* IPMZ_BOUNDS_* (0 = Both)                */
} ipmz_qp_config;

int ipmz_qp_create(ipmz_ctx* ctx, const ipmz_qp_config* cfg, ipmz_qp** out);
int ipmz_qp_destroy(ipmz_qp* qp);
/* build_environment: validates l_x < u_x and l_A <= u_A (throws in the
 * reference, IPMZ_ERR_INVALID here), copies the data, sets the initial
 * iterate and evaluates it.  Host pointers; unused blocks may be NULL. */
int ipmz_qp_load_host(ipmz_qp* qp, const double* Q, const double* c, const double* A, const double* l_A,
                      const double* u_A, const double* C, const double* d, const double* l_x, const double* u_x);
/* The synthetic QP of SURVEY.md §8d generated in place on the device. */
int ipmz_qp_generate(ipmz_qp* qp, uint64_t seed);
/* Enqueue one Newton step (asynchronous).  A step whose factor forks onto the
 * look-ahead streams (>= 3 outer panels) is kept to one in flight: on the
 * context's own stream the next call waits for it; on a stream set with
 * ipmz_ctx_set_stream it runs on the context's own stream and the call
 * returns once it completed, the caller's stream joined to it (a join left
 * pending on the caller's stream slows the step).  A step
 * through the mixed-precision solve (ipmz_qp_set_mixed_precision) also
 * blocks the host while its refinement runs: the eager loop reads a
 * host-mapped stop test after each pass instead of enqueuing all
 * max_refine + 1 passes.  When the caller's stream is capturing a hipGraph
 * the step is enqueued into that capture on that stream (no host wait, all
 * refinement passes, IPMZ_STEP_GRAPH ignored).  flags: */
#define IPMZ_STEP_RESTART_IF_CONVERGED 1 /* reset a converged iterate to the initial one first */
#define IPMZ_STEP_GRAPH 2                /* capture once into a hipGraph, then replay (steps whose
                                            factor forks onto the look-ahead streams -- >= 3 outer
                                            panels -- are enqueued eagerly instead) */
/* IPMZ_STEP_SKIP_CONVERGED: a QP of a batch whose IPMZ_SC_CONVERGED is non-zero
 * when the step starts takes no part in it.  Its iterate, residuals, both
 * direction blocks (IPMZ_STATE_DAFF, IPMZ_STATE_DIR), its right-hand-side slot
 * and its whole scalar block keep their bits -- those of the step that
 * converged it; its factor is the one of that step's matrix.  Every other QP
 * gets bitwise the step it gets without the flag: the kernels, chosen by N,
 * the inner block and the batch size, are the same; a skipped QP's workgroups
 * return at the top of every launch, on the device, and the CUs they would
 * have held go to the QPs still working.  The batched factor's info word is
 * then the minimum over the QPs that were factored.  The step adds 1.0 to
 * IPMZ_SC_STEPS of every QP it does not skip; no other step touches that slot,
 * which restarts at 0 with the scalar block (a load, ipmz_batch_initialize,
 * ipmz_qp_generate; not ipmz_batch_set_state*): after a solve it is the QP's
 * own iteration count.
 *   Served: batches (batch > 1) of small systems, N <= 1024, with inner block
 *     64 -- every LDL^T formulation, whatever ipmz_batch_set_factor_kernel
 *     selects, and IPMZ_EQ_NONE batches; with IPMZ_STEP_GRAPH, and enqueued
 *     into a caller's capture, like any other flag set.
 *   Refused with IPMZ_ERR_INVALID before anything is enqueued (and before the
 *     check for a load): a solver of one QP (ipmz_qp_solve stops at
 *     convergence already), N > 1024 and inner block 128 (their factor is not
 *     per QP), and the flag together with IPMZ_STEP_RESTART_IF_CONVERGED.
 *     ipmz_batch_can_skip_converged answers for the solver as configured.
 *   Never skipping: the calls that reuse the step's assembly and factor --
 *     ipmz_*_kkt_solve*, ipmz_*_newton_solve_multi, ipmz_*_newton_adjoint_multi
 *     -- factor every QP, converged or not (the backward pass needs exactly
 *     the factor of converged QPs). */
#define IPMZ_STEP_SKIP_CONVERGED 4
int ipmz_qp_step(ipmz_qp* qp, int flags);
/* 1 when the last ipmz_qp_step replayed a captured hipGraph, 0 when its
 * launches were enqueued one by one (what a benchmark reports it timed). */
int ipmz_qp_last_step_graph(ipmz_qp* qp);
/* Synchronize and copy the IPMZ_SC_COUNT scalars to host memory. */
int ipmz_qp_scalars(ipmz_qp* qp, double* out);
/* Device pointer of the scalar block (for collectives). */
int ipmz_qp_device_scalars(ipmz_qp* qp, double** out);
/* Enqueue a device-to-device copy of the scalar block to dst (device). */
int ipmz_qp_copy_scalars(ipmz_qp* qp, double* dst_device);
/* Optimizer::solve: iterate until res < 1e-8 and mu < 1e-8 or max_iter.
 * trace (host, may be NULL): max_iter rows of 8 doubles
 * {f, res, mu, alpha_aff, mu_aff, sigma, alpha, converged}. */
int ipmz_qp_solve(ipmz_qp* qp, int max_iter, double* trace, int* iterations);
/* Concatenated state in Newton order.  which: 0 iterate, 1 affine
 * direction, 2 corrector direction, 3 residual vectors r_v. */
#define IPMZ_STATE_VARS 0
#define IPMZ_STATE_DAFF 1
#define IPMZ_STATE_DIR 2
#define IPMZ_STATE_RES 3
int64_t ipmz_qp_state_len(ipmz_qp* qp);
int ipmz_qp_get_state(ipmz_qp* qp, int which, double* host_out);
/* Overwrite the iterate (host, Newton order) and re-evaluate it. */
int ipmz_qp_set_state(ipmz_qp* qp, const double* host_vars);
/* Assemble the KKT matrix of the current iterate; host N x N row-major
 * (lower triangle written, upper zero).  For parity tests. */
int ipmz_qp_get_kkt(ipmz_qp* qp, double* host_K);
int ipmz_qp_kkt_dim(ipmz_qp* qp);
/* What the last step's factor left on the QP's storage, for parity tests
 * (single QPs on the fp64 augmented LDL^T with nbi = 64, else IPMZ_ERR_STATE):
 * host_L, N x N row-major (lower triangle as stored, upper zero); host_D, N;
 * host_P, the persistent solve's prepared operators, *p_len doubles (the two
 * blocks no solve reads are zero).  Each pointer may be null; synchronizes. */
int ipmz_qp_get_factor(ipmz_qp* qp, double* host_L, double* host_D, double* host_P, int64_t* p_len);
/* Solve with the KKT matrix of the QP's current iterate: assembles it (the
 * matrix ipmz_qp_get_kkt returns, order ipmz_qp_kkt_dim), factors it and
 * solves the nrhs rows of B (device, Newton order, stride ldb >= N, even) as
 * ipmz_ldlt_solve_multi does.  Returns the factor's info like
 * ipmz_ldlt_factor (synchronizes).  Leaves the iterate and all later steps
 * unchanged.  For single QPs whose step factors the augmented system with
 * fp64 LDL^T: IPMZ_ERR_INVALID for batches (their call is
 * ipmz_batch_kkt_solve), IPMZ_EQ_NONE (Bunch-Kaufman), an
 * enabled normal-equations reduction or mixed-precision mode.  The Newton
 * step itself is untouched: its two solves depend on each other and stay
 * single-vector.  The mixed-precision form is ipmz_qp_kkt_solve_mixed. */
int ipmz_qp_kkt_solve(ipmz_qp* qp, int nrhs, double* B, int64_t ldb);
/* ipmz_qp_kkt_solve for single QPs with IPMZ_EQ_NONE: the step's own assembly
 * and Bunch-Kaufman factor on the QP's storage, then ipmz_bk_solve_multi (B
 * 16-byte aligned, ldb >= N and even).  Returns the factor's info like
 * ipmz_bk_factor (synchronizes); the iterate and all later steps are unchanged
 * (bitwise).  IPMZ_ERR_INVALID for batches, any other equality handling, an
 * enabled normal-equations reduction or mixed precision; IPMZ_ERR_STATE
 * before a load. */
int ipmz_qp_kkt_solve_bk(ipmz_qp* qp, int nrhs, double* B, int64_t ldb);
/* ipmz_qp_kkt_solve through the fp32 factor + fp64 refinement
 * (ipmz_mixed_factor + ipmz_mixed_solve_multi on the assembled KKT matrix),
 * whether or not the QP's steps use mixed precision.  B 16-byte aligned; tol,
 * max_refine, stat (host, nrhs x 2, may be NULL) as ipmz_mixed_solve_multi.
 * Under the restrictions of ipmz_qp_set_mixed_precision: IPMZ_ERR_INVALID for
 * batches, IPMZ_EQ_NONE, penalty-function equalities or an enabled
 * normal-equations reduction.  Allocates the QP's mixed-precision workspace on
 * first use (the one ipmz_qp_set_mixed_precision uses, never reallocated) and
 * a multi workspace for the largest nrhs seen.  Returns the fp32 factor's
 * info; synchronizes; IPMZ_ERR_STATE during a graph capture.  Leaves the
 * iterate and all later steps bitwise unchanged in both step modes. */
int ipmz_qp_kkt_solve_mixed(ipmz_qp* qp, int nrhs, double* B, int64_t ldb, double tol, int max_refine, double* stat);
/* Newton directions through the mixed-precision solve (fp32 factor of the
 * scaled KKT matrix + fp64 refinement to tol, at most max_refine corrections
 * per solve); enable = 0 returns to the fp64 factor.  Single QPs only.  The
 * scalar block then reports IPMZ_SC_IR_*. */
int ipmz_qp_set_mixed_precision(ipmz_qp* qp, int enable, double tol, int max_refine);
/* KKT reduction of the Newton step: augmented LDL^T (default, what the
 * reference solves, Optimizer.cpp:137-138) or the normal equations (the
 * reference's normal_equations_ reduction, Optimizer.cpp:39-40).  Single
 * QPs; not combined with mixed precision. */
#define IPMZ_REDUCTION_AUGMENTED 0
#define IPMZ_REDUCTION_NORMAL 1
int ipmz_qp_set_reduction(ipmz_qp* qp, int reduction);

/* ---- batches of independent QPs (config C4) ------------------------------
 * A batch is an ipmz_qp holding `batch` QPs of identical (n, m, p); every
 * kernel launch serves the whole batch.  ipmz_qp_step / _generate (QP i gets
 * seed + i) / _destroy / _set_timing / _phase_times apply to batches; the
 * ipmz_qp_* state accessors address QP 0. */
int ipmz_batch_create(ipmz_ctx* ctx, const ipmz_qp_config* cfg, int batch, ipmz_qp** out);
int ipmz_batch_size(ipmz_qp* qp);
/* Copy QP `index`'s data (build_environment's validation); call
 * ipmz_batch_initialize once every QP is loaded.  A load leaves the batch
 * uninitialized: ipmz_qp_step / ipmz_batch_solve return IPMZ_ERR_STATE until
 * ipmz_batch_initialize has rebuilt the kept KKT matrix and the residuals
 * from the new data (a step on the previous data's matrix would be silent
 * corruption). */
int ipmz_batch_load_host(ipmz_qp* qp, int index, const double* Q, const double* c, const double* A,
                         const double* l_A, const double* u_A, const double* C, const double* d, const double* l_x,
                         const double* u_x);
int ipmz_batch_initialize(ipmz_qp* qp);
/* out: host, batch * IPMZ_SC_COUNT doubles */
int ipmz_batch_scalars(ipmz_qp* qp, double* out);
int ipmz_batch_get_state(ipmz_qp* qp, int index, int which, double* host_out);
int ipmz_batch_set_state(ipmz_qp* qp, int index, const double* host_vars);
/* The whole batch loaded from device memory, and its states read back to
 * device memory: neither the data nor the answers pass through the host, and
 * no call is made per QP.
 *
 * ipmz_qp_device_data describes the data of every QP as strided blocks of
 * doubles on the context's device.  Matrices are row-major with a row stride
 * (ldq, lda, ldc >= n) and a QP stride; vectors have a QP stride; strides are
 * in elements.  QP q's block starts q * (QP stride) elements after the
 * pointer, and a QP stride of 0 is ONE block shared by every QP (parametric
 * QPs with a common Q / A / C).  A non-zero QP stride is at least the block's
 * extent ((rows - 1) * row stride + n, or the vector's length); no stride is
 * negative.  There is no alignment rule: blocks whose pointer is 16-byte
 * aligned and whose strides are even are copied with 16-byte accesses, the
 * others element by element, with equal results.  Elements outside the blocks
 * (row padding, the space between QPs) are never read.  A NULL block keeps
 * the data the solver already holds; blocks of dimension 0 (A, l_A, u_A with
 * m == 0; C, d with p == 0) are ignored whatever they hold. */
typedef struct ipmz_qp_device_data {
  const double* Q;    /* n rows of n */
  int64_t ldq, sQ;
  const double* A;    /* m rows of n */
  int64_t lda, sA;
  const double* C;    /* p rows of n */
  int64_t ldc, sC;
  const double *c, *l_x, *u_x; /* n each */
  int64_t sc, slx, sux;
  const double *l_A, *u_A;     /* m each */
  int64_t slA, suA;
  const double* d;    /* p */
  int64_t sd;
} ipmz_qp_device_data;
/* Load every QP of the solver (a solver of ipmz_qp_create is a batch of one)
 * from `data`, then do what ipmz_batch_initialize does: a fresh iterate, the
 * kept KKT matrix and the residuals rebuilt from the data the solver now
 * holds -- the supplied blocks merged with the kept ones (the parametric
 * re-load: e.g. c and d only); the scalar blocks restart too, so that the
 * solver equals a new one loaded with the merged data.  On the context's stream, in this order: the
 * bound check (one kernel), one synchronize for its verdict, the copy
 * kernels, the initialization (which synchronizes).  The caller orders
 * whatever produced the input blocks before the context's stream (the same
 * stream, an event, or a synchronize); the blocks are no longer read once the
 * call returns.
 *
 * build_environment's validation, over every QP: !(l_x[k] < u_x[k]) and
 * !(l_A[k] <= u_A[k]) are violations (a NaN therefore is one), for the bound
 * pairs of which the call supplies at least one side -- the other side is then
 * the one the solver holds.  A violation returns IPMZ_ERR_INVALID with a
 * message naming the QP, the bound and the index of the first one in the order
 * (QP, l_x before l_A, index), whatever the kernel's schedule; NOTHING is
 * written: the data, the iterate and the loaded state stay as they were and
 * the solver steps on as if the call had not been made.
 *
 * IPMZ_ERR_INVALID also for a null qp or data, a row stride < n, a negative
 * stride, a non-zero QP stride below the block's extent (batches only).
 * IPMZ_ERR_STATE for a NULL block of non-zero dimension that the solver has
 * never held for every QP (held: filled by an earlier device load, by
 * ipmz_qp_load_host, by ipmz_batch_load_host of every QP, or by
 * ipmz_qp_generate), and while the context's stream is capturing (the call
 * synchronizes).  A step graph captured earlier (IPMZ_STEP_GRAPH) stays valid:
 * it holds addresses and the kernel selection, which a load does not change. */
int ipmz_batch_load_device(ipmz_qp* qp, const ipmz_qp_device_data* data);
/* ipmz_batch_get_state of every QP at once, to device memory: row q of dst
 * (device, at dst + q * ld, ld >= ipmz_qp_state_len) receives exactly the
 * ipmz_qp_state_len doubles ipmz_batch_get_state(qp, q, which, ..) returns --
 * the reference's Newton order, for IPMZ_EQ_SLACKED_SLACKS / IPMZ_EQ_NAIVE_SLACKS
 * the same permutation of the step's merged slots, applied by the kernel.
 * dst[q][state_len .. ld) is never written.  One launch on the context's
 * stream: asynchronous, no allocation, no synchronize, so it may be enqueued
 * into a caller's graph capture.  IPMZ_ERR_INVALID for a bad `which`, a null
 * dst or ld < state_len; IPMZ_ERR_STATE before a load. */
int ipmz_batch_copy_state(ipmz_qp* qp, int which, double* dst_device, int64_t ld);
/* The warm start: ipmz_batch_set_state of the whole batch from device memory,
 * the inverse of ipmz_batch_copy_state(qp, IPMZ_STATE_VARS, ..).  Row q of src
 * (device, at src + q * ld, ld >= ipmz_qp_state_len) holds QP q's iterate in the
 * reference's Newton order; for IPMZ_EQ_SLACKED_SLACKS / IPMZ_EQ_NAIVE_SLACKS
 * the kernel scatters it through the inverse of that call's permutation.  No
 * alignment rule; src[q][state_len .. ld) is never read; a solver of one QP
 * reads row 0.
 *
 * take (device, batch ints; NULL: every QP): QP q is overwritten only if
 * take[q] != 0, and the rows of the others are never read.
 *
 * floor >= 0, the interior push: every component v of a taken row in a slot
 * the step length keeps non-negative -- lambda_y, lambda_z, lambda_g,
 * lambda_h, and y, z, g, h where they are Newton variables -- becomes
 * v < floor ? floor : v, before any check; 0 changes nothing in a row the
 * check passes (a negative component becomes 0, a violation all the same).
 * x, s and the free duals are never pushed.  (A converged iterate lies on the boundary:
 * complementary pairs have one side near 0, and a Newton step from there is
 * short.  A warm start normally wants floor > 0.)
 *
 * The check, over the pushed rows of every taken QP: a NaN anywhere, !(v > 0)
 * in one of those slots, and -- IPMZ_INEQ_SLACKS, and every formulation with
 * m == 0, where the step length holds x and s inside explicit bounds --
 * !(l_x < x < u_x), !(l_A < s < u_A) against the data the solver holds.  One
 * kernel and one synchronize for its verdict.  A violation returns
 * IPMZ_ERR_INVALID with a message naming the QP and the index within its row
 * of the first one in the order (QP, index), whatever the kernel's schedule;
 * NOTHING is written.  IPMZ_SET_STATE_UNCHECKED: no check and no synchronize
 * -- stream-ordered launches only, no allocation, so the call may be enqueued
 * into a caller's graph capture; what an iterate outside the interior does to
 * the following steps is then the caller's affair.
 *
 * Then the taken rows are scattered and every QP is evaluated, as
 * ipmz_batch_set_state does: for a taken QP the iterate, the residuals and the
 * scalar block are bitwise what ipmz_batch_set_state(qp, q, the pushed row)
 * leaves, the others keep their iterate.  The directions, the last step's
 * scalars, the kept KKT matrix, the restart snapshot, a captured step graph
 * and the blocking stay as they are.  The checked form returns with the
 * launches enqueued, not synchronized.
 *
 * IPMZ_ERR_INVALID also for a null qp or src, ld < state_len, an unknown flag
 * bit, a negative or non-finite floor, and floor > 0 with IPMZ_INEQ_SLACKS
 * (that formulation's positivity is x - l_x etc., not a slot).  IPMZ_ERR_STATE
 * before a load or between a load and ipmz_batch_initialize, and, for the
 * checked form only, while the context's stream is capturing. */
#define IPMZ_SET_STATE_UNCHECKED 1
int ipmz_batch_set_state_device(ipmz_qp* qp, const double* src, int64_t ld, const int32_t* take, double floor,
                                int flags);
/* Enqueue a device-to-device copy of all batch * IPMZ_SC_COUNT scalars
 * (QP-major) to dst (device): the input of the cross-GPU convergence summary. */
int ipmz_batch_copy_scalars(ipmz_qp* qp, double* dst_device);
/* Enqueue ONE kernel writing the batch's convergence summary to dst (device,
 * 3 doubles): {max res, max mu, unconverged count} over its QPs -- the
 * stopping rule of Optimizer.cpp:124-135 in MAX-reducible form, so a single
 * all-reduce (MAX) across the ranks of a sharded batch decides the stop
 * (reduced dst[2] == 0 <=> every QP of the job converged).  For the RCCL
 * driver loop of ipmz_amd.dist.solve_sharded. */
int ipmz_batch_summary(ipmz_qp* qp, double* dst_device);
/* Step until every QP converged (converged QPs keep their iterate). */
int ipmz_batch_solve(ipmz_qp* qp, int max_iter, int* iterations, int* converged_count);
/* 1 when ipmz_qp_step serves IPMZ_STEP_SKIP_CONVERGED for this solver under
 * the context's current blocking, else 0 (also for a null qp). */
int ipmz_batch_can_skip_converged(ipmz_qp* qp);
/* ipmz_batch_solve with the steps' flags and a host that looks at the device
 * only every check_every steps.  step_flags: 0, IPMZ_STEP_SKIP_CONVERGED,
 * IPMZ_STEP_GRAPH or both.  Between two looks the call enqueues check_every
 * steps (>= 1), never going beyond max_iter; a look is ipmz_batch_summary's
 * kernel and a copy of its 3 doubles, not of batch * IPMZ_SC_COUNT.
 * iterations (host, may be NULL): the steps enqueued, at most ipmz_batch_solve's
 * count rounded up to a multiple of check_every; with the skip flag each QP's
 * own count is its IPMZ_SC_STEPS whatever check_every was.  converged_count:
 * host, may be NULL.  check_every 1 and step_flags 0 give the iterates and
 * both counts of ipmz_batch_solve.  IPMZ_ERR_INVALID: a null qp, max_iter < 0,
 * check_every < 1, any other flag, or the skip flag where ipmz_qp_step refuses
 * it; then IPMZ_ERR_STATE before a load, between a load and
 * ipmz_batch_initialize, or while the context's stream is capturing. */
int ipmz_batch_solve_ex(ipmz_qp* qp, int max_iter, int step_flags, int check_every, int* iterations,
                        int* converged_count);
/* Which kernel factors a batch of small systems (N <= 1024, 64-column
 * blocks, one LDL^T): IPMZ_BATCH_FACTOR_AUTO (default: the wave-specialized
 * left-looking kernel for 64 < N <= 320; above that two workgroups per QP
 * when 2 * batch <= #CU, else the left-looking one), IPMZ_BATCH_FACTOR_ONE
 * (right-looking, one workgroup per QP), IPMZ_BATCH_FACTOR_PAIR (the same
 * right-looking factor on two workgroups per QP -- identical results to ONE;
 * IPMZ_ERR_INVALID unless 2 * batch <= #CU, since both workgroups of a QP
 * must be resident together), IPMZ_BATCH_FACTOR_LEFT (left-looking, one
 * workgroup per QP: every L tile formed once in registers; sums in a
 * different order, so 1e-16-level differences against ONE / PAIR). */
#define IPMZ_BATCH_FACTOR_AUTO 0
#define IPMZ_BATCH_FACTOR_ONE 1
#define IPMZ_BATCH_FACTOR_PAIR 2
#define IPMZ_BATCH_FACTOR_LEFT 3
int ipmz_batch_set_factor_kernel(ipmz_qp* qp, int kernel);
/* ipmz_qp_get_kkt for QP `index` of a batch: host N x N row-major, lower triangle
 * written, upper zero.  index out of range: IPMZ_ERR_INVALID.  (ipmz_qp_get_kkt
 * on a batch addresses QP 0.) */
int ipmz_batch_get_kkt(ipmz_qp* qp, int index, double* host_K);
/* For every QP q of the batch: assemble the KKT matrix of its current iterate
 * (the matrix ipmz_batch_get_kkt returns), factor it (the step's own batched
 * assembly and factor, on the storage the next step overwrites anyway) and
 * solve the nrhs rows at B + q * sB (device, Newton order, row stride ldb) in
 * place: row <- K_q^{-1} row.
 *
 * Arguments: ldb >= N and even; sB >= nrhs * ldb and even; B 16-byte aligned;
 * nrhs >= 0 (nrhs == 0 still assembles and factors and returns the info word).
 * Only the first N elements of each of the nrhs rows of a QP are written:
 * B[q][r][N .. ldb) and everything between nrhs * ldb and sB keep their bits.
 * A contiguous (batch, nrhs, ldb) array has sB = nrhs * ldb.
 *
 * Served: batches whose step factors the augmented system with fp64 LDL^T --
 * every equality and inequality handling except IPMZ_EQ_NONE, any N, inner
 * blocks (ipmz_ctx_set_blocking) of 64 and 128.  IPMZ_EQ_NONE batches factor
 * with Bunch-Kaufman and return IPMZ_ERR_INVALID.  A solver that holds one QP
 * (ipmz_qp_create, or ipmz_batch_create with batch 1) forwards to
 * ipmz_qp_kkt_solve; sB is then ignored.  IPMZ_ERR_STATE between a load and
 * ipmz_batch_initialize, and while the context's stream is capturing (the
 * call synchronizes).
 *
 * Returns the batched factor's info word as a step sees it: ONE word for the
 * whole batch, IPMZ_OK when every pivot of every QP was finite, otherwise the
 * smallest 1-based pivot index at which any QP met a non-finite pivot (which
 * QP is not recorded; the rows of the other QPs are still their solutions).
 * IPMZ_ERR_HIP when the two-workgroup batched factor ran and a hand-off in it
 * timed out (its sticky error word).
 *
 * The iterate, the matrix the fused steps keep across steps, a captured step
 * graph (IPMZ_STEP_GRAPH) and all later steps are unchanged, bitwise.  Only
 * stream-ordered launches, no cross-workgroup waiting and no atomics in the
 * solve: a row's result does not depend on the other rows of the call, a QP's
 * not on the other QPs of the batch (given the same kernel selection, which
 * depends on N, the inner block, nrhs and -- through the single-vector
 * kernels below the crossover -- the batch size), and equal inputs give equal
 * bits.  Few right-hand sides run through the step's single-vector batched
 * solve row by row, more through one blocked launch per batch (systems whose
 * 16 right-hand sides fit a workgroup's LDS: N <= 832 with inner block 64,
 * <= 768 with 128, on 160 KiB) or the panel chain of ipmz_ldlt_solve_multi
 * with the QP on a grid dimension. */
int ipmz_batch_kkt_solve(ipmz_qp* qp, int nrhs, double* B, int64_t ldb, int64_t sB);
/* ipmz_batch_kkt_solve for IPMZ_EQ_NONE batches (N <= 4096): the step's own assembly and
 * batched Bunch-Kaufman factor on the storage the next step overwrites anyway, then
 * ipmz_bk_prepare_solve_batch and ipmz_bk_solve_multi_batch on a workspace allocated on first
 * use and freed with the solver (IPMZ_ERR_NOMEM when it cannot be had).  Same argument rules
 * as ipmz_batch_kkt_solve.  info (host, batch ints, may be NULL): per QP ipmz_bk_factor's
 * word (0 or 1 + the first all-zero column met); returns the smallest non-zero one, else IPMZ_OK; synchronizes.  The
 * iterate, a captured step graph (IPMZ_STEP_GRAPH) and all later steps are unchanged, bitwise.
 * IPMZ_ERR_INVALID for any other equality handling; IPMZ_ERR_STATE before a load, between a
 * load and ipmz_batch_initialize, and while the stream is capturing.  A solver that holds one
 * QP forwards to ipmz_qp_kkt_solve_bk: sB is then ignored and info[0] is the return value. */
int ipmz_batch_kkt_solve_bk(ipmz_qp* qp, int nrhs, double* B, int64_t ldb, int64_t sB, int* info);

/* compute_search_direction_ (Optimizer.cpp:344-380) for a block of residual
 * vectors, plus get_max_step_ (Optimizer.cpp:270-342) of every direction: for
 * every QP q of the solver and every row r < nrhs, the full Newton direction d
 * of J d = -r at the current iterate, J the Jacobian of the formulation's
 * Newton system (tests/golden/formulations.txt, "newton system / lhs").
 *
 * Rows: with L = ipmz_qp_state_len(qp), row r of QP q of R is at R + q * sR +
 * r * ldr (device) and holds L doubles: the residual vectors r_v in Newton
 * order, the layout of ipmz_qp_get_state(.., IPMZ_STATE_RES, ..) ("shorthand
 * definitions" of formulations.txt).  Dir has the same shape (q * sD + r *
 * ldd) and receives the full direction in the layout of IPMZ_STATE_DAFF.  Per
 * row: the augmented right-hand side from the row's r_v and the iterate (the
 * step's own expressions), K^{-1} of it, then the delta_definitions in reverse
 * (the step's own back-substitution).  mu does not enter: the caller has put
 * whatever mu and corrector terms it wants into R.  The row
 * ipmz_qp_get_state(IPMZ_STATE_RES) of a fresh iterate gives the affine
 * direction the next step computes (IPMZ_STATE_DAFF after it).
 *
 * alpha (device, batch * nrhs doubles, QP-major, may be NULL): alpha[q * nrhs
 * + r] = get_max_step_ of (the iterate, row r's direction) before the 0.995
 * factor -- what a step stores in IPMZ_SC_ALPHA_AFF / IPMZ_SC_ALPHA -- by the
 * step's rules, the explicit l_x, u_x, l_A, u_A bounds of box-only and
 * IPMZ_INEQ_SLACKS forms included.
 *
 * Factor, by the solver's formulation: the fp64 augmented LDL^T for every
 * equality handling but IPMZ_EQ_NONE, Bunch-Kaufman for IPMZ_EQ_NONE (any N for
 * a single QP, N <= 4096 for batches): the step's own assembly and factor on
 * the storage the next step overwrites anyway, then the blocked solves of
 * ipmz_qp_kkt_solve / _bk and ipmz_batch_kkt_solve / _bk with their crossovers
 * and kernels.  The reduced right-hand sides live in a workspace of the solver
 * (batch * nrhs * round_up(N, 2) doubles, allocated on first use, grown for
 * the largest nrhs seen, freed with the solver; IPMZ_ERR_NOMEM when it cannot
 * be had), not in Dir: the solves see rows of stride round_up(N, 2) whatever
 * ldd is, and nothing relies on the head of a Newton-order row being the KKT
 * order.
 *
 * Arguments: nrhs >= 0 (nrhs == 0 still assembles, factors and returns the
 * info word); ldr >= L, ldd >= L, both even; sR >= nrhs * ldr, sD >= nrhs *
 * ldd, both even; R and Dir 16-byte aligned.  Dir[q][r][L .. ldd) and
 * everything between nrhs * ldd and sD keep their bits.  R is never written
 * unless it is Dir: Dir == R with ldd == ldr and sD == sR is allowed (in place
 * -- every element of a row is read and written by exactly one thread of the
 * back-substitution); any other overlap is the caller's error and is not
 * detected.
 *
 * Returns what the matching *_kkt_solve* call returns: the factor's info word,
 * after the sticky error words were checked; synchronizes once, at the end.
 * info (host, batch ints, may be NULL): per QP for IPMZ_EQ_NONE batches, as in
 * ipmz_batch_kkt_solve_bk; otherwise every entry is the return value.  A
 * solver that holds one QP forwards from the batch call to the single one (sR
 * and sD ignored).
 *
 * The iterate, the step's own right-hand side, direction and residual slots,
 * the scalar block, the matrix the fused steps keep across steps, a captured
 * step graph (IPMZ_STEP_GRAPH) and all later steps are unchanged, bitwise.
 * Stream-ordered launches only, no cross-workgroup waiting, no atomics: a
 * row's result does not depend on the other rows of the call, a QP's not on
 * the other QPs (given the same kernel selection), equal inputs give equal
 * bits.
 *
 * Accuracy: the eliminated slack / dual pairs are back-substituted slack
 * first, each from its own row of the Newton system (dg = ds - r_lg, then
 * dl_g from row g), so those rows are met to a few units of roundoff
 * componentwise for any residual row, at a late iterate too.  The step itself
 * keeps the reference's order (dual first), which is as accurate for the
 * iterate's own residual only; a row equal to that residual therefore agrees
 * with the step's direction to rounding, not bit for bit.
 *
 * IPMZ_ERR_INVALID: an enabled normal-equations reduction or mixed precision;
 * IPMZ_EQ_SLACKED_SLACKS / IPMZ_EQ_NAIVE_SLACKS (their public state is a
 * permuted, merged view of the step's slots; ipmz_batch_copy_state applies that
 * permutation on the device, this call does not yet); bad strides or alignment; IPMZ_EQ_NONE batches
 * with N > 4096.  IPMZ_ERR_STATE before a load, between a load and
 * ipmz_batch_initialize, and while the context's stream is capturing. */
int ipmz_qp_newton_solve_multi(ipmz_qp* qp, int nrhs, const double* R, int64_t ldr, double* Dir, int64_t ldd,
                               double* alpha /* device, nrhs, may be NULL */);
int ipmz_batch_newton_solve_multi(ipmz_qp* qp, int nrhs, const double* R, int64_t ldr, int64_t sR, double* Dir,
                                  int64_t ldd, int64_t sD, double* alpha /* device, batch*nrhs, QP-major, may be NULL */,
                                  int* info /* host, batch ints, may be NULL */);

/* The transpose of ipmz_*_newton_solve_multi, for a backward pass through the
 * Newton step: with Dir = M R the map of that call at the current iterate (M =
 * -J^{-1}, J the Jacobian of the formulation's Newton system, which is not
 * symmetric), for every QP q of the solver and every row r < nrhs
 *
 *     out = M^T g,   that is   J^T out = -g,
 *
 * so that <g, Dir(r)> = <out(g), r> for all g and r.  Row r of QP q of G is at
 * G + q * sG + r * ldg (device) and holds L = ipmz_qp_state_len(qp) doubles in
 * the layout of IPMZ_STATE_DAFF: the cotangent of a direction.  Out has the
 * same shape (q * sO + r * ldo) and receives the cotangent with respect to the
 * residual vectors r_v, in the layout of IPMZ_STATE_RES; both layouts are the
 * same Newton order.
 *
 * Per row the forward call is b = G_r r (the augmented right-hand side), x =
 * K^{-1} b, d = E x + F r (the delta_definitions), G_r, E and F element-local
 * maps of the iterate alone.  K is symmetric, so every blocked K^{-1} is its own
 * transpose, and out = F^T g + G_r^T K^{-1} (E^T g): E^T g of every row into
 * the workspace of ipmz_*_newton_solve_multi, the same assembly, factor and
 * blocked solves by the solver's formulation, then the expansion into every
 * slot the formulation has.  The coefficients are read off the step's own
 * expressions, not restated.  There is no step length.
 *
 * Arguments, as for the forward pair: nrhs >= 0 (nrhs == 0 still assembles,
 * factors and returns the info word); ldg >= L, ldo >= L, both even; sG >= nrhs
 * * ldg, sO >= nrhs * ldo, both even; G and Out 16-byte aligned.  All L
 * elements of every Out row are written; Out[q][r][L .. ldo) and everything
 * between nrhs * ldo and sO keep their bits.  G is never written unless it is
 * Out: Out == G with ldo == ldg and sO == sG is allowed (in place -- a thread
 * reads every g element it owns before it writes any out element it owns, and
 * no element has two owners); any other overlap is the caller's error and is
 * not detected.
 *
 * Returns, synchronizes and fills info (host, batch ints, may be NULL) like the
 * forward pair; a solver that holds one QP forwards from the batch call to the
 * single one (sG and sO ignored).  The iterate, the step's own slots, the
 * scalar block, the matrix the fused steps keep across steps, a captured step
 * graph and all later steps are unchanged, bitwise.  Stream-ordered launches
 * only, no cross-workgroup waiting, no atomics: a row's result does not depend
 * on the other rows, a QP's not on the other QPs, equal inputs give equal bits.
 *
 * Served and refused exactly like the forward pair: IPMZ_ERR_INVALID for an
 * enabled normal-equations reduction or mixed precision, IPMZ_EQ_SLACKED_SLACKS
 * / IPMZ_EQ_NAIVE_SLACKS, bad strides or alignment, IPMZ_EQ_NONE batches with
 * N > 4096; IPMZ_ERR_STATE before a load, between a load and
 * ipmz_batch_initialize, and while the context's stream is capturing. */
int ipmz_qp_newton_adjoint_multi(ipmz_qp* qp, int nrhs, const double* G, int64_t ldg, double* Out, int64_t ldo);
int ipmz_batch_newton_adjoint_multi(ipmz_qp* qp, int nrhs, const double* G, int64_t ldg, int64_t sG, double* Out,
                                    int64_t ldo, int64_t sO, int* info /* host, batch ints, may be NULL */);

/* The last link of a backward pass through a solved QP: the cotangent with
 * respect to the residual vectors r_v (what the adjoint pair above returns)
 * contracted with d r_v / d (Q, c, A, l_A, u_A, C, d, l_x, u_x) at the current
 * iterate -- the gradient of a loss with respect to the problem data.  At a
 * fixed iterate and a fixed mu every r_v is affine in the data ("shorthand
 * definitions" of tests/golden/formulations.txt), so with w the cotangent row
 * of a QP (J^T w = -g, the adjoint's own sign: dz = -J^{-1} r_theta dtheta)
 *
 *     dL/dtheta = (d r / d theta)^T w.
 *
 * In the default form: gc = w_x; gQ[i][j] = w_x[i] x[j]; gA[i][j] =
 * w_lambda_A[i] x[j] + lambda_A[i] w_x[j]; gC the same with lambda_C; gd =
 * -w_lambda_C; g l_x = w_lambda_y, g u_x = -w_lambda_z, g l_A = w_lambda_g,
 * g u_A = -w_lambda_h.  IPMZ_INEQ_SLACKS: the bounds enter the complementarity
 * rows multiplied by the duals (g l_x = -lambda_y w_lambda_y, g u_x = lambda_z
 * w_lambda_z, and so for l_A, u_A).  IPMZ_INEQ_NAIVE_SLACKS: A x sits in
 * r_lambda_g and r_lambda_h and A^T multiplies (lambda_h - lambda_g).  A bound
 * the formulation does not have gets a zero gradient.  Conventions: mu is a
 * constant of the call (the data's effect on IPMZ_SC_MU is not differentiated;
 * it matters only for penalty equalities with IPMZ_INEQ_SLACKS); the n^2
 * entries of Q are independent, gQ = w_x x^T is NOT symmetrised (a caller who
 * keeps Q symmetric takes (gQ + gQ^T) / 2); IPMZ_EQ_REGULARIZATION's delta is
 * not data.
 *
 * W (device): one row per QP at W + q * sW, ipmz_qp_state_len doubles in the
 * layout of IPMZ_STATE_RES -- row 0 of Out of ipmz_batch_newton_adjoint_multi
 * with sW = sO.  A solver of one QP ignores sW.  No alignment rule for W.
 *
 * ipmz_qp_device_grad is ipmz_qp_device_data with writable blocks and the same
 * rules: strides in elements; a NULL block is not wanted; blocks of dimension 0
 * are ignored whatever they hold; a row stride is at least n; a non-zero QP
 * stride is at least the block's extent; no stride is negative; no alignment
 * rule (16-byte stores where the pointer and strides allow them, element by
 * element otherwise, with equal bits).  Nothing outside the blocks (row
 * padding, the space between QPs) is written.  QP stride non-zero: QP q's block
 * receives that QP's gradient, overwritten, never accumulated.  QP stride 0
 * (batches): the ONE block receives the sum over all QPs -- the gradient of
 * data that ipmz_batch_load_device shared.  Shared vector blocks: the batch is cut
 * into 64 contiguous ranges, each summed in QP order, the ranges' sums then
 * added in range order; shared matrix blocks are a product with the batch as
 * the inner dimension on fp64 MFMA, chunks of 64 QPs each summed in QP order
 * (in groups of four), the chunks' partials then summed in chunk order: an
 * order fixed by the shape alone, no atomics, equal inputs give equal bits.  The partials live
 * in a workspace of the solver (ceil(batch / 64) * max(n, m, p) * n doubles,
 * allocated when a shared matrix block is first asked for, freed with the
 * solver).
 *
 * Asynchronous on the context's stream, no synchronize; the iterate, the
 * step's slots, the scalars, the kept KKT matrix, a captured step graph and all
 * later steps are unchanged, bitwise: the call reads the iterate and W only.
 *
 * Served and refused like the adjoint pair: IPMZ_ERR_INVALID for a null qp, W
 * or grad, bad strides, IPMZ_EQ_SLACKED_SLACKS / IPMZ_EQ_NAIVE_SLACKS, an
 * enabled normal-equations reduction or mixed precision; IPMZ_ERR_STATE before
 * a load, between a load and ipmz_batch_initialize, and when the workspace
 * would have to be allocated while the context's stream is capturing;
 * IPMZ_ERR_NOMEM when it cannot be had. */
typedef struct ipmz_qp_device_grad {
  double* Q;    /* n rows of n */
  int64_t ldq, sQ;
  double* A;    /* m rows of n */
  int64_t lda, sA;
  double* C;    /* p rows of n */
  int64_t ldc, sC;
  double *c, *l_x, *u_x; /* n each */
  int64_t sc, slx, sux;
  double *l_A, *u_A;     /* m each */
  int64_t slA, suA;
  double* d;    /* p */
  int64_t sd;
} ipmz_qp_device_grad;
int ipmz_batch_data_vjp(ipmz_qp* qp, const double* W, int64_t sW, const ipmz_qp_device_grad* grad);

/* The call above for a block of ncot cotangent rows per QP: the last link of
 * a reverse-mode Jacobian, ipmz_*_newton_adjoint_multi's nrhs rows contracted
 * with d r / d data in one call instead of a host loop over the rows.
 *
 * W (device): row r of QP q at W + q * sW + r * ldw, ipmz_qp_state_len doubles
 * in the layout of IPMZ_STATE_RES -- the adjoint pair's Out with ldw = ldo and
 * sW = sO.  ldw >= state_len; on batches sW >= (ncot - 1) * ldw + state_len.  A
 * solver of one QP ignores sW.  No alignment rule for W.
 *
 * ipmz_qp_device_grad_multi is ipmz_qp_device_grad (blocks, row strides, QP
 * strides) plus a cotangent-row stride per block: row r of QP q of block X
 * starts at X + q * sX + r * tX.  The rules are ipmz_qp_device_tangent's with
 * writable blocks: strides in elements; a NULL block is not wanted; blocks of
 * dimension 0 are ignored whatever they hold; a row stride is at least n; no
 * stride is negative; with ncot > 1 a cotangent-row stride is at least the
 * block's extent and a non-zero QP stride at least (ncot - 1) * tX + extent (a
 * call with one row does not look at tX); no alignment rule (16-byte stores
 * where the pointer and all three strides allow them, element by element
 * otherwise, with equal bits).  Nothing outside the blocks (row padding, the
 * space between rows and QPs) is written.  QP stride 0 (batches): ncot blocks,
 * block r receiving the sum over all QPs of row r's gradient.
 *
 * Row contract: every row's blocks are bitwise what ipmz_batch_data_vjp writes
 * for that row alone (W + r * ldw, sW), per QP and shared; the summation order
 * of a shared block is the one stated above -- chunks of 64 QPs, groups of
 * four in QP order, chunks in chunk order, the 64 ranges for vectors -- fixed
 * by the batch size alone, whatever ncot.  No atomics, no cross-workgroup
 * waiting.  In a shared matrix block x and the iterate's dual do not depend on
 * the row: a wave keeps them in registers over a group of 4 rows.
 *
 * Workspace: the shared matrix blocks' partials pass through the workspace of
 * ipmz_batch_data_vjp in slabs of 16 rows, one slab after the other on the
 * stream: ceil(batch / 64) * min(ncot, 16) * max(n, m, p) * n doubles, grown
 * for the largest need seen, never linear in ncot.
 *
 * ncot == 0 is a no-op.  Asynchronous on the context's stream, no synchronize;
 * the iterate, the step's slots, the scalars, the kept KKT matrix, a captured
 * step graph and all later steps are unchanged, bitwise.
 *
 * Served and refused like ipmz_batch_data_vjp: IPMZ_ERR_INVALID for a null qp,
 * W or grad, ncot < 0, bad strides, IPMZ_EQ_SLACKED_SLACKS /
 * IPMZ_EQ_NAIVE_SLACKS, an enabled normal-equations reduction or mixed
 * precision; IPMZ_ERR_STATE before a load, between a load and
 * ipmz_batch_initialize, and when the workspace would have to grow while the
 * context's stream is capturing; IPMZ_ERR_NOMEM when it cannot be had. */
typedef struct ipmz_qp_device_grad_multi {
  ipmz_qp_device_grad g;                           /* blocks, row strides, QP strides */
  int64_t tQ, tA, tC, tc, tlx, tux, tlA, tuA, td;  /* cotangent-row strides, in elements */
} ipmz_qp_device_grad_multi;
int ipmz_batch_data_vjp_multi(ipmz_qp* qp, int ncot, const double* W, int64_t ldw, int64_t sW,
                              const ipmz_qp_device_grad_multi* grad);

/* The first link of a forward pass through a solved QP: tangents of the problem
 * data in, the tangents of the residual vectors out.  At a fixed iterate and a
 * fixed mu every r_v is affine in the data, so for tangent t < ntan of QP q
 *
 *     R[q][t] = (d r / d theta) D_t,
 *
 * the linear part of r in the data evaluated at the tangents, in the layout of
 * IPMZ_STATE_RES.  With dz = -J^{-1} r_theta dtheta (above) and Dir = -J^{-1} R
 * of ipmz_*_newton_solve_multi, Dir of this R is the tangent of the whole
 * Newton state; its leading n entries are dx*:
 *
 *     data tangents -> R (this call) -> ipmz_*_newton_solve_multi -> dz.
 *
 * In the default form: r_x = dQ x + dc + dA^T lambda_A + dC^T lambda_C;
 * r_lambda_A = dA x; r_lambda_C = dC x - dd (all three equality handlings);
 * r_lambda_y = dl_x, r_lambda_z = -du_x, r_lambda_g = dl_A, r_lambda_h = -du_A.
 * IPMZ_INEQ_SLACKS: the bounds enter multiplied by the duals (r_lambda_y =
 * -lambda_y dl_x, r_lambda_z = lambda_z du_x, and so for l_A, u_A).
 * IPMZ_INEQ_NAIVE_SLACKS: r_x has dA^T (lambda_h - lambda_g), r_lambda_g = dl_A
 * - dA x, r_lambda_h = dA x - du_A.  A bound the formulation does not have
 * contributes nothing.  mu is a constant of the call, as for the vjp; the n^2
 * entries of dQ are independent.
 *
 * ipmz_qp_device_tangent is ipmz_qp_device_data (blocks, row strides, QP
 * strides: the rules of ipmz_batch_load_device) plus a tangent stride per
 * block: tangent t of QP q of block X starts at X + q * sX + t * tX.  Strides in
 * elements; a row stride is at least n; no stride is negative; blocks of
 * dimension 0 are ignored whatever they hold; a NULL block is a zero tangent.
 * With ntan > 1 a tangent stride is at least the block's extent; a non-zero QP
 * stride is at least (ntan - 1) * tX + extent.  QP stride 0 (batches): ONE set
 * of ntan tangents shared by every QP -- the tangent of data that
 * ipmz_batch_load_device shared.  No alignment rule (16-byte loads where the
 * pointer and all three strides allow them, element by element otherwise, with
 * equal bits).  Nothing outside the blocks (row padding, the space between
 * tangents and QPs) is read.
 *
 * R (device): row (q, t) at R + q * sR + t * ldr receives all L =
 * ipmz_qp_state_len doubles; slots no datum enters (r_s, r_p, the
 * complementarity rows of the SlackedSlacks and NaiveSlacks forms) are written
 * as zeros.  R[q][t][L .. ldr) and everything between ntan * ldr and sR keep
 * their bits.  R, ldr and sR obey the rules of ipmz_batch_newton_solve_multi's
 * R, so that the output feeds that call directly, in place if the caller
 * likes: ldr >= L and even; sR >= ntan * ldr and even; R 16-byte aligned.  A
 * solver of one QP ignores the QP strides and sR.  ntan == 0 is a no-op.
 *
 * Per-QP tangent matrices are one bandwidth-bound pass that reads every element
 * once (dA serves dA x and dA^T lambda from the same load); shared tangent
 * matrices are products on fp64 MFMA with the batch as a tile dimension.  The
 * products go through a workspace of the solver (batch * ntan segments; per
 * given matrix block the row products' partials, one per tile of up to 512
 * columns, and for A and C the column products' partials, one per chunk of 8 to
 * 32 rows; one partial each for shared blocks: csrc/jvp.hip), allocated on first
 * use, grown for the largest need seen, freed with the solver; one last launch
 * then writes every element of R exactly once.  Stream-ordered
 * launches only, no cross-workgroup waiting, no atomics; the order in which the
 * terms of every element are summed is fixed by (n, m, p) alone: a row's
 * result does not depend on the other rows, a QP's not on the other QPs, equal
 * inputs give equal bits.
 *
 * Asynchronous on the context's stream, no synchronize; the iterate, the
 * step's slots, the scalars, the kept KKT matrix, a captured step graph and all
 * later steps are unchanged, bitwise: the call reads the iterate and the
 * tangents only.
 *
 * Served and refused exactly like ipmz_batch_data_vjp: IPMZ_ERR_INVALID for a
 * null qp, tan or R, bad strides or alignment of R, ntan < 0,
 * IPMZ_EQ_SLACKED_SLACKS / IPMZ_EQ_NAIVE_SLACKS, an enabled normal-equations
 * reduction or mixed precision; IPMZ_ERR_STATE before a load, between a load
 * and ipmz_batch_initialize, and when the workspace would have to be allocated
 * while the context's stream is capturing; IPMZ_ERR_NOMEM when it cannot be
 * had. */
typedef struct ipmz_qp_device_tangent {
  ipmz_qp_device_data d;  /* blocks, row strides, QP strides: the rules of ipmz_batch_load_device */
  int64_t tQ, tA, tC, tc, tlx, tux, tlA, tuA, td;  /* tangent strides, in elements */
} ipmz_qp_device_tangent;
int ipmz_batch_data_jvp(ipmz_qp* qp, int ntan, const ipmz_qp_device_tangent* tan, double* R, int64_t ldr, int64_t sR);

/* Centering on the central path: damped Newton iterations from the current
 * iterate toward the point z with r(z; mu = kappa) = 0 of every QP of the
 * solver (a solver of ipmz_qp_create is a batch of one), kappa > 0 a constant
 * of the call.  Why: the adjoint, vjp and jvp calls above differentiate the
 * Newton system at the current iterate with mu held constant.  At the final
 * iterate of a solve (mu about 1e-9, a function of the data) that is the
 * derivative of the solution map only where strict complementarity holds.  On
 * the central path at a FIXED kappa the Jacobian J is nonsingular whatever the
 * active set, theta -> z(theta; kappa) is smooth, and the same calls, unchanged,
 * return its exact derivative, duals included.  The solve loop and its stop
 * rule are not touched; call this after a solve.
 *
 * Per iteration, on the context's stream:
 *   test       r_v(z; mu = kappa) of every QP by the step's own residual pass,
 *              e_q = ||r||_inf over all ipmz_qp_state_len entries (workgroup
 *              partials, then their maximum in index order: no atomics).  A QP
 *              with e_q <= tol is centered and frozen from then on: its iterate
 *              keeps its bits and it takes part in no later update.  A NaN
 *              never passes.
 *   direction  d = -J^{-1} r: the map of ipmz_*_newton_solve_multi for one row
 *              per QP -- the same assembly, the formulation's own factor (fp64
 *              LDL^T, Bunch-Kaufman for IPMZ_EQ_NONE), the same solves and
 *              slack-first back-substitution -- and that call's step length
 *              alpha.  Every QP is factored, centered or not.
 *   update     z <- z + 0.995 alpha d for the QPs not centered (the step's own
 *              update rule); the workgroups of the others return at the top of
 *              the launch.
 * The loop ends when every QP is centered or max_iter updates were applied; a
 * test follows the last update.  The host looks at the device once per
 * iteration -- two doubles of a summary launch and the factor's words -- never
 * at batch x state_len values.  max_iter == 0 tests, evaluates and reports, and
 * moves nothing.
 *
 * Afterwards every QP is evaluated as ipmz_batch_set_state does: the residual
 * slots and the scalar block are bitwise what ipmz_batch_set_state(qp, q, z_q)
 * leaves (IPMZ_SC_MU about kappa; IPMZ_SC_CONVERGED 0 for kappa > 1e-8), and
 * later steps continue from there.
 *
 * iterations (host, batch ints, may be NULL): the updates QP q received.
 * centered_count (host, may be NULL): the QPs that passed the test.  Returns as
 * the Newton-solve pair does: the smallest non-zero factor info word any
 * iteration met, else IPMZ_OK; a raised sticky error word is IPMZ_ERR_HIP.  The
 * call synchronizes.
 *
 * Only stream-ordered launches, no cross-workgroup waiting, no atomics: a QP's
 * result does not depend on the other QPs of the batch (given the same kernel
 * selection), and equal inputs give equal bits.  The Newton formulas are not
 * restated: the kernels are the step's residual pass and update and the
 * Newton-solve pair's right-hand side, back-substitution and ratio test.
 * Overwritten: the iterate, the direction slot (IPMZ_STATE_DIR), the residual
 * slots and the scalar block's evaluated entries.  Untouched: the data, a
 * captured step graph, the blocking, the restart snapshot, IPMZ_SC_STEPS and
 * the scalar block's layout.  A small device buffer of the solver (a few
 * doubles per QP and workgroup) is allocated on first use.
 *
 * Served: every formulation ipmz_*_newton_solve_multi serves except those
 * below; single QPs of any N; batches on every path that call has (the
 * one-launch blocked solve, the panel chain for N > 1024, inner block 128,
 * IPMZ_EQ_NONE batches with N <= 4096).
 * IPMZ_ERR_INVALID, before anything is enqueued: a null qp; kappa or tol not
 * finite or <= 0; max_iter < 0; an enabled normal-equations reduction or mixed
 * precision; IPMZ_EQ_SLACKED_SLACKS / IPMZ_EQ_NAIVE_SLACKS (as the Newton-solve
 * pair); IPMZ_EQ_PENALTY / IPMZ_EQ_PENALTY_EXTRA_DUAL (their KKT block is
 * -mu I with the environment's mu, which centering would have to own);
 * IPMZ_INEQ_SLACKS (its solves never converge -- the reference's corrector
 * defect -- so there is no solved iterate to center); IPMZ_EQ_NONE batches
 * with N > 4096.  IPMZ_ERR_STATE: before a load, between a load and
 * ipmz_batch_initialize, and while the context's stream is capturing.
 *
 * tol and max_iter are the caller's: 1e-10 and 30 (the Python defaults) come
 * from a CPU prototype of this loop in numpy -- generated QPs (48,16,8),
 * (130,40,22), (12,0,0) at kappa 1e-2 .. 1e-6 centered in 2-6 iterations from a
 * converged iterate, a diagonal box QP with coordinates on a bound in 9-12.
 * Measured on an MI355X (DESIGN.md "Centering on the central path",
 * profiles/center/bench.json): 1024 QPs of n = 256, m = 48, p = 16 and one QP
 * of n = 8192, m = 2048, p = 1024 are centered in at most 11 iterations at
 * kappa 1e-2 .. 1e-6; an iteration costs 1.23 and 0.98 Newton steps there. */
int ipmz_batch_center(ipmz_qp* qp, double kappa, double tol, int max_iter,
                      int* iterations /* host, batch ints, may be NULL */,
                      int* centered_count /* host, may be NULL */);

/* Phase timing (HIP events on the context stream; eager launches only).
 * ms: host array of IPMZ_PH_COUNT floats, cumulative since enable. */
enum ipmz_phase {
  IPMZ_PH_STEP = 0, IPMZ_PH_ASSEMBLE, IPMZ_PH_FACTOR, IPMZ_PH_SOLVE, IPMZ_PH_TRAILING, IPMZ_PH_EVAL,
  IPMZ_PH_COUNT = 8
};
int ipmz_qp_set_timing(ipmz_qp* qp, int enable);
int ipmz_qp_phase_times(ipmz_qp* qp, double* ms, double* trailing_flops, int64_t* trailing_launches);

#ifdef __cplusplus
}
#endif
#endif /* IPMZ_H */
