// C ABI of libipmz (include/ipmz.h): contexts, workspaces and the
// LinearSolvers entry points (the Newton-step solver object is qp.cpp).  Host
// orchestration only -- all arithmetic runs in the gfx950 kernels of ldlt.hip
// / trsv.hip / newton.hip.  There is deliberately no CPU fallback: without a
// device every computing entry point fails with IPMZ_ERR_NO_DEVICE.
#include "capi.h"

#include <cstring>

namespace {
thread_local std::string g_last_error;
}

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
int hip_fail(hipError_t e, const char* expr, const char* file, int line) {
  return fail(IPMZ_ERR_HIP, std::string(expr) + ": " + hipGetErrorString(e) + " @" + file + ":" + std::to_string(line));
}

std::mutex g_ctx_mutex;

// The pool's events only order the factor's streams on one device: no
// system-scope release / acquire fence when one is recorded or waited for
// (the default writes the L2 back for the host at every record, on the
// panel chain's stream between every two chain launches); a runtime that
// refuses the flag gets the default events
static int ensure_events(ipmz_ctx* ctx, size_t n) {
  while (ctx->evpool.size() < n) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess &&
        hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
      return fail(IPMZ_ERR_HIP, "hipEventCreate failed");
    ctx->evpool.push_back(e);
  }
  return IPMZ_OK;
}

static int check_device(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(IPMZ_ERR_NO_DEVICE, "no HIP device visible: libipmz has no CPU fallback");
  if (device < 0 || device >= count) return fail(IPMZ_ERR_INVALID, "device index out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(IPMZ_ERR_NO_DEVICE, "device query failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(IPMZ_ERR_NO_DEVICE, std::string("libipmz is built for gfx950, device is ") + prop.gcnArchName);
  return IPMZ_OK;
}

void ctx_free(ipmz_ctx* ctx) {
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  for (hipStream_t s : {ctx->own, ctx->sB, ctx->sC, ctx->sD})
    if (s) {
      hipStreamSynchronize(s);
      hipStreamDestroy(s);
    }
  for (auto e : ctx->evpool) hipEventDestroy(e);
  delete ctx;
}

// a spin that timed out in the outer-panel factor or the persistent solve
// (sync.h, 0.5 s) means the results are invalid
const char PANEL_TIMEOUT[] = ": a hand-off inside the outer-panel factor kernel timed out (spin limit 0.5 s); the "
                             "factor is invalid";
const char SOLVE_TIMEOUT[] = ": a hand-off inside the persistent triangular solve timed out (spin limit 0.5 s); the "
                             "solution is invalid";
int ws_result(hipStream_t st, const int* info, const unsigned* pe_word, const unsigned* se_word, const char* what,
              const char* pe_text, const char* se_text) {
  int i = 0x7f7f7f7f;
  unsigned pe = 0, se = 0;
  if (pe_word) HIP_OK(hipMemcpyAsync(&pe, pe_word, 4, hipMemcpyDeviceToHost, st));
  if (se_word) HIP_OK(hipMemcpyAsync(&se, se_word, 4, hipMemcpyDeviceToHost, st));
  if (info) HIP_OK(hipMemcpyAsync(&i, info, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (pe) return fail(IPMZ_ERR_HIP, std::string(what) + pe_text);
  if (se) return fail(IPMZ_ERR_HIP, std::string(what) + se_text);
  return i == 0x7f7f7f7f ? IPMZ_OK : i;
}

int read_info(ipmz_ctx* ctx, const LdltWs& w) {
  return ws_result(ctx->stream, w.info, w.pctrl + PANEL_ERR_WORD, w.ctrl + SOLVE_ERR_WORD, "ipmz_ldlt_factor");
}

// the solve: one persistent launch for nbi == 64 (trsv_persist.hip), else
// the block-step kernel chain (trsv.hip)
hipError_t solve_ws(const double* K, int64_t ld, int N, const double* D, const LdltWs& w, int nbi, double* b,
                    hipStream_t st) {
  if (nbi == 64) return ldlt_solve_persistent(K, ld, N, D, w.P, b, w.y, w.z, w.ctrl, st);
  return ldlt_solve(K, ld, N, D, w.Linv, nbi, b, w.side, st);
}

hipError_t solve_ws_tail(const double* K, int64_t ld, int N, const double* D, const LdltWs& w, double* b, int rows,
                         hipStream_t st) {
  return ldlt_solve_persistent_tail(K, ld, N, D, w.P, b, w.y, w.z, w.ctrl, rows, st);
}

int chain_bound_rows(int N, int nbo) {
  int k = 0;
  while (N - k * nbo > IPMZ_EARLY_CHAIN_MAX_N) ++k;
  const int r = k * nbo / IPMZ_SOLVE_BLOCK * IPMZ_SOLVE_BLOCK;
  return r >= N - IPMZ_SOLVE_BLOCK ? 0 : r;
}

int factor_impl(ipmz_ctx* ctx, int N, double* K, int64_t ld, double* D, const LdltWs& w, int nbo, TrailTimer* timer,
                int* info2, StepEdges* edges) {
  // one launch: info, the panel ctrl words and the persistent solve's state
  // for this factor
  HIP_OK(solve_reset(w.y, w.z, sizeof(double), N, w.ctrl, ctx->stream, w.info, w.pctrl, panel_ctrl_words(N, nbo),
                     info2));
  const int npan = (N + nbo - 1) / nbo;
  // the persistent solve's per-block operators, built once from this factor
  auto prep = [&]() -> hipError_t {
    return ctx->nbi == 64 ? solve_prep(K, ld, N, w.Linv, w.P, ctx->stream) : hipSuccess;
  };
  FactorHooks hooks;
  if (edges) {
    edges->swept = false;
    hooks.before_b = edges->rest;
  }
  if (npan < 3 || (debug_inject_mask() & IPMZ_DEBUG_ONE_STREAM)) {
    HIP_OK(ldlt_factor(K, ld, N, D, w.Linv, w.W, nbo, ctx->nbi, w.info, ctx->stream, timer, nullptr, nullptr, nullptr,
                       0, w.pctrl, nullptr, edges ? &hooks : nullptr));
    HIP_OK(prep());
    return IPMZ_OK;
  }
  // ldlt_factor's 5 npan + 3, its hook's, the early sweep's; the fork, one spare
  const int nev = 5 * npan + 7;
  int rc = ensure_events(ctx, (size_t)nev + 4);
  if (rc) return rc;
  hipEvent_t* ev = ctx->evpool.data();
  // the back edge: the leading rows' operators and forward sweep on the
  // fourth stream, which this factor leaves idle
  hipEvent_t evSwept = ev[5 * npan + 4];
  const int R = edges && ctx->nbi == 64 && edges->rows % IPMZ_SOLVE_BLOCK == 0 && edges->rows < N ? edges->rows : 0;
  if (R > 0) {
    hooks.final_rows = R;
    hooks.final_st = ctx->sD;
    hooks.rows_final = [&](hipStream_t s4) -> hipError_t {
      hipError_t e = solve_prep_split(K, ld, N, w.Linv, w.P, R, true, s4);
      if (e == hipSuccess) e = ldlt_solve_persistent_head(K, ld, N, D, w.P, edges->b, w.y, w.z, w.ctrl, R, s4);
      if (e == hipSuccess) e = stream_record(evSwept, s4);
      return e;
    };
  }
  // the fourth look-ahead stream pays for the fp32 factor only (C5 23.6 ->
  // 22.9 ms per step); the fp64 one runs faster without it (C3 14.2 -> 14.0
  // ms), profiles/r03_s5/fourth_stream_ab.log -- not forked at all here
  const bool fourth = false;
  // the panel chain on the caller's stream itself: its first launch follows
  // the assembly in stream order, with no cross-queue hop; ldlt_factor forks
  // B (trailing updates) and C (rows launches) from it and joins them back
  // (a fork onto A cost the C2 step ~70 us of host enqueue before the first
  // panel, profiles/r05_s18)
  HIP_OK(ldlt_factor(K, ld, N, D, w.Linv, w.W, nbo, ctx->nbi, w.info, ctx->stream, timer, ctx->sB, ctx->sC, ev,
                     nev - 2, w.pctrl, fourth ? ctx->sD : nullptr, edges ? &hooks : nullptr));
  if (hooks.fired) {  // join the fourth stream; the operators that read rows >= R
    HIP_OK(stream_wait(ctx->stream, evSwept));
    HIP_OK(solve_prep_split(K, ld, N, w.Linv, w.P, R, false, ctx->stream));
    edges->swept = true;
    return IPMZ_OK;
  }
  HIP_OK(prep());
  return IPMZ_OK;
}

// once per factor: L' (into Lp, may be F), then the persistent solve's operators
hipError_t bk_setup(const double* F, int64_t ld, int N, const int* ipiv, const int* info, double* LT, double* Lp,
                    int64_t ldp, const BkWs& w, hipStream_t st) {
  hipError_t e = bk_fast_prepare(F, ld, N, ipiv, info, LT, Lp, ldp, w.meta, st);
  if (e == hipSuccess) e = linv_from_l(Lp, ldp, N, 64, w.Linv, st);
  if (e == hipSuccess) e = solve_prep(Lp, ldp, N, w.Linv, w.P, st);
  if (e == hipSuccess) e = solve_reset(w.y, w.x, sizeof(double), N, w.ctrl, st);
  return e;
}
// b <- A^{-1} b: P^T L'^{-T} D^{-1} L'^{-1} P b, or the one-workgroup sweeps on
// LT when the factor needs the reference's exact interchange order
hipError_t bk_run(const double* Lp, int64_t ldp, int N, const double* LT, const int* ipiv, const BkWs& w, double* b,
                  hipStream_t st) {
  const unsigned* flag = bk_fast_flag(w.meta);
  double* t = bk_fast_tmp(w.meta, N);
  const double* ones = bk_fast_ones(w.meta, N);
  hipError_t e = bk_fast_gather(b, N, w.meta, st);
  if (e == hipSuccess) e = ldlt_solve_persistent_sweep(Lp, ldp, N, ones, w.P, t, w.y, w.x, w.ctrl, false, st, flag);
  if (e == hipSuccess) e = bk_fast_dsolve(w.y, N, w.meta, st);
  if (e == hipSuccess) e = ldlt_solve_persistent_sweep(Lp, ldp, N, ones, w.P, t, w.y, w.x, w.ctrl, true, st, flag);
  if (e == hipSuccess) e = bk_fast_scatter(b, N, w.meta, st);
  if (e == hipSuccess) e = bk_fast_fallback(LT, N, ipiv, b, w.meta, st);
  return e;
}

// factor of S K S in fp32, with the same two-stream look-ahead as the fp64 factor
int mixed_factor_impl(ipmz_ctx* ctx, const double* K, int64_t ld, MixedWs& w, TrailTimer* timer) {
  const int npan = (w.N + w.nbo - 1) / w.nbo;
  if (npan < 3 || (debug_inject_mask() & IPMZ_DEBUG_ONE_STREAM)) {
    HIP_OK(mixed_factor(K, ld, w, ctx->stream, nullptr, nullptr, nullptr, 0, timer));
    HIP_OK(solve_prep(w.K32, w.ld32, w.N, w.Linv32, w.P32, ctx->stream));
    return IPMZ_OK;
  }
  const int nev = 5 * npan + 5;  // ldlt_factor's 5 npan + 3, the fork, one spare
  int rc = ensure_events(ctx, (size_t)nev + 4);
  if (rc) return rc;
  hipEvent_t* ev = ctx->evpool.data();
  const bool fourth = !(debug_inject_mask() & IPMZ_DEBUG_NO_FOURTH);
  // the chain on the caller's stream (factor_impl); ldlt_factor forks and
  // joins B, C and D
  HIP_OK(mixed_factor(K, ld, w, ctx->stream, ctx->sB, ctx->sC, ev, nev - 2, timer, fourth ? ctx->sD : nullptr));
  HIP_OK(solve_prep(w.K32, w.ld32, w.N, w.Linv32, w.P32, ctx->stream));
  return IPMZ_OK;
}

// Multi-right-hand-side solve (trsm.hip).  Panel width of the blocked path
// (IPMZ_SOLVE_MULTI_PANEL) and the number of right-hand sides from which it
// runs; below it the rows go through the single-vector solve one by one.
// Both from tools/solve_multi_bench.py (profiles/solve_multi/bench.json,
// DESIGN.md "Multi-right-hand-side solve"): 256 columns beat 128 and 512 at
// every measured point; the blocked path breaks even with the loop at 6.6
// rows (N = 11264) and 8.5 rows (N = 2560).
static constexpr int SOLVE_MULTI_PANEL = IPMZ_SOLVE_MULTI_PANEL;
static constexpr int SOLVE_MULTI_CROSSOVER = 10;
static_assert(SOLVE_MULTI_PANEL % 128 == 0 && SOLVE_MULTI_PANEL <= IPMZ_TRSM_PANEL_MAX, "panel width");

// nrhs >= 2 rows through the LDL^T factor in w: looped single-vector solves
// below the crossover, the blocked solve from it on
static int ldlt_multi_impl(ipmz_ctx* ctx, int N, const double* K, int64_t ld, const double* D, const LdltWs& w,
                           double* B, int64_t ldb, int nrhs) {
  const MultiPlan plan =
      multi_plan(nrhs, SOLVE_MULTI_CROSSOVER, SOLVE_MULTI_PANEL, debug_inject_mask(), MultiKind::Ldlt);
  if (!plan.blocked) {
    for (int r = 0; r < nrhs; ++r) HIP_OK(solve_ws(K, ld, N, D, w, ctx->nbi, B + (int64_t)r * ldb, ctx->stream));
  } else {
    HIP_OK(ldlt_solve_multi<double>(K, ld, N, D, w.Linv, ctx->nbi, B, ldb, nrhs, plan.width, ctx->stream));
  }
  watch(ctx, w);  // as ipmz_ldlt_solve: the workspace's error words are checked by ipmz_ctx_sync
  return IPMZ_OK;
}

// Multi-right-hand-side Bunch-Kaufman solve (bk.hip bk_multi_*, trsm.hip on
// L').  The blocked kernels are the LDL^T solve's, so the panel width is
// SOLVE_MULTI_PANEL.  BK_MULTI_CROSSOVER: the number of right-hand sides from
// which the blocked path runs, from tools/bk_multi_bench.py
// (profiles/bk_multi/crossover_scan.json and bench.json, DESIGN.md
// "Multi-right-hand-side Bunch-Kaufman solve"): a looped row on the prepared
// workspace costs 71 us (N = 2560) / 382 us (N = 11264), the blocked path 0.76
// / 3.66 ms at ten rows, so they break even at 10.7 / 9.6 rows; 12 is the
// first count at which the blocked path leads by more than the loop's own
// spread at both orders (1.10x / 1.25x; at 10 it loses at N = 2560, at 11 it
// leads by 1.01x, inside the spread).
static constexpr int BK_MULTI_CROSSOVER = 12;

int bk_multi_impl(ipmz_ctx* ctx, int N, const double* F, int64_t ld, const int* ipiv, const double* LT,
                  const double* Lp, int64_t ldp, const BkWs& w, double* B, int64_t ldb, int nrhs) {
  const MultiPlan plan = multi_plan(nrhs, BK_MULTI_CROSSOVER, SOLVE_MULTI_PANEL, debug_inject_mask(), MultiKind::Bk);
  hipStream_t st = ctx->stream;
  if (!plan.blocked) {
    // exactly ipmz_bk_solve's launches for this order, row by row
    for (int r = 0; r < nrhs; ++r) {
      double* b = B + (int64_t)r * ldb;
      if (N < IPMZ_BK_GRID_MIN) HIP_OK(bk_solve(F, ld, N, ipiv, b, 1, 0, 0, 0, st));
      else HIP_OK(bk_run(Lp, ldp, N, LT, ipiv, w, b, st));
    }
  } else {
    // every stage exits on the fallback flag, read on the device; the
    // fallback launch is gated the other way
    const unsigned* flag = bk_fast_flag(w.meta);
    HIP_OK(bk_multi_gather(B, ldb, nrhs, N, w.meta, st));
    HIP_OK(trsm_sweep<double>(Lp, ldp, N, w.Linv, 64, B, ldb, nrhs, plan.width, false, st, flag));
    HIP_OK(bk_multi_dsolve(B, ldb, nrhs, N, w.meta, st));
    HIP_OK(trsm_sweep<double>(Lp, ldp, N, w.Linv, 64, B, ldb, nrhs, plan.width, true, st, flag));
    HIP_OK(bk_multi_scatter(B, ldb, nrhs, N, w.meta, st));
    HIP_OK(bk_multi_fallback(LT, N, ipiv, B, ldb, nrhs, w.meta, st));
  }
  watch(ctx, w);  // the persistent sweeps' error word is checked by ipmz_ctx_sync
  return IPMZ_OK;
}

// Batches of Bunch-Kaufman systems of one order (one workgroup per matrix) -----
// BK_BATCH_MULTI_CROSSOVER: the number of right-hand sides per system from
// which the blocked paths run; below it every row is one launch of the step's
// own batched single-vector solve (bk_solve), all systems at once.  From
// tools/batch_bk_multi_bench.py (profiles/batch_bk_multi/bench.json, DESIGN.md
// "Batched multi-right-hand-side Bunch-Kaufman solve"), solve alone = call(nrhs)
// - call(0), the blocked legs including their once-per-call prepare: the loop
// costs 3.58 ms for 2 rows and 4.80 ms for 3 (C4 with EQ_NONE, N = 320, batch
// 1024) / 1.05 and 1.49 ms (batch 128), the one-launch solve 1.39-1.43 / 0.26
// ms, far outside the loop's spread (0.09 / 0.04 ms): by BATCH_MULTI_CROSSOVER's
// rule the constant would be 2.  It is 4 because the tests pin nrhs = 3 to the
// loop's bitwise property (three rows are three one-row calls), as they do for
// ipmz_batch_kkt_solve; 2 is the measured choice once that case may change.
// Fused or panels: no panel width leads the one-launch solve by more than the
// spread at both C4 batch sizes at any count, so eligibility alone decides.
static constexpr int BK_BATCH_MULTI_CROSSOVER = 4;

int bk_batch_info(hipStream_t st, const int* dinfo, int batch, int* info) {
  std::vector<int> h((size_t)batch, 0);
  HIP_OK(hipMemcpyAsync(h.data(), dinfo, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  int rc = 0;
  for (int q = 0; q < batch; ++q) {
    if (info) info[q] = h[q];
    if (h[q] != 0 && (rc == 0 || h[q] < rc)) rc = h[q];
  }
  return rc;
}

// the batch's strides as the kernels take them: the prepared workspace's, and the caller's for F, ipiv and B
static BkBatch bk_batch(const BkBatchWs& w, int batch, int64_t sA, int64_t sP, int64_t sB) {
  return BkBatch{batch, sA, sP, w.sLT, w.sLp, sB};
}
// ... and as the blocked sweeps take them (K = L', no D; the gate: a flagged system's launches exit)
static TrsmBatch trsm_batch(const BkBatchWs& w, int batch, int64_t sB) {
  return TrsmBatch{batch, w.sLp, 0, w.sLinv, sB, w.sM / (int64_t)sizeof(unsigned)};
}

int bk_batch_prepare(ipmz_ctx* ctx, int N, int batch, const double* F, int64_t ld, int64_t sA, const int* ipiv,
                     int64_t sP, const int* info, const BkBatchWs& w) {
  hipStream_t st = ctx->stream;
  const BkBatch bb = bk_batch(w, batch, sA, sP, 0);
  HIP_OK(bk_transpose(F, ld, N, w.LT, st, bb));
  HIP_OK(bk_fast_prepare(F, ld, N, ipiv, info, w.LT, w.Lp, w.ldp, w.meta, st, bb));
  HIP_OK(linv_from_l(w.Lp, w.ldp, N, 64, w.Linv, st, batch, w.sLp, w.sLinv));
  return IPMZ_OK;
}

int bk_batch_multi_impl(ipmz_ctx* ctx, int N, int batch, const double* F, int64_t ld, int64_t sA, const int* ipiv,
                        int64_t sP, const BkBatchWs& w, double* B, int64_t ldb, int64_t sB, int nrhs) {
  const MultiPlan plan =
      multi_plan(nrhs, BK_BATCH_MULTI_CROSSOVER, SOLVE_MULTI_PANEL, debug_inject_mask(), MultiKind::Batch);
  hipStream_t st = ctx->stream;
  if (!plan.blocked) {
    // the step's own kernel, one launch per row for all systems
    for (int r = 0; r < nrhs; ++r) HIP_OK(bk_solve(F, ld, N, ipiv, B + (int64_t)r * ldb, batch, sA, sP, sB, st));
    return IPMZ_OK;
  }
  const BkBatch bb = bk_batch(w, batch, sA, sP, sB);
  const TrsmBatch tb = trsm_batch(w, batch, sB);
  const unsigned* flag = bk_fast_flag(w.meta);
  // one launch per batch where a system's slab fits a workgroup's LDS, unless
  // a panel width is forced; then the flagged systems' reference sweeps
  if (plan.fused && bk_solve_fused_eligible(N)) {
    HIP_OK(bk_solve_fused(w.Lp, w.ldp, N, w.Linv, B, ldb, nrhs, bk_fused_meta(w.meta, N, bb), st, tb));
    HIP_OK(bk_multi_fallback_batch(w.LT, N, ipiv, B, ldb, nrhs, w.meta, st, bb));
    return IPMZ_OK;
  }
  HIP_OK(bk_multi_gather(B, ldb, nrhs, N, w.meta, st, bb));
  HIP_OK(trsm_sweep<double>(w.Lp, w.ldp, N, w.Linv, 64, B, ldb, nrhs, plan.width, false, st, flag, tb));
  HIP_OK(bk_multi_dsolve(B, ldb, nrhs, N, w.meta, st, bb));
  HIP_OK(trsm_sweep<double>(w.Lp, w.ldp, N, w.Linv, 64, B, ldb, nrhs, plan.width, true, st, flag, tb));
  HIP_OK(bk_multi_scatter(B, ldb, nrhs, N, w.meta, st, bb));
  HIP_OK(bk_multi_fallback_batch(w.LT, N, ipiv, B, ldb, nrhs, w.meta, st, bb));
  return IPMZ_OK;
}

// Mixed-precision multi-right-hand-side solve (mixed_multi.hip, trsm.hip).
// MIXED_MULTI_PANEL: column panel of the blocked fp32 solve;
// MIXED_MULTI_CROSSOVER: the number of right-hand sides from which the blocked
// refinement runs -- below it the rows go through mixed_solve one by one.
// Both from tools/mixed_multi_bench.py (profiles/mixed_multi/bench.json and
// crossover_scan.json, DESIGN.md "Mixed-precision multi-right-hand-side
// solve"): 256 columns beat 128 and 512 at every measured point.  At tol =
// 1e-12, max_refine = 20 the blocked path breaks even with the loop at 5.0
// rows (N = 2560) and 5.6 rows (N = 16384) and leads by 1.41x / 1.25x at 7.
// That loop pays ~18 skipped passes per vector (it enqueues all max_refine + 1,
// ~30 us each once the stop test holds: 0.5 of its 2.4 ms at N = 16384);
// with a small max_refine it does not, which moves the break-even at N = 16384
// to ~7.1 rows.  8 is the first count with a clear margin either way
// (measured 1.60x / 1.43x).
static constexpr int MIXED_MULTI_PANEL = 256;
static constexpr int MIXED_MULTI_CROSSOVER = 8;
static_assert(MIXED_MULTI_PANEL % 128 == 0 && MIXED_MULTI_PANEL <= IPMZ_TRSM_PANEL_MAX, "panel width");

// nrhs >= 2 rows through the factor in w (w.hst == nullptr: the looped solves
// enqueue all their passes); stats left in m.stat, copied to stat (host, may be
// null); synchronizes
int mixed_multi_impl(ipmz_ctx* ctx, const double* K, int64_t ld, MixedWs& w, const MixedMultiWs& m, double* B,
                     int64_t ldb, int nrhs, double tol, int max_refine, double* stat) {
  const MultiPlan plan =
      multi_plan(nrhs, MIXED_MULTI_CROSSOVER, MIXED_MULTI_PANEL, debug_inject_mask(), MultiKind::Ldlt);
  hipStream_t st = ctx->stream;
  if (!plan.blocked) {
    for (int r = 0; r < nrhs; ++r) {
      HIP_OK(mixed_solve(K, ld, w, B + (int64_t)r * ldb, tol, max_refine, st));
      HIP_OK(hipMemcpyAsync(m.stat + 2 * r, w.stat, 2 * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
  } else {
    HIP_OK(mixed_solve_multi(K, ld, w, m, B, ldb, nrhs, tol, max_refine, plan.width, st));
  }
  if (stat) HIP_OK(hipMemcpyAsync(stat, m.stat, (size_t)nrhs * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return IPMZ_OK;
}

int not_capturing(ipmz_ctx* ctx, const char* who) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIP_OK(hipStreamIsCapturing(ctx->stream, &cs));
  if (cs != hipStreamCaptureStatusNone)
    return fail(IPMZ_ERR_STATE, std::string(who) + ": the context's stream is capturing a hipGraph; this call waits "
                                                   "for its stop test on the host and cannot be captured");
  return IPMZ_OK;
}

// The normal equations as the x-first blocked LDL^T of [[H, B^T], [B, -E]]
// (normal.hip): Cholesky(H), the TRSM of B, the SYRK into the (2,2) block and
// Cholesky(S) in one pipelined factor; then H's pivots > 0, S's < 0.
int normal_factor_impl(ipmz_ctx* ctx, int n, int mp, double* K, int64_t ld, double* D, const NormalWs& w, int nbo,
                       TrailTimer* timer) {
  hipStream_t st = ctx->stream;
  int rc = factor_impl(ctx, n + mp, K, ld, D, w.k, nbo, timer, w.info);
  if (rc) return rc;
  HIP_OK(ne_check_sign(D, n, 0, 1.0, w.info, st));
  HIP_OK(ne_check_sign(D + n, mp, n, -1.0, w.info, st));
  return IPMZ_OK;
}

// b = [r0; r1] <- [x; l]: the factor's forward and backward sweeps
int normal_solve_impl(ipmz_ctx* ctx, int n, int mp, const double* K, int64_t ld, const double* D, const NormalWs& w,
                      double* b) {
  HIP_OK(solve_ws(K, ld, n + mp, D, w.k, ctx->nbi, b, ctx->stream));
  return IPMZ_OK;
}

namespace {
// Host adapters: device storage for the length of one call
template <typename T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { hipFree(p); }
  bool alloc(int64_t count) { return hipMalloc(&p, (size_t)count * sizeof(T)) == hipSuccess; }
  operator T*() const { return p; }
};
// rows x n elements between a dense host array and a device array of row
// stride ld (one row: a vector, one plain copy); true when enqueued
template <typename T>
bool rows_in(T* dev, int64_t ld, const T* host, int64_t n, int rows, hipStream_t st) {
  const size_t w = (size_t)n * sizeof(T);
  return (rows == 1 ? hipMemcpyAsync(dev, host, w, hipMemcpyHostToDevice, st)
                    : hipMemcpy2DAsync(dev, ld * sizeof(T), host, w, w, rows, hipMemcpyHostToDevice, st)) == hipSuccess;
}
template <typename T>
bool rows_out(T* host, const T* dev, int64_t ld, int64_t n, int rows, hipStream_t st) {
  const size_t w = (size_t)n * sizeof(T);
  return (rows == 1 ? hipMemcpyAsync(host, dev, w, hipMemcpyDeviceToHost, st)
                    : hipMemcpy2DAsync(host, w, dev, ld * sizeof(T), w, rows, hipMemcpyDeviceToHost, st)) == hipSuccess;
}
}  // namespace

extern "C" {

const char* ipmz_last_error(void) { return g_last_error.c_str(); }

int ipmz_ctx_create(ipmz_ctx** out, int device) {
  if (!out) return fail(IPMZ_ERR_INVALID, "null out");
  *out = nullptr;
  int rc = check_device(device);
  if (rc) return rc;
  HIP_OK(hipSetDevice(device));
  auto* c = new ipmz_ctx();
  c->device = device;
  int least = 0, greatest = 0;
  hipDeviceGetStreamPriorityRange(&least, &greatest);
  // own: the steps' stream, and the factor's panel chain (high priority)
  if (hipStreamCreateWithPriority(&c->own, hipStreamNonBlocking, greatest) != hipSuccess) {
    delete c;
    return fail(IPMZ_ERR_HIP, "hipStreamCreate failed");
  }
  c->stream = c->own;
  if (hipStreamCreateWithPriority(&c->sB, hipStreamNonBlocking, least) != hipSuccess ||
      hipStreamCreateWithPriority(&c->sC, hipStreamNonBlocking, greatest) != hipSuccess ||
      hipStreamCreateWithPriority(&c->sD, hipStreamNonBlocking, greatest) != hipSuccess) {
    ipmz_ctx_destroy(c);
    return fail(IPMZ_ERR_HIP, "hipStreamCreateWithPriority failed");
  }
  *out = c;
  return IPMZ_OK;
}

int ipmz_ctx_destroy(ipmz_ctx* ctx) {
  if (!ctx) return IPMZ_OK;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mutex);
    if (ctx->closed) return IPMZ_OK;
    ctx->closed = true;
    if (ctx->users > 0) {
      // freed with its last solver: from now on the solvers run on the
      // context's own stream, so that late free never touches a caller's
      // stream whose owner may have released it after this call (what the
      // solvers enqueued there is drained first)
      if (ctx->stream != ctx->own) {
        hipSetDevice(ctx->device);
        hipStreamSynchronize(ctx->stream);
      }
      ctx->stream = ctx->own;
      return IPMZ_OK;
    }
  }
  ctx_free(ctx);
  return IPMZ_OK;
}

int ipmz_ctx_set_stream(ipmz_ctx* ctx, void* s) {
  if (!ctx) return fail(IPMZ_ERR_INVALID, "null ctx");
  ctx->stream = static_cast<hipStream_t>(s);  // NULL = the legacy default stream
  return IPMZ_OK;
}

int ipmz_ctx_reset_stream(ipmz_ctx* ctx) {
  if (!ctx) return fail(IPMZ_ERR_INVALID, "null ctx");
  ctx->stream = ctx->own;
  return IPMZ_OK;
}

int ipmz_ctx_sync(ipmz_ctx* ctx) {
  if (!ctx) return fail(IPMZ_ERR_INVALID, "null ctx");
  HIP_OK(hipStreamSynchronize(ctx->stream));  // (a failure here leaves the watched words watched)
  const unsigned *pe = ctx->check_pe, *se = ctx->check_se;
  unwatch(ctx);
  return pe || se ? ws_result(ctx->stream, nullptr, pe, se, "ipmz_ctx_sync") : IPMZ_OK;
}

int ipmz_debug_inject(int mask) {
  set_debug_inject_mask(mask);
  return IPMZ_OK;
}

int ipmz_ctx_set_blocking(ipmz_ctx* ctx, int nbo, int nbi) {
  if (!ctx) return fail(IPMZ_ERR_INVALID, "null ctx");
  if ((nbi != 64 && nbi != 128) || (nbo != 0 && (nbo < nbi || nbo % nbi != 0 || nbo > IPMZ_NBO_MAX)))
    return fail(IPMZ_ERR_INVALID, "blocking: nbi in {64,128}, nbo 0 (auto) or a multiple of nbi, <= 512");
  ctx->nbo = nbo;
  ctx->nbi = nbi;
  return IPMZ_OK;
}

int ipmz_ctx_get_blocking(ipmz_ctx* ctx, int N, int* nbo, int* nbi) {
  if (!ctx || N < 0 || !nbo || !nbi) return fail(IPMZ_ERR_INVALID, "ipmz_ctx_get_blocking: bad arguments");
  *nbo = nbo_for(ctx, N);
  *nbi = ctx->nbi;
  return IPMZ_OK;
}

// fp64 LDL^T ------------------------------------------------------------------
int64_t ipmz_ldlt_workspace_bytes(ipmz_ctx* ctx, int N) {
  if (!ctx || N < 0) return 0;
  return ldlt_ws(nullptr, N, nbo_for(ctx, N), ctx->nbi).total;
}

int ipmz_ldlt_factor(ipmz_ctx* ctx, int N, double* K, int64_t ld, double* D, void* ws, int64_t ws_bytes) {
  if (!ctx || N < 0 || (N > 0 && (!K || !D || !ws)) || ld < N || (ld & 1))
    return fail(IPMZ_ERR_INVALID, "ipmz_ldlt_factor: bad arguments (ld >= N, ld even)");
  if (N == 0) return IPMZ_OK;
  const int nbo = nbo_for(ctx, N);
  const LdltWs w = ldlt_ws(static_cast<char*>(ws), N, nbo, ctx->nbi);
  if (ws_bytes < w.total) return fail(IPMZ_ERR_INVALID, "workspace too small");
  HIP_OK(hipSetDevice(ctx->device));
  int rc = factor_impl(ctx, N, K, ld, D, w, nbo, nullptr);
  if (rc) return rc;
  return read_info(ctx, w);  // synchronous: checks the error words itself
}

int ipmz_ldlt_solve(ipmz_ctx* ctx, int N, const double* K, int64_t ld, const double* D, const void* ws, double* b) {
  if (!ctx || N < 0 || ld < N) return fail(IPMZ_ERR_INVALID, "ipmz_ldlt_solve: bad arguments");
  if (N == 0) return IPMZ_OK;
  HIP_OK(hipSetDevice(ctx->device));
  const LdltWs w = ldlt_ws(static_cast<char*>(const_cast<void*>(ws)), N, nbo_for(ctx, N), ctx->nbi);
  HIP_OK(solve_ws(K, ld, N, D, w, ctx->nbi, b, ctx->stream));
  // its error words are checked by ipmz_ctx_sync (addresses resolved now: a
  // later ipmz_ctx_set_blocking does not move them)
  watch(ctx, w);
  return IPMZ_OK;
}

int ipmz_ldlt_prepare_solve(ipmz_ctx* ctx, int N, const double* L, int64_t ld, void* ws, int64_t ws_bytes) {
  if (!ctx || N < 0 || ld < N) return fail(IPMZ_ERR_INVALID, "ipmz_ldlt_prepare_solve: bad arguments");
  if (N == 0) return IPMZ_OK;
  const int nbo = nbo_for(ctx, N);
  const LdltWs w = ldlt_ws(static_cast<char*>(ws), N, nbo, ctx->nbi);
  if (ws_bytes < w.total) return fail(IPMZ_ERR_INVALID, "workspace too small");
  HIP_OK(hipSetDevice(ctx->device));
  HIP_OK(linv_from_l(L, ld, N, ctx->nbi, w.Linv, ctx->stream));
  if (ctx->nbi == 64) HIP_OK(solve_prep(L, ld, N, w.Linv, w.P, ctx->stream));
  // no factorization ran in this workspace: clear its sticky error words
  HIP_OK(solve_reset(w.y, w.z, sizeof(double), N, w.ctrl, ctx->stream, nullptr, w.pctrl, panel_ctrl_words(N, nbo)));
  return IPMZ_OK;
}

int ipmz_ldlt_solve_multi(ipmz_ctx* ctx, int N, const double* K, int64_t ld, const double* D, const void* ws,
                          double* B, int64_t ldb, int nrhs) {
  if (!ctx || N < 0 || nrhs < 0 || ld < N || ldb < N || (ld & 1) || (ldb & 1))
    return fail(IPMZ_ERR_INVALID, "ipmz_ldlt_solve_multi: bad arguments (nrhs >= 0, ld >= N, ldb >= N, both even)");
  if (N == 0 || nrhs == 0) return IPMZ_OK;
  if (!K || !D || !ws || !B) return fail(IPMZ_ERR_INVALID, "ipmz_ldlt_solve_multi: null pointer");
  if (nrhs == 1) return ipmz_ldlt_solve(ctx, N, K, ld, D, ws, B);
  if (((uintptr_t)K & 15) || ((uintptr_t)B & 15))
    return fail(IPMZ_ERR_INVALID, "ipmz_ldlt_solve_multi: K and B must be 16-byte aligned");
  HIP_OK(hipSetDevice(ctx->device));
  const LdltWs w = ldlt_ws(static_cast<char*>(const_cast<void*>(ws)), N, nbo_for(ctx, N), ctx->nbi);
  return ldlt_multi_impl(ctx, N, K, ld, D, w, B, ldb, nrhs);
}

// Mixed precision (config C5) -------------------------------------------------
int64_t ipmz_mixed_workspace_bytes(ipmz_ctx* ctx, int N) {
  if (!ctx || N < 0) return 0;
  return mixed_ws_bytes(N, nbo_for(ctx, N));
}

int ipmz_mixed_factor(ipmz_ctx* ctx, int N, const double* K, int64_t ld, void* ws, int64_t ws_bytes) {
  if (!ctx || N < 0 || (N > 0 && (!K || !ws)) || ld < N) return fail(IPMZ_ERR_INVALID, "ipmz_mixed_factor: bad arguments");
  if (N == 0) return IPMZ_OK;
  MixedWs w;
  if (ws_bytes < mixed_ws_carve(static_cast<char*>(ws), N, nbo_for(ctx, N), w))
    return fail(IPMZ_ERR_INVALID, "workspace too small");
  HIP_OK(hipSetDevice(ctx->device));
  int rc = mixed_factor_impl(ctx, K, ld, w, nullptr);
  if (rc) return rc;
  return ws_result(ctx->stream, w.info, nullptr, nullptr, "ipmz_mixed_factor");
}

int ipmz_mixed_solve(ipmz_ctx* ctx, int N, const double* K, int64_t ld, void* ws, double* b, double tol,
                     int max_refine, double* stat) {
  if (!ctx || N < 0 || ld < N || max_refine < 0) return fail(IPMZ_ERR_INVALID, "ipmz_mixed_solve: bad arguments");
  if (N == 0) return IPMZ_OK;
  if (!K || !ws || !b) return fail(IPMZ_ERR_INVALID, "null pointer");
  HIP_OK(hipSetDevice(ctx->device));
  MixedWs w;
  mixed_ws_carve(static_cast<char*>(ws), N, nbo_for(ctx, N), w);
  HIP_OK(mixed_solve(K, ld, w, b, tol, max_refine, ctx->stream));
  if (stat) {
    HIP_OK(hipMemcpyAsync(stat, w.stat, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
  }
  return IPMZ_OK;
}

int64_t ipmz_mixed_multi_workspace_bytes(ipmz_ctx* ctx, int N, int nrhs) {
  if (!ctx || N < 0 || nrhs < 0) return 0;
  MixedMultiWs m;
  return mixed_multi_ws_carve(nullptr, N, nrhs, m);
}

int ipmz_mixed_solve_multi(ipmz_ctx* ctx, int N, const double* K, int64_t ld, void* ws, double* B, int64_t ldb,
                           int nrhs, double tol, int max_refine, void* mws, int64_t mws_bytes, double* stat) {
  if (!ctx || N < 0 || nrhs < 0 || max_refine < 0 || ld < N || ldb < N || (ld & 1) || (ldb & 1))
    return fail(IPMZ_ERR_INVALID, "ipmz_mixed_solve_multi: bad arguments (nrhs >= 0, max_refine >= 0, ld >= N, "
                                  "ldb >= N, both even)");
  if (N == 0 || nrhs == 0) return IPMZ_OK;
  if (!K || !ws || !B) return fail(IPMZ_ERR_INVALID, "ipmz_mixed_solve_multi: null pointer");
  HIP_OK(hipSetDevice(ctx->device));
  int rc = not_capturing(ctx, "ipmz_mixed_solve_multi");
  if (rc) return rc;
  if (nrhs == 1) return ipmz_mixed_solve(ctx, N, K, ld, ws, B, tol, max_refine, stat);
  if (((uintptr_t)K & 15) || ((uintptr_t)B & 15))
    return fail(IPMZ_ERR_INVALID, "ipmz_mixed_solve_multi: K and B must be 16-byte aligned");
  MixedMultiWs m;
  if (!mws || mws_bytes < mixed_multi_ws_carve(static_cast<char*>(mws), N, nrhs, m))
    return fail(IPMZ_ERR_INVALID, "ipmz_mixed_solve_multi: multi workspace too small "
                                  "(ipmz_mixed_multi_workspace_bytes(N, nrhs))");
  MixedWs w;
  mixed_ws_carve(static_cast<char*>(ws), N, nbo_for(ctx, N), w);
  return mixed_multi_impl(ctx, K, ld, w, m, B, ldb, nrhs, tol, max_refine, stat);
}

int ipmz_sym_residual_multi(ipmz_ctx* ctx, int N, const double* K, int64_t ld, const double* X, int64_t ldx,
                            const double* B, int64_t ldb, double* R, int64_t ldr, int nrhs) {
  if (!ctx || N < 0 || nrhs < 0 || ld < N || ldx < N || ldb < N || ldr < N || (ld & 1) || (ldx & 1) || (ldb & 1) ||
      (ldr & 1))
    return fail(IPMZ_ERR_INVALID, "ipmz_sym_residual_multi: bad arguments (nrhs >= 0; ld, ldx, ldb, ldr >= N and even)");
  if (N == 0 || nrhs == 0) return IPMZ_OK;
  if (!K || !X || !B || !R) return fail(IPMZ_ERR_INVALID, "ipmz_sym_residual_multi: null pointer");
  if (((uintptr_t)K & 15) || ((uintptr_t)X & 15) || ((uintptr_t)B & 15) || ((uintptr_t)R & 15))
    return fail(IPMZ_ERR_INVALID, "ipmz_sym_residual_multi: K, X, B and R must be 16-byte aligned");
  HIP_OK(hipSetDevice(ctx->device));
  HIP_OK(sym_residual_multi(K, ld, N, X, ldx, B, ldb, R, ldr, nrhs, ctx->stream));
  return IPMZ_OK;
}

// Normal equations (config C2) ------------------------------------------------
int64_t ipmz_normal_workspace_bytes(ipmz_ctx* ctx, int n, int mp) {
  if (!ctx || n <= 0 || mp < 0) return 0;
  return normal_ws(nullptr, n + mp, nbo_for(ctx, n + mp), ctx->nbi).total;
}

int ipmz_normal_factor(ipmz_ctx* ctx, int n, int mp, double* K, int64_t ld, double* D, void* ws, int64_t ws_bytes) {
  if (!ctx || n <= 0 || mp < 0 || !K || !D || !ws || ld < n + mp || (ld & 1))
    return fail(IPMZ_ERR_INVALID, "ipmz_normal_factor: bad arguments (n > 0, ld >= n + mp, ld even)");
  const int nbo = nbo_for(ctx, n + mp);
  const NormalWs w = normal_ws(static_cast<char*>(ws), n + mp, nbo, ctx->nbi);
  if (ws_bytes < w.total) return fail(IPMZ_ERR_INVALID, "workspace too small");
  HIP_OK(hipSetDevice(ctx->device));
  int rc = normal_factor_impl(ctx, n, mp, K, ld, D, w, nbo, nullptr);
  if (rc) return rc;
  if ((rc = ws_result(ctx->stream, w.info, nullptr, nullptr, "ipmz_normal_factor"))) return rc;
  return read_info(ctx, w.k);  // a non-finite pivot of the factor
}

int ipmz_normal_solve(ipmz_ctx* ctx, int n, int mp, const double* K, int64_t ld, const double* D, void* ws,
                      double* b) {
  if (!ctx || n <= 0 || mp < 0 || !K || !D || !ws || !b || ld < n + mp)
    return fail(IPMZ_ERR_INVALID, "ipmz_normal_solve: bad arguments");
  HIP_OK(hipSetDevice(ctx->device));
  const NormalWs w = normal_ws(static_cast<char*>(ws), n + mp, nbo_for(ctx, n + mp), ctx->nbi);
  return normal_solve_impl(ctx, n, mp, K, ld, D, w, b);
}

int ipmz_normal_solve_multi(ipmz_ctx* ctx, int n, int mp, const double* K, int64_t ld, const double* D, void* ws,
                            double* B, int64_t ldb, int nrhs) {
  const int N = n + mp;
  if (!ctx || n <= 0 || mp < 0 || nrhs < 0 || ld < N || ldb < N || (ld & 1) || (ldb & 1))
    return fail(IPMZ_ERR_INVALID, "ipmz_normal_solve_multi: bad arguments (n > 0, nrhs >= 0, ld >= n + mp, "
                                  "ldb >= n + mp, both even)");
  if (nrhs == 0) return IPMZ_OK;
  if (!K || !D || !ws || !B) return fail(IPMZ_ERR_INVALID, "ipmz_normal_solve_multi: null pointer");
  if (nrhs == 1) return ipmz_normal_solve(ctx, n, mp, K, ld, D, ws, B);
  if (((uintptr_t)K & 15) || ((uintptr_t)B & 15))
    return fail(IPMZ_ERR_INVALID, "ipmz_normal_solve_multi: K and B must be 16-byte aligned");
  HIP_OK(hipSetDevice(ctx->device));
  const NormalWs w = normal_ws(static_cast<char*>(ws), N, nbo_for(ctx, N), ctx->nbi);
  return ldlt_multi_impl(ctx, N, K, ld, D, w.k, B, ldb, nrhs);
}

// Bunch-Kaufman (f3) ----------------------------------------------------------
int ipmz_bk_factor(ipmz_ctx* ctx, int N, double* A, int64_t ld, int* ipiv, int fix_kp) {
  return ipmz_bk_factor_ex(ctx, N, A, ld, ipiv, fix_kp, IPMZ_BK_AUTO);
}

int ipmz_bk_factor_ex(ipmz_ctx* ctx, int N, double* A, int64_t ld, int* ipiv, int fix_kp, int algo) {
  if (!ctx || N < 0 || ld < N || (N > 0 && (!A || !ipiv)) || algo < IPMZ_BK_AUTO || algo > IPMZ_BK_GRID)
    return fail(IPMZ_ERR_INVALID, "ipmz_bk_factor: bad arguments");
  const bool grid = algo == IPMZ_BK_GRID || (algo == IPMZ_BK_AUTO && N >= IPMZ_BK_GRID_MIN);
  if (!grid && N > IPMZ_BK_NMAX) return fail(IPMZ_ERR_INVALID, "ipmz_bk_factor: N > 4096 for the one-workgroup factor");
  if (N == 0) return IPMZ_OK;
  HIP_OK(hipSetDevice(ctx->device));
  const size_t wsb = grid ? bk_grid_ws_bytes(N) : 0;
  char* dws = nullptr;
  HIP_OK(hipMallocAsync(reinterpret_cast<void**>(&dws), 256 + wsb, ctx->stream));
  int* dinfo = reinterpret_cast<int*>(dws);
  int rc = IPMZ_OK, info = 0;
  unsigned err = 0;
  const hipError_t e = grid ? bk_factor_grid(A, ld, N, ipiv, dinfo, fix_kp, dws + 256, ctx->stream)
                            : bk_factor(A, ld, N, ipiv, dinfo, fix_kp, 1, 0, 0, ctx->stream);
  if (e != hipSuccess || hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      (grid && hipMemcpyAsync(&err, bk_grid_err_word(dws + 256, N), 4, hipMemcpyDeviceToHost, ctx->stream) !=
                   hipSuccess) ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    rc = fail(IPMZ_ERR_HIP, "ipmz_bk_factor: launch failed");
  else if (err)
    rc = fail(IPMZ_ERR_HIP, "ipmz_bk_factor: a grid barrier of the whole-device factor timed out; the factor is invalid");
  hipFreeAsync(dws, ctx->stream);
  return rc ? rc : info;
}

int ipmz_bk_solve(ipmz_ctx* ctx, int N, const double* F, int64_t ld, const int* ipiv, double* b) {
  if (!ctx || N < 0 || ld < N) return fail(IPMZ_ERR_INVALID, "ipmz_bk_solve: bad arguments");
  if (N == 0) return IPMZ_OK;  // LinearSolvers.cpp:212-214
  if (!F || !ipiv || !b) return fail(IPMZ_ERR_INVALID, "null pointer");
  HIP_OK(hipSetDevice(ctx->device));
  if (N < IPMZ_BK_GRID_MIN) {
    HIP_OK(bk_solve(F, ld, N, ipiv, b, 1, 0, 0, 0, ctx->stream));
    return IPMZ_OK;
  }
  // large N: the device-wide solve (L' with the interchanges folded in,
  // built here from F into stream-ordered buffers, freed after the solve)
  const int64_t ldp = round_up(N, 64);
  double *lt = nullptr, *lp = nullptr;
  char* wb = nullptr;
  HIP_OK(hipMallocAsync(reinterpret_cast<void**>(&lt), (size_t)N * N * sizeof(double), ctx->stream));
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&lp), (size_t)N * ldp * sizeof(double), ctx->stream);
  if (e == hipSuccess) e = hipMallocAsync(reinterpret_cast<void**>(&wb), (size_t)bk_ws(nullptr, N).total, ctx->stream);
  const BkWs w = bk_ws(wb, N);
  if (e == hipSuccess) e = bk_transpose(F, ld, N, lt, ctx->stream);
  if (e == hipSuccess) e = bk_setup(F, ld, N, ipiv, nullptr, lt, lp, ldp, w, ctx->stream);
  if (e == hipSuccess) e = bk_run(lp, ldp, N, lt, ipiv, w, b, ctx->stream);
  // the error word is read, and the stream drained, before the buffers go
  // (their stream-ordered frees stay pending: nothing waits for them)
  const int rc = e == hipSuccess ? ws_result(ctx->stream, nullptr, nullptr, w.ctrl + SOLVE_ERR_WORD, "ipmz_bk_solve")
                                 : IPMZ_OK;
  if (wb) hipFreeAsync(wb, ctx->stream);
  if (lp) hipFreeAsync(lp, ctx->stream);
  hipFreeAsync(lt, ctx->stream);
  HIP_OK(e);
  return rc;
}

int64_t ipmz_bk_solve_workspace_bytes(ipmz_ctx* ctx, int N) {
  if (!ctx || N < 0) return 0;
  return bk_solve_ws(nullptr, N).total;
}

int ipmz_bk_prepare_solve(ipmz_ctx* ctx, int N, const double* F, int64_t ld, const int* ipiv, void* ws,
                          int64_t ws_bytes) {
  if (!ctx || N < 0 || ld < N) return fail(IPMZ_ERR_INVALID, "ipmz_bk_prepare_solve: bad arguments (ld >= N)");
  if (N == 0) return IPMZ_OK;
  if (!F || !ipiv || !ws) return fail(IPMZ_ERR_INVALID, "ipmz_bk_prepare_solve: null pointer");
  const BkSolveWs w = bk_solve_ws(static_cast<char*>(ws), N);
  if (ws_bytes < w.total)
    return fail(IPMZ_ERR_INVALID, "ipmz_bk_prepare_solve: workspace too small (ipmz_bk_solve_workspace_bytes(N))");
  HIP_OK(hipSetDevice(ctx->device));
  HIP_OK(bk_transpose(F, ld, N, w.LT, ctx->stream));
  HIP_OK(bk_setup(F, ld, N, ipiv, nullptr, w.LT, w.Lp, w.ldp, w.k, ctx->stream));
  return IPMZ_OK;
}

int ipmz_bk_solve_multi(ipmz_ctx* ctx, int N, const double* F, int64_t ld, const int* ipiv, const void* ws, double* B,
                        int64_t ldb, int nrhs) {
  if (!ctx || N < 0 || nrhs < 0 || ld < N || ldb < N || (ldb & 1))
    return fail(IPMZ_ERR_INVALID, "ipmz_bk_solve_multi: bad arguments (nrhs >= 0, ld >= N, ldb >= N and even)");
  if (N == 0 || nrhs == 0) return IPMZ_OK;
  if (!F || !ipiv || !ws || !B) return fail(IPMZ_ERR_INVALID, "ipmz_bk_solve_multi: null pointer");
  if ((uintptr_t)B & 15) return fail(IPMZ_ERR_INVALID, "ipmz_bk_solve_multi: B must be 16-byte aligned");
  HIP_OK(hipSetDevice(ctx->device));
  const BkSolveWs w = bk_solve_ws(static_cast<char*>(const_cast<void*>(ws)), N);
  return bk_multi_impl(ctx, N, F, ld, ipiv, w.LT, w.Lp, w.ldp, w.k, B, ldb, nrhs);
}

// Batches of Bunch-Kaufman systems of one order (one workgroup per matrix) -----
// what the batch entry points share: the order, the count and the strides of F and ipiv
// (even_sA: the prepared solve's rule; the factor reads and writes element by element)
static const char* bk_batch_args(ipmz_ctx* ctx, int N, int batch, int64_t ld, int64_t sA, int64_t sP,
                                 bool even_sA = true) {
  if (!ctx || N < 0 || batch < 0 || ld < N) return "bad arguments (N >= 0, batch >= 0, ld >= N)";
  if (N > IPMZ_BK_NMAX) return "N > 4096 (one workgroup per matrix)";
  if (batch > 65535) return "batch > 65535";
  if ((even_sA && (sA & 1)) || (batch > 1 && (sA < (int64_t)(N - 1) * ld + N || sP < N)))
    return "bad strides (sA even and >= (N - 1) * ld + N, sP >= N)";
  return nullptr;
}

int ipmz_bk_factor_batch(ipmz_ctx* ctx, int N, int batch, double* A, int64_t ld, int64_t sA, int* ipiv, int64_t sP,
                         int fix_kp, int* info) {
  if (const char* why = bk_batch_args(ctx, N, batch, ld, sA, sP, false))
    return fail(IPMZ_ERR_INVALID, std::string("ipmz_bk_factor_batch: ") + why);
  if (batch == 0) return IPMZ_OK;
  if (N == 0) {
    if (info) std::memset(info, 0, (size_t)batch * sizeof(int));
    return IPMZ_OK;
  }
  if (!A || !ipiv) return fail(IPMZ_ERR_INVALID, "ipmz_bk_factor_batch: null pointer");
  HIP_OK(hipSetDevice(ctx->device));
  int* dinfo = nullptr;
  HIP_OK(hipMallocAsync(reinterpret_cast<void**>(&dinfo), (size_t)batch * sizeof(int), ctx->stream));
  int rc;
  const hipError_t e = bk_factor(A, ld, N, ipiv, dinfo, fix_kp, batch, sA, sP, ctx->stream);
  if (e != hipSuccess) rc = hip_fail(e, "bk_factor", __FILE__, __LINE__);
  else rc = bk_batch_info(ctx->stream, dinfo, batch, info);
  hipFreeAsync(dinfo, ctx->stream);
  return rc;
}

int64_t ipmz_bk_batch_solve_workspace_bytes(ipmz_ctx* ctx, int N, int batch) {
  if (!ctx || N < 0 || batch < 0 || N > IPMZ_BK_NMAX) return 0;
  return bk_batch_ws(nullptr, N, batch).total;
}

int ipmz_bk_prepare_solve_batch(ipmz_ctx* ctx, int N, int batch, const double* F, int64_t ld, int64_t sA,
                                const int* ipiv, int64_t sP, void* ws, int64_t ws_bytes) {
  if (const char* why = bk_batch_args(ctx, N, batch, ld, sA, sP))
    return fail(IPMZ_ERR_INVALID, std::string("ipmz_bk_prepare_solve_batch: ") + why);
  if (N == 0 || batch == 0) return IPMZ_OK;
  if (!F || !ipiv || !ws) return fail(IPMZ_ERR_INVALID, "ipmz_bk_prepare_solve_batch: null pointer");
  const BkBatchWs w = bk_batch_ws(static_cast<char*>(ws), N, batch);
  if (ws_bytes < w.total)
    return fail(IPMZ_ERR_INVALID,
                "ipmz_bk_prepare_solve_batch: workspace too small (ipmz_bk_batch_solve_workspace_bytes(N, batch))");
  HIP_OK(hipSetDevice(ctx->device));
  return bk_batch_prepare(ctx, N, batch, F, ld, sA, ipiv, sP, nullptr, w);
}

int ipmz_bk_solve_multi_batch(ipmz_ctx* ctx, int N, int batch, const double* F, int64_t ld, int64_t sA,
                              const int* ipiv, int64_t sP, const void* ws, double* B, int64_t ldb, int64_t sB,
                              int nrhs) {
  if (const char* why = bk_batch_args(ctx, N, batch, ld, sA, sP))
    return fail(IPMZ_ERR_INVALID, std::string("ipmz_bk_solve_multi_batch: ") + why);
  if (nrhs < 0 || ldb < N || (ldb & 1) || sB < (int64_t)nrhs * ldb || (sB & 1))
    return fail(IPMZ_ERR_INVALID, "ipmz_bk_solve_multi_batch: bad arguments (nrhs >= 0, ldb >= N and even, sB >= "
                                  "nrhs * ldb and even)");
  if (N == 0 || batch == 0 || nrhs == 0) return IPMZ_OK;
  if (!F || !ipiv || !ws || !B) return fail(IPMZ_ERR_INVALID, "ipmz_bk_solve_multi_batch: null pointer");
  if ((uintptr_t)B & 15) return fail(IPMZ_ERR_INVALID, "ipmz_bk_solve_multi_batch: B must be 16-byte aligned");
  HIP_OK(hipSetDevice(ctx->device));
  const BkBatchWs w = bk_batch_ws(static_cast<char*>(const_cast<void*>(ws)), N, batch);
  return bk_batch_multi_impl(ctx, N, batch, F, ld, sA, ipiv, sP, w, B, ldb, sB, nrhs);
}

// Host adapters with the reference's signatures ------------------------------
int ipmz_symmetric_indefinite_factorization(ipmz_ctx* ctx, int N, const double* A, double* F, int* ipiv) {
  if (!ctx || N < 0 || (N > 0 && (!A || !F || !ipiv)))
    return fail(IPMZ_ERR_INVALID, "ipmz_symmetric_indefinite_factorization: bad arguments");
  if (N == 0) return IPMZ_OK;
  HIP_OK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t nn = (int64_t)N * N;
  DevBuf<double> dA;
  DevBuf<int> dp;
  if (!dA.alloc(nn) || !dp.alloc(N)) return fail(IPMZ_ERR_NOMEM, "device allocation failed");
  if (!rows_in(dA.p, nn, A, nn, 1, st)) return fail(IPMZ_ERR_HIP, "copy-in failed");
  const int rc = ipmz_bk_factor(ctx, N, dA, N, dp, 0);
  if (rc < 0) return rc;
  if (!rows_out(F, dA.p, nn, nn, 1, st) || !rows_out(ipiv, dp.p, N, N, 1, st) || hipStreamSynchronize(st) != hipSuccess)
    return fail(IPMZ_ERR_HIP, "copy-out failed");
  return IPMZ_OK;  // the reference reports no info
}

int ipmz_overwriting_solve_bunch_kaufman(ipmz_ctx* ctx, int N, const double* F, const int* ipiv, double* b) {
  if (!ctx || N < 0) return fail(IPMZ_ERR_INVALID, "ipmz_overwriting_solve_bunch_kaufman: bad arguments");
  if (N == 0) return IPMZ_OK;
  if (!F || !ipiv || !b) return fail(IPMZ_ERR_INVALID, "null pointer");
  HIP_OK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t nn = (int64_t)N * N;
  DevBuf<double> dF, db;
  DevBuf<int> dp;
  if (!dF.alloc(nn) || !db.alloc(N) || !dp.alloc(N)) return fail(IPMZ_ERR_NOMEM, "device allocation failed");
  if (!rows_in(dF.p, nn, F, nn, 1, st) || !rows_in(db.p, N, b, N, 1, st) || !rows_in(dp.p, N, ipiv, N, 1, st))
    return fail(IPMZ_ERR_HIP, "copy-in failed");
  const int rc = ipmz_bk_solve(ctx, N, dF, N, dp, db);
  if (rc) return rc;
  if (!rows_out(b, db.p, N, N, 1, st) || hipStreamSynchronize(st) != hipSuccess)
    return fail(IPMZ_ERR_HIP, "copy-out failed");
  return IPMZ_OK;
}

int ipmz_overwriting_solve_bunch_kaufman_multi(ipmz_ctx* ctx, int N, const double* F, const int* ipiv, double* B,
                                               int nrhs) {
  if (!ctx || N < 0 || nrhs < 0)
    return fail(IPMZ_ERR_INVALID, "ipmz_overwriting_solve_bunch_kaufman_multi: bad arguments");
  if (N == 0 || nrhs == 0) return IPMZ_OK;
  if (!F || !ipiv || !B) return fail(IPMZ_ERR_INVALID, "null pointer");
  HIP_OK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t nn = (int64_t)N * N, ldb = round_up(N, 2);
  const int64_t wsb = bk_solve_ws(nullptr, N).total;
  DevBuf<double> dF, dB;
  DevBuf<int> dp;
  DevBuf<char> ws;
  if (!dF.alloc(nn) || !dB.alloc(ldb * nrhs) || !dp.alloc(N) || !ws.alloc(wsb))
    return fail(IPMZ_ERR_NOMEM, "device allocation failed");
  if (!rows_in(dF.p, nn, F, nn, 1, st) || !rows_in(dB.p, ldb, B, N, nrhs, st) || !rows_in(dp.p, N, ipiv, N, 1, st))
    return fail(IPMZ_ERR_HIP, "copy-in failed");
  int rc = ipmz_bk_prepare_solve(ctx, N, dF, N, dp, ws, wsb);
  if (!rc) rc = ipmz_bk_solve_multi(ctx, N, dF, N, dp, ws, dB, ldb, nrhs);
  // ws is freed on return: check the solve's error word now, not at a later sync
  unwatch(ctx);
  if (!rc)
    rc = ws_result(st, nullptr, nullptr, bk_solve_ws(ws, N).k.ctrl + SOLVE_ERR_WORD,
                   "ipmz_overwriting_solve_bunch_kaufman_multi");
  if (rc) return rc;
  if (!rows_out(B, dB.p, ldb, N, nrhs, st) || hipStreamSynchronize(st) != hipSuccess)
    return fail(IPMZ_ERR_HIP, "copy-out failed");
  return IPMZ_OK;
}

int ipmz_ldlt_decomposition(ipmz_ctx* ctx, int N, const double* A, double* L, double* D) {
  if (!ctx || N < 0 || (N > 0 && (!A || !L || !D))) return fail(IPMZ_ERR_INVALID, "ipmz_ldlt_decomposition: bad arguments");
  if (N == 0) return IPMZ_OK;
  HIP_OK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t ld = round_up(N, 64);
  const int nbo = nbo_for(ctx, N);
  DevBuf<double> dK, dD;
  DevBuf<char> ws;
  HIP_OK(hipMalloc(&dK.p, (size_t)(ld * N * 8)));
  if (!dD.alloc(N) || !ws.alloc(ldlt_ws(nullptr, N, nbo, ctx->nbi).total))
    return fail(IPMZ_ERR_NOMEM, "device allocation failed");
  const LdltWs w = ldlt_ws(ws, N, nbo, ctx->nbi);
  if (!rows_in(dK.p, ld, A, N, N, st)) return fail(IPMZ_ERR_HIP, "copy-in failed");
  const int rc = factor_impl(ctx, N, dK, ld, dD, w, nbo, nullptr);
  if (rc) return rc;
  const int info = read_info(ctx, w);
  if (info < 0) return info;
  if (!rows_out(L, dK.p, ld, N, N, st) || !rows_out(D, dD.p, N, N, 1, st) || hipStreamSynchronize(st) != hipSuccess)
    return fail(IPMZ_ERR_HIP, "copy-out failed");
  // the reference returns a full L: zeros above, ones on the diagonal (LinearSolvers.cpp:18, :38)
  for (int i = 0; i < N; ++i) {
    L[(int64_t)i * N + i] = 1.0;
    for (int j = i + 1; j < N; ++j) L[(int64_t)i * N + j] = 0.0;
  }
  return info;
}

// the two overwriting_solve_ldlt adapters.  multi: the nrhs rows of B (dense
// on the host) through ipmz_ldlt_solve_multi; else B is the one vector of
// ipmz_ldlt_solve
static int overwriting_solve_ldlt(ipmz_ctx* ctx, int N, const double* L, const double* D, double* B, int nrhs,
                                  bool multi, const char* who) {
  if (!ctx || N < 0 || nrhs < 0) return fail(IPMZ_ERR_INVALID, std::string(who) + ": bad arguments");
  if (N == 0 || nrhs == 0) return IPMZ_OK;  // LinearSolvers.cpp:46-48
  if (!L || !D || !B) return fail(IPMZ_ERR_INVALID, "null pointer");
  HIP_OK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t ld = round_up(N, 64), ldb = multi ? round_up(N, 2) : N;
  const int nbo = nbo_for(ctx, N);
  const int64_t wsb = ldlt_ws(nullptr, N, nbo, ctx->nbi).total;
  DevBuf<double> dL, dD, dB;
  DevBuf<char> ws;
  if (!dL.alloc(ld * N) || !dD.alloc(N) || !dB.alloc(ldb * nrhs) || !ws.alloc(wsb))
    return fail(IPMZ_ERR_NOMEM, "device allocation failed");
  if (!rows_in(dL.p, ld, L, N, N, st) || !rows_in(dD.p, N, D, N, 1, st) || !rows_in(dB.p, ldb, B, N, nrhs, st))
    return fail(IPMZ_ERR_HIP, "copy-in failed");
  int rc = ipmz_ldlt_prepare_solve(ctx, N, dL, ld, ws, wsb);
  if (!rc) rc = multi ? ipmz_ldlt_solve_multi(ctx, N, dL, ld, dD, ws, dB, ldb, nrhs)
                      : ipmz_ldlt_solve(ctx, N, dL, ld, dD, ws, dB);
  // ws is freed on return: check the solve's error words now, not at a later sync
  unwatch(ctx);
  const LdltWs w = ldlt_ws(ws, N, nbo, ctx->nbi);
  if (!rc) rc = ws_result(st, nullptr, w.pctrl + PANEL_ERR_WORD, w.ctrl + SOLVE_ERR_WORD, who);
  if (rc) return rc;
  if (!rows_out(B, dB.p, ldb, N, nrhs, st) || hipStreamSynchronize(st) != hipSuccess)
    return fail(IPMZ_ERR_HIP, "copy-out failed");
  return IPMZ_OK;
}

int ipmz_overwriting_solve_ldlt(ipmz_ctx* ctx, int N, const double* L, const double* D, double* b) {
  return overwriting_solve_ldlt(ctx, N, L, D, b, 1, false, "ipmz_overwriting_solve_ldlt");
}

int ipmz_overwriting_solve_ldlt_multi(ipmz_ctx* ctx, int N, const double* L, const double* D, double* B, int nrhs) {
  return overwriting_solve_ldlt(ctx, N, L, D, B, nrhs, true, "ipmz_overwriting_solve_ldlt_multi");
}

}  // extern "C"
