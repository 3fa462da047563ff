// What capi.cpp (contexts, workspaces, the LinearSolvers entry points) and
// qp.cpp (the Newton-step solver object) share.  Internal to libipmz.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "ipmz.h"
#include "kernels.h"

using namespace ipmz;

// the host layer's own functions and data stay inside libipmz.so: only the
// C ABI of ipmz.h is exported
#pragma GCC visibility push(hidden)

// sets ipmz_last_error (one thread_local string, capi.cpp) and returns code
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* expr, const char* file, int line);
#define HIP_OK(expr)                                                           \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) return hip_fail(_e, #expr, __FILE__, __LINE__);      \
  } while (0)

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct ipmz_ctx {
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  int nbo = 0, nbi = 64;  // nbo 0: by matrix order (nbo_for)
  // factorization look-ahead: the panel chain on `stream` itself, panel rows
  // on sC (high priority), trailing updates on sB, the fp32 factor's
  // look-ahead strips on sD; forked from / joined to `stream` (ldlt_factor)
  hipStream_t sB = nullptr, sC = nullptr, sD = nullptr;
  std::vector<hipEvent_t> evpool;
  // the sticky error words (spin timeouts of the persistent kernels) of the
  // workspace the last asynchronous device-memory solve used, resolved when
  // it was enqueued (watch): ipmz_ctx_sync checks and clears them (the caller
  // keeps that workspace alive until then)
  const unsigned* check_pe = nullptr;
  const unsigned* check_se = nullptr;
  // solvers created on this context and not yet destroyed: a context
  // destroyed before them (e.g. a garbage collector finalizing both in either
  // order) is only marked, and freed with the last of them.  Both fields are
  // read and written only under g_ctx_mutex (ctypes drops the GIL around
  // every call, and finalizers run on any thread).
  int users = 0;
  bool closed = false;
};
extern std::mutex g_ctx_mutex;
void ctx_free(ipmz_ctx* ctx);

// outer panel width for an order-N factor: the context's, or by size --
// 512 for N > 4096 (kbench factor, N = 11264: 12.95 ms at 384, 12.34 at
// 512; N = 16384: 32.1 -> 31.2 ms), 384 for 2048 <= N <= 4096 (C2, N = 2560,
// chain-bound: 679-689 steps/s at 512, 711-718 at 384 in round 5,
// profiles/r05_s/c2_nbo_ab.txt; 256: 675), 256 below.  Every workspace
// layout and every factor / solve of an order-N matrix uses this same value.
inline int nbo_for(const ipmz_ctx* ctx, int N) {
  if (ctx->nbo > 0) return ctx->nbo;
  if (ctx->nbi != 64 || N < 2048) return 256;
  return N <= 4096 ? 384 : 512;
}

// Workspaces (DESIGN.md "Workspaces") -----------------------------------------
// The fp64 LDL^T factor + solve of one order-N matrix.  W is triple-buffered
// (look-ahead); y, z, ctrl are the persistent solve's state, P its per-block
// operators (nbi 64 only: nbi 128 solves by the block-step kernel chain and
// has no such region).  Sticky error words: pctrl[PANEL_ERR_WORD],
// ctrl[SOLVE_ERR_WORD].
struct LdltWs {
  int* info = nullptr;  // first non-finite pivot (256 B)
  unsigned* pctrl = nullptr;
  double *side = nullptr, *Linv = nullptr, *W = nullptr, *y = nullptr, *z = nullptr;
  unsigned* ctrl = nullptr;  // (256 B)
  double* P = nullptr;
  int64_t total = 0;
};
inline LdltWs ldlt_ws(char* base, int N, int nbo, int nbi) {
  LdltWs w;
  Carver c{base};
  w.info = c.take<int>(64);
  w.pctrl = c.take<unsigned>(panel_ctrl_words(N, nbo));
  w.side = c.take<double>(2 * nbi);
  w.Linv = c.take<double>((int64_t)((N + nbi - 1) / nbi) * nbi * nbi);
  w.W = c.take<double>(3 * (int64_t)N * nbo);
  w.y = c.take<double>(solve_vec_elems(N));
  w.z = c.take<double>(solve_vec_elems(N));
  w.ctrl = c.take<unsigned>(64);
  if (nbi == 64) w.P = c.take<double>(solve_prep_elems(N));
  w.total = c.off;
  return w;
}
// The normal equations: the definiteness info word (256 B), then the order
// N = n + mp LDL^T
struct NormalWs {
  int* info = nullptr;
  LdltWs k;
  int64_t total = 0;
};
inline NormalWs normal_ws(char* base, int N, int nbo, int nbi) {
  NormalWs w;
  Carver c{base};
  w.info = c.take<int>(64);
  w.k = ldlt_ws(base ? base + c.off : nullptr, N, nbo, nbi);
  w.total = c.off + w.k.total;
  return w;
}
// The device-wide Bunch-Kaufman solve (bk.hip bk_fast_*): the persistent
// triangular solve's operators for L' (64 x 64 inverse diagonal blocks, the
// 128-row-block prep), its y / x vectors and ctrl words (sticky error word
// ctrl[SOLVE_ERR_WORD]), and the interchange bookkeeping (meta)
struct BkWs {
  double *Linv = nullptr, *P = nullptr, *y = nullptr, *x = nullptr;
  unsigned* ctrl = nullptr;
  char* meta = nullptr;
  int64_t total = 0;
};
inline BkWs bk_ws(char* base, int N) {
  BkWs w;
  Carver c{base};
  w.Linv = c.take<double>((int64_t)((N + 63) / 64) * 64 * 64);
  w.P = c.take<double>(solve_prep_elems(N));
  w.y = c.take<double>(solve_vec_elems(N));
  w.x = c.take<double>(solve_vec_elems(N));
  w.ctrl = c.take<unsigned>(64);
  w.meta = c.take<char>((int64_t)bk_fast_meta_bytes(N));
  w.total = c.off;
  return w;
}
// A prepared Bunch-Kaufman solve (ipmz_bk_prepare_solve, once per factor):
// the factor transposed (LT, N x N: the interchange folding's input and the
// fallback's factor), L' (N x ldp, ldp = round_up(N, 64)) and the device-wide
// solve's workspace above
struct BkSolveWs {
  double *LT = nullptr, *Lp = nullptr;
  int64_t ldp = 0;
  BkWs k;
  int64_t total = 0;
};
inline BkSolveWs bk_solve_ws(char* base, int N) {
  BkSolveWs w;
  Carver c{base};
  w.ldp = round_up(N, 64);
  w.LT = c.take<double>((int64_t)N * N);
  w.Lp = c.take<double>((int64_t)N * w.ldp);
  w.k = bk_ws(base ? base + c.off : nullptr, N);
  w.total = c.off + w.k.total;
  return w;
}
// The prepared solve of a batch of Bunch-Kaufman factors of one order
// (ipmz_bk_prepare_solve_batch): per system the factor transposed (LT, N x N),
// L' (N x ldp), the 64 x 64 inverse diagonal blocks of L' and the interchange
// bookkeeping with the system's fallback flag -- member by member, each an
// array over the batch (strides sLT, sLp, sLinv elements, sM bytes).  No
// persistent-solve operators: no batched path uses the persistent sweeps.
struct BkBatchWs {
  double *LT = nullptr, *Lp = nullptr, *Linv = nullptr;
  char* meta = nullptr;
  int64_t ldp = 0, sLT = 0, sLp = 0, sLinv = 0, sM = 0;
  int64_t total = 0;
};
inline BkBatchWs bk_batch_ws(char* base, int N, int batch) {
  BkBatchWs w;
  Carver c{base};
  w.ldp = round_up(N, 64);
  w.sLT = round_up((int64_t)N * N, 32);
  w.sLp = (int64_t)N * w.ldp;
  w.sLinv = (int64_t)((N + 63) / 64) * 64 * 64;
  w.sM = (int64_t)bk_fast_meta_bytes(N);
  w.LT = c.take<double>(w.sLT * batch);
  w.Lp = c.take<double>(w.sLp * batch);
  w.Linv = c.take<double>(w.sLinv * batch);
  w.meta = c.take<char>(w.sM * batch);
  w.total = c.off;
  return w;
}

// ipmz_batch_data_vjp's and ipmz_batch_data_vjp_multi's shared matrix blocks:
// the chunks' partial products of one slab of cotangent rows (grad.hip; elems =
// qp_grad_part_elems of the batch and the call's row count)
struct VjpWs {
  double* part = nullptr;
  int64_t total = 0;
};
inline VjpWs vjp_ws(char* base, int64_t elems) {
  VjpWs w;
  Carver c{base};
  w.part = c.take<double>(elems);
  w.total = c.off;
  return w;
}

// ipmz_batch_data_jvp's matrix products: one segment per row (q, t)
// (jvp.hip; elems = batch * ntan * qp_jvp_plan(...).seg)
struct JvpWs {
  double* prod = nullptr;
  int64_t total = 0;
};
inline JvpWs jvp_ws(char* base, int64_t elems) {
  JvpWs w;
  Carver c{base};
  w.prod = c.take<double>(elems);
  w.total = c.off;
  return w;
}

// ipmz_batch_center's state on the device (kernels.h CenterWs): a few doubles and two ints per QP
inline CenterWs center_ws(char* base, int batch, int nb) {
  CenterWs w;
  Carver c{base};
  w.part = c.take<double>((int64_t)batch * nb);
  w.e = c.take<double>(batch);
  w.alpha = c.take<double>(batch);
  w.sum = c.take<double>(2);
  w.frozen = c.take<int>(batch);
  w.iters = c.take<int>(batch);
  w.nb = nb;
  w.total = c.off;
  return w;
}

// the workspace whose sticky error words the next ipmz_ctx_sync checks (pe:
// a panel factor's, may be null; se: a persistent solve's)
inline void watch(ipmz_ctx* ctx, const unsigned* pe, const unsigned* se) {
  ctx->check_pe = pe;
  ctx->check_se = se;
}
inline void watch(ipmz_ctx* ctx, const LdltWs& w) { watch(ctx, w.pctrl + PANEL_ERR_WORD, w.ctrl + SOLVE_ERR_WORD); }
inline void watch(ipmz_ctx* ctx, const BkWs& w) { watch(ctx, nullptr, w.ctrl + SOLVE_ERR_WORD); }
inline void unwatch(ipmz_ctx* ctx) { ctx->check_pe = ctx->check_se = nullptr; }

// How a multi-right-hand-side solve serves nrhs rows: looped single-vector solves below the path's crossover, from
// it on the blocked solve in column panels of the path's default width.  Debug bits (kernels.h) force the blocked
// solve (IPMZ_DEBUG_MULTI_BLOCKED) or a panel width (_W512, _W128).  The kinds differ on purpose:
//   Ldlt   one system, LDL^T (fp64, normal equations, mixed): MULTI_BLOCKED at any row count; both width bits: 512
//   Bk     one system, Bunch-Kaufman: MULTI_BLOCKED from 2 rows on (one row stays ipmz_bk_solve's launches); both: 512
//   Batch  a batch, either factor: MULTI_BLOCKED from 2 rows on; the one-launch solve where it is eligible and no
//          width is forced; both width bits: the panel chain at the default width (tools/batch_multi_bench.py)
enum class MultiKind { Ldlt, Bk, Batch };
struct MultiPlan {
  bool blocked;  // false: nrhs looped single-vector solves
  int width;     // the blocked solve's panel width
  bool fused;    // blocked, and the one-launch solve may be taken where eligible
};
constexpr MultiPlan multi_plan(int nrhs, int crossover, int panel, int dbg, MultiKind kind) {
  const bool w512 = dbg & IPMZ_DEBUG_MULTI_W512, w128 = dbg & IPMZ_DEBUG_MULTI_W128;
  const bool batch = kind == MultiKind::Batch;
  const bool blocked =
      nrhs >= crossover || ((dbg & IPMZ_DEBUG_MULTI_BLOCKED) && (kind == MultiKind::Ldlt || nrhs >= 2));
  return {blocked, batch && w512 && w128 ? panel : w512 ? 512 : w128 ? 128 : panel, blocked && batch && !w512 && !w128};
}
// Pinned for all eight combinations of the three bits at 1, 2, crossover - 1 and crossover rows (crossover 10,
// default panel 256).  forced: the counts that MULTI_BLOCKED runs blocked (a bit per count, lowest: 1 row); the
// widths with no width bit, W512, W128 and both; fused: the one-launch solve where blocked and no width bit is set
constexpr bool multi_plan_pins(MultiKind kind, int forced, int w0, int w512, int w128, int wboth, bool fused) {
  const int rows[4] = {1, 2, 9, 10}, width[4] = {w0, w512, w128, wboth};
  for (int m = 0; m < 8; ++m)
    for (int i = 0; i < 4; ++i) {
      const int dbg = (m & 1 ? IPMZ_DEBUG_MULTI_W512 : 0) | (m & 2 ? IPMZ_DEBUG_MULTI_W128 : 0) |
                      (m & 4 ? IPMZ_DEBUG_MULTI_BLOCKED : 0);
      const bool blocked = i == 3 || ((m & 4) && (forced >> i & 1));
      const MultiPlan p = multi_plan(rows[i], 10, 256, dbg, kind);
      if (p.blocked != blocked || p.width != width[m & 3] || p.fused != (blocked && fused && !(m & 3))) return false;
    }
  return true;
}
static_assert(multi_plan_pins(MultiKind::Ldlt, 0b1111, 256, 512, 128, 512, false), "Ldlt: blocked at any count, 512 wins");
static_assert(multi_plan_pins(MultiKind::Bk, 0b1110, 256, 512, 128, 512, false), "Bk: blocked from 2 rows, 512 wins");
static_assert(multi_plan_pins(MultiKind::Batch, 0b1110, 256, 512, 128, 256, true), "Batch: from 2 rows, both = default");

// capi.cpp --------------------------------------------------------------------
// One batch of copies and one synchronize: the sticky error words pe (panel
// factor) and se (persistent solve), then the info word; each may be null.
// A raised error word is IPMZ_ERR_HIP (never success: the results are
// invalid), reported before info, as what + pe_text or what + se_text (the
// two timeout sentences, or a caller's own wording).  Returns info, IPMZ_OK
// when it is unset.
extern const char PANEL_TIMEOUT[], SOLVE_TIMEOUT[];
int ws_result(hipStream_t st, const int* info, const unsigned* pe, const unsigned* se, const char* what,
              const char* pe_text = PANEL_TIMEOUT, const char* se_text = SOLVE_TIMEOUT);
int read_info(ipmz_ctx* ctx, const LdltWs& w);  // ws_result of a factor's whole workspace
// The Newton step's work in the idle edges of a forked factor (run_step;
// DESIGN.md §4 "The factor's idle edges").  rest: the assembly of the columns
// >= nbo, on the trailing stream beside the first panel.  rows > 0 (nbi 64
// only): once the leading `rows` rows of the factor are final, the fourth
// stream prepares their solve operators and runs the forward sweep of b over
// them; `swept` then, and the solve of b is solve_ws_tail.  A factor that does
// not fork runs `rest` first on the step's stream and leaves swept false.
struct StepEdges {
  std::function<hipError_t(hipStream_t)> rest;
  int rows = 0;
  const double* b = nullptr;
  bool swept = false;
};
// the forked factor's chain-bound stretch begins with the first panel that
// leaves an order <= IPMZ_EARLY_CHAIN_MAX_N: the rows final by then, as a
// multiple of the solve's block (0: no GEMM-paced stretch, or no block left
// after it)
int chain_bound_rows(int N, int nbo);
// info2: a caller's own info word, reset in the same launch
int factor_impl(ipmz_ctx* ctx, int N, double* K, int64_t ld, double* D, const LdltWs& w, int nbo, TrailTimer* timer,
                int* info2 = nullptr, StepEdges* edges = nullptr);
// the rest of a solve whose forward sweep over the leading rows ran in the factor (StepEdges::swept)
hipError_t solve_ws_tail(const double* K, int64_t ld, int N, const double* D, const LdltWs& w, double* b, int rows,
                         hipStream_t st);
hipError_t solve_ws(const double* K, int64_t ld, int N, const double* D, const LdltWs& w, int nbi, double* b,
                    hipStream_t st);
int mixed_factor_impl(ipmz_ctx* ctx, const double* K, int64_t ld, MixedWs& w, TrailTimer* timer);
int mixed_multi_impl(ipmz_ctx* ctx, const double* K, int64_t ld, MixedWs& w, const MixedMultiWs& m, double* B,
                     int64_t ldb, int nrhs, double tol, int max_refine, double* stat);
int not_capturing(ipmz_ctx* ctx, const char* who);
int normal_factor_impl(ipmz_ctx* ctx, int n, int mp, double* K, int64_t ld, double* D, const NormalWs& w, int nbo,
                       TrailTimer* timer);
int normal_solve_impl(ipmz_ctx* ctx, int n, int mp, const double* K, int64_t ld, const double* D, const NormalWs& w,
                      double* b);
hipError_t bk_setup(const double* F, int64_t ld, int N, const int* ipiv, const int* info, double* LT, double* Lp,
                    int64_t ldp, const BkWs& w, hipStream_t st);
hipError_t bk_run(const double* Lp, int64_t ldp, int N, const double* LT, const int* ipiv, const BkWs& w, double* b,
                  hipStream_t st);
// the nrhs rows of B <- A^{-1} row from a prepared factor (LT, L' in Lp, w);
// F: the factor itself, read only below IPMZ_BK_GRID_MIN (the one-workgroup
// solve of rows below the crossover).  Asynchronous; arguments checked by the
// caller (ldb even, B 16-byte aligned)
int bk_multi_impl(ipmz_ctx* ctx, int N, const double* F, int64_t ld, const int* ipiv, const double* LT,
                  const double* Lp, int64_t ldp, const BkWs& w, double* B, int64_t ldb, int nrhs);
// the same for a batch of prepared factors (bk_batch_prepare: LT, L', the
// inverse diagonal blocks and the bookkeeping of every system, from the
// factors' F, ipiv and info words -- info may be null).  Asynchronous, stream
// order only; arguments checked by the caller
int bk_batch_prepare(ipmz_ctx* ctx, int N, int batch, const double* F, int64_t ld, int64_t sA, const int* ipiv,
                     int64_t sP, const int* info, const BkBatchWs& w);
int bk_batch_multi_impl(ipmz_ctx* ctx, int N, int batch, const double* F, int64_t ld, int64_t sA, const int* ipiv,
                        int64_t sP, const BkBatchWs& w, double* B, int64_t ldb, int64_t sB, int nrhs);
// copies the batch's device info words to info (host, may be null), synchronizes, returns the smallest non-zero one
int bk_batch_info(hipStream_t st, const int* dinfo, int batch, int* info);

#pragma GCC visibility pop
