// C ABI of libipmz (include/ipmz.h), second half: the Newton-step solver
// object ipmz_qp on the contexts, workspaces and factor / solve paths of
// capi.cpp (shared through capi.h).
//
// Newton-step solver: B QPs with identical dimensions (B = 1 for ipmz_qp_*).
// Every per-QP array lives in one allocation with a per-QP stride; the
// kernels take a device array of QPDev descriptors and index it with
// blockIdx.y, so one launch serves the whole batch.
#include <algorithm>
#include <cmath>

#include "capi.h"

// a device buffer kept for the largest size asked of it so far (grow)
struct GrowBuf {
  char* p = nullptr;
  size_t bytes = 0;
};

struct ipmz_qp {
  ipmz_ctx* ctx = nullptr;
  int n = 0, m = 0, p = 0, N = 0, B = 1;
  int64_t ldn = 0, ldk = 0, state_len = 0;
  double delta = 1e-4;
  std::vector<void*> allocs;
  bool alloc_failed = false;  // sticky: a dev_alloc failed (create_solver checks it once)
  std::vector<QPDev> hq;   // host copies of the descriptors
  QPDev* dq = nullptr;     // device array of B descriptors
  QPBatch qb{};
  // factor storage
  double *K = nullptr, *D = nullptr;
  int64_t sK = 0, sD = 0, sb = 0;
  // batches of small systems (fused phases, LDL^T): the assembled KKT kept
  // across steps (off-diagonal part written once per data load, the diagonal
  // every step); the small factor reads it and writes L to K (strides sK)
  double* K0 = nullptr;
  char* ws = nullptr;      // B == 1: ldlt_ws(N); B > 1: bLinv, bW, binfo below
  double *bLinv = nullptr, *bW = nullptr;  // batched factor workspace (B > 1)
  int* binfo = nullptr;
  int64_t sL = 0, sW = 0;
  bool loaded = false;
  // ipmz_batch_load_device: the data blocks the solver holds for every QP (HELD_* bits; a block this call does not
  // supply must be held), the QPs a host load has filled since the last whole-batch fill, and the device word the
  // bound check answers in
  unsigned held = 0;
  std::vector<char> host_filled;
  int host_filled_count = 0;
  unsigned long long* verdict = nullptr;
  // mixed precision (C5): fp32 factor of S K S + fp64 refinement
  bool mixed = false;
  double ir_tol = 1e-12;
  int ir_max = 10;
  MixedWs mw;
  GrowBuf mws;
  // ipmz_qp_kkt_solve_mixed: the multi-right-hand-side workspace, for the largest nrhs seen
  GrowBuf mmws;
  // ipmz_*_newton_solve_multi / ipmz_*_newton_adjoint_multi: the reduced right-hand sides, B x nrhs x round_up(N, 2)
  // doubles, for the largest nrhs seen
  GrowBuf nmws;
  // ipmz_batch_center: the norm's partials, the centered flags and the update counts (center_ws), on first use
  GrowBuf cws;
  // ipmz_batch_data_vjp(_multi): the shared matrix blocks' partial products (vjp_ws), when one is first asked for,
  // grown for the largest slab of cotangent rows seen
  GrowBuf vjpws;
  // ipmz_batch_data_jvp: the matrix products of every row (jvp_ws), for the largest need seen
  GrowBuf jvpws;
  // normal-equations reduction (C2)
  bool normal = false;
  // EqualityHandling::None: Bunch-Kaufman factor (pivots per QP)
  bool eqnone = false;
  // Path::BkGrid only, allocated together: the whole-device factor's workspace, the factor transposed (N x N: the
  // interchange folding's input, the fallback's factor), the device-wide solve's workspace (bk_ws; L' in K)
  char* bkws = nullptr;
  double* bklt = nullptr;
  char* bkfws = nullptr;
  // ipmz_*_kkt_solve_bk on the other two Bunch-Kaufman paths, on first use: the prepared solve (Path::BkSmall,
  // bk_solve_ws), the batch's prepared solves (Path::BkBatch, bk_batch_ws)
  GrowBuf bkpws;
  unsigned* pflags = nullptr;  // B > 1: the two-workgroup small factor's flags + sticky error word
  int small_kernel = IPMZ_BATCH_FACTOR_AUTO;  // ipmz_batch_set_factor_kernel
  bool eqpen = false;  // EqualityHandling::PenaltyFunction (LDL^T)
  // InequalityHandling / Bounds (which Newton slots exist)
  bool slacks = false, naive = false;
  // EqualityHandling::SlackedSlacks: m, p below are the step's (m + p equality
  // rows run as l = u = d inequalities, p = 0); m_usr, p_usr the data's
  bool eqss = false;
  int m_usr = 0, p_usr = 0;
  bool vlo = true, vup = true, alo = true, aup = true;
  int* ipiv = nullptr;
  int64_t sP = 0;
  GrowBuf nws;  // the normal equations' workspace (normal_ws), when the reduction is first enabled
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  int graph_flags = -1;
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;  // phase boundary events
  hipEvent_t (*tr_pairs)[2] = nullptr;
  // completion of the last multi-stream (eager) step: the next one is not
  // enqueued before it (queue depth 1, see step_impl)
  hipEvent_t step_done = nullptr;
  hipEvent_t step_in = nullptr;  // the caller's stream reached the step (the fork onto ctx->own)
  bool step_pending = false;
  int last_step_graph = 0;  // the last ipmz_qp_step replayed a captured hipGraph
  double* summary = nullptr;  // ipmz_batch_solve_ex: the 3 doubles of its looks at the device, on first use
  int tr_cap = 0;
  double ph_ms[IPMZ_PH_COUNT] = {0};
  double tr_flops = 0.0;
  int64_t tr_launches = 0;
};

namespace {
// Newton variables present per formulation (SymbolicOptimization.cpp
// get_variables_: absent blocks are dropped from the Newton order)
int64_t slot_len(const ipmz_qp* s, int slot) {
  switch (slot) {
    case X: return s->n;
    case LY: return s->vlo ? s->n : 0;
    case LZ: return s->vup ? s->n : 0;
    case Y: return (s->vlo && !s->slacks) ? s->n : 0;
    case Z: return (s->vup && !s->slacks) ? s->n : 0;
    case LA: case S: return s->naive ? 0 : s->m;
    case LG: return s->alo ? s->m : 0;
    case LH: return s->aup ? s->m : 0;
    case G: return (s->alo && !s->slacks) ? s->m : 0;
    case H: return (s->aup && !s->slacks) ? s->m : 0;
    case P: return (s->eqnone || s->eqpen) ? 0 : s->p;
    default: return s->p;
  }
}

// device storage freed with the solver (allocs); a failure is recorded in
// s->alloc_failed and every later call returns nullptr
template <typename T>
T* dev_alloc(ipmz_qp* s, size_t count, bool zero) {
  void* ptr = nullptr;
  if (s->alloc_failed || hipMalloc(&ptr, count * sizeof(T)) != hipSuccess) {
    s->alloc_failed = true;
    return nullptr;
  }
  s->allocs.push_back(ptr);
  if (zero && hipMemset(ptr, 0, count * sizeof(T)) != hipSuccess) s->alloc_failed = true;
  return static_cast<T*>(ptr);
}
// one allocation of B x stride doubles (stride = per-QP count rounded to 64 B)
double* dev_array(ipmz_qp* s, int64_t count, int64_t* stride_out = nullptr, bool zero = false) {
  const int64_t stride = round_up(count < 1 ? 1 : count, 8);
  if (stride_out) *stride_out = stride;
  return dev_alloc<double>(s, (size_t)(stride * s->B), zero);
}

// b holds at least `bytes`: kept, or freed and allocated anew (the caller has synchronized whatever may still
// read it).  A failure is IPMZ_ERR_NOMEM and leaves b empty and the solver usable: the next call tries again
int grow(ipmz_qp* s, GrowBuf& b, size_t bytes, bool zero = false) {
  if (bytes <= b.bytes) return IPMZ_OK;
  if (b.p) {
    s->allocs.erase(std::find(s->allocs.begin(), s->allocs.end(), static_cast<void*>(b.p)));
    hipFree(b.p);
  }
  b = GrowBuf{dev_alloc<char>(s, bytes, zero), bytes};
  if (!s->alloc_failed) return IPMZ_OK;
  b = GrowBuf{};
  s->alloc_failed = false;  // (create_solver's flag)
  (void)hipGetLastError();
  return fail(IPMZ_ERR_NOMEM, "device allocation failed");
}

// grow() for a call that only enqueues and so may run inside a caller's graph capture, where nothing can be
// allocated: IPMZ_ERR_STATE then, `why` ending the message.  (Launches of earlier calls may still read the old
// buffer: hipFree waits for the device.)
int grow_unless_capturing(ipmz_qp* s, GrowBuf& b, size_t need, const std::string& who, const char* why) {
  if (need <= b.bytes) return IPMZ_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIP_OK(hipStreamIsCapturing(s->ctx->stream, &cs));
  if (cs != hipStreamCaptureStatusNone)
    return fail(IPMZ_ERR_STATE, who + ": the context's stream is capturing a hipGraph and " + why);
  return grow(s, b, need);
}

// The calls that serve the augmented fp64 systems in the Newton order only (newton_multi, ipmz_batch_data_vjp,
// ipmz_batch_data_jvp) refuse everything else first, in this order
int refuse_unless_newton_order(const ipmz_qp* s, const std::string& who) {
  if (s->normal) return fail(IPMZ_ERR_INVALID, who + ": the normal-equations reduction is enabled (augmented system only)");
  if (s->mixed) return fail(IPMZ_ERR_INVALID, who + ": mixed precision is enabled (fp64 factors only)");
  if (s->eqss)
    return fail(IPMZ_ERR_INVALID, who + ": EqualityHandling::SlackedSlacks / NaiveSlacks keep a permuted, merged view of "
                                        "the Newton order on the device; not served");
  if (!s->loaded) return fail(IPMZ_ERR_STATE, who + ": load (and initialize) the QP first");
  return IPMZ_OK;
}

// A caller's ipmz_qp_device_data (ipmz_qp_device_grad has its layout; tq: ipmz_qp_device_tangent's strides in the
// table's order, or null) as the kernels' descriptor.  dims: n, m, p as the call counts them -- the load the data's
// rows (m_usr, p_usr), the other two the step's.  Blocks of dimension 0 are ignored whatever they hold.
static_assert(sizeof(ipmz_qp_device_grad) == sizeof(ipmz_qp_device_data), "one layout");
template <class T>
QpBlocks<T> data_blocks(const ipmz_qp_device_data& d, const int64_t* tq, const int (&dims)[3]) {
  const double* const ptr[DB_COUNT] = {d.Q, d.A, d.C, d.c, d.l_x, d.u_x, d.l_A, d.u_A, d.d};
  const int64_t ld[DB_MATS] = {d.ldq, d.lda, d.ldc};
  const int64_t sq[DB_COUNT] = {d.sQ, d.sA, d.sC, d.sc, d.slx, d.sux, d.slA, d.suA, d.sd};
  QpBlocks<T> b{};
  for (int k = 0; k < DB_COUNT; ++k) {
    if (!dims[DATA_BLOCKS[k].dim]) continue;
    b.p[k] = const_cast<T*>(ptr[k]);
    if (k < DB_MATS) b.ld[k] = ld[k];
    b.sq[k] = sq[k];
    if (tq) b.tq[k] = tq[k];
  }
  return b;
}

// What differs between the three calls' checks of their blocks -- and nothing else does
struct BlockRules {
  const char* zero_means;  // a QP stride of 0, as the message says it: "shared", "summed over the batch"
  int ntan;                // tangents per QP; < 0: the call has no tangent strides (the load, the gradient)
  bool one_qp_ignores_sq;  // a solver of one QP does not look at its QP strides (the tangents); the load and the
                           // gradient refuse a negative one even there
  bool one_tangent_ignores_tq;  // a call with at most one tangent does not look at its tangent strides
};
struct BlockFacts {
  unsigned supplied;   // the HELD_* bits of the blocks given
  bool shared_matrix;  // a matrix block has QP stride 0 in a batch
};
// Every given block of b in the table's order: the row stride at least n, no negative stride, the tangent stride at
// least the block's extent, the QP stride 0 or at least the extent of the QP's block (of all its tangents)
template <class T>
int check_blocks(const ipmz_qp* s, const std::string& who, const QpBlocks<T>& b, const int (&dims)[3],
                 const BlockRules& r, BlockFacts* facts) {
  const int64_t n = dims[0];
  const bool tangents = r.ntan >= 0, use_tq = tangents && !(r.one_tangent_ignores_tq && r.ntan <= 1);
  *facts = BlockFacts{0, false};
  for (int k = 0; k < DB_COUNT; ++k) {
    if (!b.p[k]) continue;
    const DataBlockInfo& info = DATA_BLOCKS[k];
    const std::string name = who + ": " + info.name;
    facts->supplied |= info.held;
    const int64_t rows = dims[info.dim], ld = info.matrix ? b.ld[k] : rows, sq = b.sq[k], tq = b.tq[k];
    if (info.matrix && ld < n) return fail(IPMZ_ERR_INVALID, name + ": row stride " + std::to_string(ld) + " < n");
    if (ld < 0 || (sq < 0 && !(r.one_qp_ignores_sq && s->B == 1)) || (use_tq && tq < 0))
      return fail(IPMZ_ERR_INVALID, name + ": negative stride");
    const int64_t extent = info.matrix ? (rows - 1) * ld + n : ld;
    if (use_tq && tq < extent)
      return fail(IPMZ_ERR_INVALID, name + ": tangent stride " + std::to_string(tq) +
                                        " is less than the block's extent " + std::to_string(extent));
    const int64_t all = (use_tq ? (int64_t)(r.ntan - 1) * tq : 0) + extent;
    if (s->B > 1 && sq != 0 && sq < all)
      return fail(IPMZ_ERR_INVALID,
                  name + ": QP stride " + std::to_string(sq) + " is neither 0 (" + r.zero_means + ") nor at least " +
                      (tangents ? "the extent of the QP's tangents " : "the block's extent ") + std::to_string(all));
    if (info.matrix && s->B > 1 && sq == 0) facts->shared_matrix = true;
  }
  return IPMZ_OK;
}

void drop_graph(ipmz_qp* s) {
  if (s->gexec) hipGraphExecDestroy(s->gexec);
  if (s->graph) hipGraphDestroy(s->graph);
  s->gexec = nullptr;
  s->graph = nullptr;
}

// slot pointers into one contiguous Newton-order vector (the reference's
// order: slot_in_order, kernels.h)
void carve(const ipmz_qp* s, double* base, double** slots) {
  int64_t off = 0;
  for (int k = 0; k < NSLOT; ++k) {
    const int slot = slot_in_order(s->naive, k);
    slots[slot] = base + off;
    off += slot_len(s, slot);
  }
}

QPDev& q0(ipmz_qp* s) { return s->hq[0]; }

// The factor / solve path a solver runs, from its configuration alone: the fp64 augmented LDL^T of one QP or of a
// batch, the normal-equations reduction, the fp32 factor with fp64 refinement (both B == 1), and
// EqualityHandling::None's Bunch-Kaufman -- B == 1 from IPMZ_BK_GRID_MIN up (whole-device factor, device-wide
// solve) and below it (one workgroup), B > 1 (one workgroup per system)
enum class Path { Ldlt, LdltBatch, Normal, Mixed, BkGrid, BkSmall, BkBatch };
Path path_of(const ipmz_qp* s) {
  if (s->eqnone) return s->B > 1 ? Path::BkBatch : s->N >= IPMZ_BK_GRID_MIN ? Path::BkGrid : Path::BkSmall;
  if (s->normal) return Path::Normal;
  if (s->mixed) return Path::Mixed;
  return s->B == 1 ? Path::Ldlt : Path::LdltBatch;
}

// the solver's own workspaces at the context's current blocking: s->ws
// (Path::Ldlt) and s->nws (Path::Normal, N = n + m + p)
LdltWs ldlt_ws_of(const ipmz_qp* s) { return ldlt_ws(s->ws, s->N, nbo_for(s->ctx, s->N), s->ctx->nbi); }
NormalWs normal_ws_of(const ipmz_qp* s) { return normal_ws(s->nws.p, s->N, nbo_for(s->ctx, s->N), s->ctx->nbi); }

// IPMZ_STEP_SKIP_CONVERGED: the batch's convergence words for the factor and solve kernels (skip false: nobody skips)
size_t scal_pitch(const ipmz_qp* s);
SkipGate skip_gate(const ipmz_qp* s, bool skip) {
  return skip ? SkipGate{s->hq[0].scal + SC_CONVERGED, (int64_t)(scal_pitch(s) / 8)} : SkipGate{};
}
// the batch's strides as the batched LDL^T factor and the blocked solves take them
BatchStrides batch_strides(const ipmz_qp* s, const double* K0, bool skip) {
  return BatchStrides{s->B, s->sK, s->sD, s->sL, s->sW, s->pflags, K0, s->small_kernel, skip_gate(s, skip)};
}
TrsmBatch trsm_batch(const ipmz_qp* s, int64_t sB) { return TrsmBatch{s->B, s->sK, s->sD, s->sL, sB}; }

// skip: the step's IPMZ_STEP_SKIP_CONVERGED (the per-QP batch paths only, can_skip_converged)
int solve_batch(ipmz_qp* s, hipStream_t st, int which, bool skip = false) {
  switch (path_of(s)) {
    case Path::BkGrid:  // overwriting_solve_bunch_kaufman, device-wide (L' in K)
      HIP_OK(bk_run(s->K, s->ldk, s->N, s->bklt, s->ipiv, bk_ws(s->bkfws, s->N), q0(s).b, st));
      break;
    case Path::BkSmall:
    case Path::BkBatch:  // overwriting_solve_bunch_kaufman
      HIP_OK(bk_solve(s->K, s->ldk, s->N, s->ipiv, q0(s).b, s->B, s->sK, s->sP, s->sb, st, skip_gate(s, skip)));
      break;
    case Path::Normal:
      return normal_solve_impl(s->ctx, s->n, s->m + s->p, s->K, s->ldk, s->D, normal_ws_of(s), q0(s).b);
    case Path::Mixed:
      HIP_OK(mixed_solve(s->K, s->ldk, s->mw, q0(s).b, s->ir_tol, s->ir_max, st));
      HIP_OK(hipMemcpyAsync(q0(s).scal + IPMZ_SC_IR_RATIO_AFF + 2 * which, s->mw.stat, 2 * sizeof(double),
                            hipMemcpyDeviceToDevice, st));
      break;
    case Path::Ldlt:
      HIP_OK(solve_ws(s->K, s->ldk, s->N, s->D, ldlt_ws_of(s), s->ctx->nbi, q0(s).b, st));
      break;
    case Path::LdltBatch:
      HIP_OK(ldlt_solve_batched(s->K, s->ldk, s->N, s->D, s->bLinv, s->ctx->nbi, q0(s).b, s->B, s->sK, s->sD, s->sL,
                                s->sb, st, skip_gate(s, skip)));
      break;
  }
  return IPMZ_OK;
}

// info_reset: the caller already reset the batched factor's info word; skip: as solve_batch's (the callers that
// reuse the step's factor -- the kkt, Newton-multi and adjoint solves -- never pass it: they need every QP's)
bool uses_k0(const ipmz_qp* s);
int factor_batch(ipmz_qp* s, TrailTimer* tt, bool info_reset, StepEdges* edges = nullptr, bool skip = false) {
  hipStream_t st = s->ctx->stream;
  const int nbo = nbo_for(s->ctx, s->N);
  switch (path_of(s)) {
    // EqualityHandling::None, zero diagonal block: symmetric_indefinite_factorization (reference kp behaviour)
    case Path::BkGrid:
      HIP_OK(bk_factor_grid(s->K, s->ldk, s->N, s->ipiv, s->binfo, 0, s->bkws, st));
      HIP_OK(bk_transpose(s->K, s->ldk, s->N, s->bklt, st));
      // L' into K (the factor is not read again this step)
      HIP_OK(bk_setup(s->K, s->ldk, s->N, s->ipiv, s->binfo, s->bklt, s->K, s->ldk, bk_ws(s->bkfws, s->N), st));
      return IPMZ_OK;
    case Path::BkSmall:
    case Path::BkBatch:
      HIP_OK(bk_factor(s->K, s->ldk, s->N, s->ipiv, s->binfo, 0, s->B, s->sK, s->sP, st, skip_gate(s, skip)));
      return IPMZ_OK;
    case Path::Mixed: return mixed_factor_impl(s->ctx, s->K, s->ldk, s->mw, tt);
    case Path::Normal:
      return normal_factor_impl(s->ctx, s->n, s->m + s->p, s->K, s->ldk, s->D, normal_ws_of(s), nbo, tt);
    case Path::Ldlt: return factor_impl(s->ctx, s->N, s->K, s->ldk, s->D, ldlt_ws_of(s), nbo, tt, nullptr, edges);
    case Path::LdltBatch: break;
  }
  // (info_reset: the fused step, whose pre phase assembled into K0)
  if (!info_reset) HIP_OK(hipMemsetAsync(s->binfo, 0x7f, sizeof(int), st));
  HIP_OK(ldlt_factor_batched(s->K, s->ldk, s->N, s->D, s->bLinv, s->bW, nbo, s->ctx->nbi, s->binfo, st,
                             batch_strides(s, info_reset && uses_k0(s) ? s->K0 : nullptr, skip)));
  return IPMZ_OK;
}

// batches of small systems: the O(N) / O(n^2) phases as three per-QP
// workgroup kernels (newton.hip k_fused_*)
bool fused_phases(const ipmz_qp* s) { return s->B > 1 && s->N <= IPMZ_FUSED_NMAX; }
// ... whose solves are the small batched solve (solve_batch's last branch,
// nbi 64): then both solves and the phases between them run as one launch
bool fused_solves(const ipmz_qp* s) {
  return fused_phases(s) && path_of(s) == Path::LdltBatch && s->ctx->nbi == 64 && fused_solves_ok(s->N, s->ldk) &&
         !(debug_inject_mask() & IPMZ_DEBUG_NO_FUSED_SOLVES);
}
// the fused step keeps the assembled matrix in K0 when the small batched
// factor (nbi 64) consumes it; otherwise the whole matrix is assembled into K
bool uses_k0(const ipmz_qp* s) {
  return s->K0 && s->ctx->nbi == 64 && s->N <= IPMZ_SMALL_NMAX && !(debug_inject_mask() & IPMZ_DEBUG_NO_K0);
}

// IPMZ_STEP_SKIP_CONVERGED is served where every launch of the step runs whole workgroups per QP: the fused
// small-system step of a batch on the small batched LDL^T factor (inner block 64) or the batched Bunch-Kaufman
bool can_skip_converged(const ipmz_qp* s) {
  const Path path = path_of(s);
  return fused_phases(s) && s->ctx->nbi == 64 && (path == Path::LdltBatch || path == Path::BkBatch);
}

// The single-QP fp64 augmented LDL^T step whose factor forks onto the
// look-ahead streams runs its memory-bound neighbours in the factor's two idle
// edges (DESIGN.md §4 "The factor's idle edges"): the assembly of the columns
// beyond the first panel beside that panel, and -- the affine right-hand side
// moved ahead of the factor -- the solve preparation and forward sweep of the
// rows that are final when the factor turns chain-bound beside its tail.
// IPMZ_DEBUG_SERIAL_EDGES keeps the serial order (bitwise the same step).
bool step_edges(const ipmz_qp* s) {
  const int dbg = debug_inject_mask();
  if (path_of(s) != Path::Ldlt || (dbg & (IPMZ_DEBUG_SERIAL_EDGES | IPMZ_DEBUG_ONE_STREAM))) return false;
  const int nbo = nbo_for(s->ctx, s->N);
  return (s->N + nbo - 1) / nbo >= 3;
}
// rows of the early forward sweep (0: none); debug bits 24-29 force them
int step_edge_rows(const ipmz_qp* s) {
  if (s->ctx->nbi != 64) return 0;
  const int v = (debug_inject_mask() & IPMZ_DEBUG_EDGE_ROWS_MASK) >> IPMZ_DEBUG_EDGE_ROWS_SHIFT;
  const int r = v ? (v - 1) * IPMZ_SOLVE_BLOCK : chain_bound_rows(s->N, nbo_for(s->ctx, s->N));
  return r >= s->N - IPMZ_SOLVE_BLOCK ? 0 : r;
}

int run_step(ipmz_qp* s, int flags) {
  hipStream_t st = s->ctx->stream;
  QPBatch qb = s->qb;  // (a copy: this step's skip flag travels in it)
  const bool t = s->timing;
  auto mark = [&](int i) {
    IPMZ_TRACE("step: phase mark %d", i);
    if (t) hipEventRecord(s->ev[i], st);
  };
  const bool restart = flags & IPMZ_STEP_RESTART_IF_CONVERGED;
  const int freeze = restart ? 0 : 1;
  const bool fused = fused_phases(s);
  const bool skip = flags & IPMZ_STEP_SKIP_CONVERGED;  // (fused: step_impl refused every other step)
  qb.skip = skip;  // (the fused phases' gate; the factor and the solves take theirs below)
  TrailTimer tt;
  tt.pairs = s->tr_pairs;
  tt.cap = t ? s->tr_cap : 0;
  int rc;
  if (fused) {
    // phases: assemble = pre (restart, assembly, affine rhs); factor;
    // solve = the two solves; eval = mid + post
    mark(0);
    HIP_OK(qp_fused_pre(qb, restart ? 1 : 0, s->eqnone ? nullptr : s->binfo, st, uses_k0(s) ? KMODE_K0_DIAG : KMODE_K));
    mark(1);
    if ((rc = factor_batch(s, nullptr, true, nullptr, skip))) return rc;
    mark(2);
    if (fused_solves(s)) {
      // both solves and the phases between them in one launch (the solve
      // phase then holds mid and post too; eval = the evaluation alone)
      HIP_OK(qp_fused_solves(qb, s->K, s->ldk, s->N, s->D, s->bLinv, q0(s).b, s->sK, s->sD, s->sL, s->sb, freeze, st));
      mark(3);
      mark(4);
      mark(5);
      HIP_OK(qp_fused_eval(qb, st));
    } else {
      if ((rc = solve_batch(s, st, 0, skip))) return rc;
      mark(3);
      HIP_OK(qp_fused_mid(qb, st));
      mark(4);
      if ((rc = solve_batch(s, st, 1, skip))) return rc;
      mark(5);
      HIP_OK(qp_fused_post(qb, freeze, st));
    }
    mark(6);
    mark(7);
  } else {
    if (restart) HIP_OK(qp_restart_if_converged(qb, st));
    mark(0);
    StepEdges edges;
    const bool overlap = step_edges(s);
    if (overlap) {
      // the head: what the first panel reads; the rest beside it (phase
      // accounting: inside `factor`), and the affine right-hand side -- from
      // the residuals, which the factor does not touch -- for the early sweep
      const int c_head = nbo_for(s->ctx, s->N);
      HIP_OK(qp_assemble_cols(qb, c_head, true, st));
      mark(1);
      HIP_OK(qp_rhs(qb, st));
      edges.rest = [&qb, c_head](hipStream_t sb) { return qp_assemble_cols(qb, c_head, false, sb); };
      edges.rows = step_edge_rows(s);
      edges.b = q0(s).b;
      IPMZ_TRACE("step: edges, head columns %d, early sweep rows %d", c_head, edges.rows);
    } else {
      HIP_OK(qp_assemble(qb, st));
      mark(1);
    }
    if ((rc = factor_batch(s, t ? &tt : nullptr, false, overlap ? &edges : nullptr))) return rc;
    mark(2);
    // predictor (affine scaling) direction
    if (!overlap) HIP_OK(qp_rhs(qb, st));
    if (edges.swept) {
      IPMZ_TRACE("step: forward sweep from row %d on", edges.rows);
      HIP_OK(solve_ws_tail(s->K, s->ldk, s->N, s->D, ldlt_ws_of(s), q0(s).b, edges.rows, st));
    } else if ((rc = solve_batch(s, st, 0))) {
      return rc;
    }
    mark(3);
    HIP_OK(qp_backsub(qb, 0, st));
    HIP_OK(qp_ratio(qb, 0, SC_ALPHA_AFF, st));
    HIP_OK(qp_mu_aff(qb, st));
    // centering-corrector direction
    HIP_OK(qp_corrector_residuals(qb, st));
    HIP_OK(qp_rhs(qb, st));
    mark(4);
    if ((rc = solve_batch(s, st, 1))) return rc;
    mark(5);
    HIP_OK(qp_backsub(qb, 1, st));
    HIP_OK(qp_ratio(qb, 1, SC_ALPHA, st));
    HIP_OK(qp_update(qb, freeze, st));
    mark(6);
    HIP_OK(qp_evaluate(qb, st));
    mark(7);
  }
  if (t) {
    HIP_OK(hipStreamSynchronize(st));
    float ms = 0.f;
    auto el = [&](int a, int b) {
      hipEventElapsedTime(&ms, s->ev[a], s->ev[b]);
      return (double)ms;
    };
    s->ph_ms[IPMZ_PH_STEP] += el(0, 7);
    s->ph_ms[IPMZ_PH_ASSEMBLE] += el(0, 1);
    s->ph_ms[IPMZ_PH_FACTOR] += el(1, 2);
    s->ph_ms[IPMZ_PH_SOLVE] += el(2, 3) + el(4, 5);
    s->ph_ms[IPMZ_PH_EVAL] += fused ? el(3, 4) + el(5, 6) : el(6, 7);
    for (int i = 0; i < tt.used; ++i) {
      hipEventElapsedTime(&ms, s->tr_pairs[i][0], s->tr_pairs[i][1]);
      s->ph_ms[IPMZ_PH_TRAILING] += ms;
    }
    s->tr_launches += tt.used;
    s->tr_flops += tt.flops * s->B;
  }
  return IPMZ_OK;
}

// the data on the device just changed: a fresh iterate, evaluated and kept as
// the restart snapshot; synchronizes
int initialize(ipmz_qp* s) {
  HIP_OK(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  HIP_OK(qp_init_iterate(s->qb, st));
  if (s->K0) HIP_OK(qp_fused_pre(s->qb, 0, nullptr, st, KMODE_K0_OFFDIAG));
  HIP_OK(qp_evaluate(s->qb, st));
  // the per-QP step count restarts with the scalar block (no step but one with IPMZ_STEP_SKIP_CONVERGED writes it)
  HIP_OK(hipMemset2DAsync(q0(s).scal + SC_STEPS, scal_pitch(s), 0, sizeof(double), (size_t)s->B, st));
  HIP_OK(qp_save_initial(s->qb, st));
  s->loaded = true;
  HIP_OK(hipStreamSynchronize(st));
  return IPMZ_OK;
}

int create_solver(ipmz_ctx* ctx, const ipmz_qp_config* cfg, int B, ipmz_qp** out) {
  if (!ctx || !cfg || !out) return fail(IPMZ_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->n <= 0 || cfg->m < 0 || cfg->p < 0 || B <= 0)
    return fail(IPMZ_ERR_INVALID, "dimensions: n > 0, m >= 0, p >= 0, batch > 0");
  if (cfg->equality_handling != IPMZ_EQ_REGULARIZATION && cfg->equality_handling != IPMZ_EQ_NONE &&
      cfg->equality_handling != IPMZ_EQ_PENALTY && cfg->equality_handling != IPMZ_EQ_PENALTY_EXTRA_DUAL &&
      cfg->equality_handling != IPMZ_EQ_SLACKED_SLACKS && cfg->equality_handling != IPMZ_EQ_NAIVE_SLACKS)
    return fail(IPMZ_ERR_INVALID, "unknown equality handling");
  const int mk = cfg->inequality_handling == IPMZ_INEQ_NAIVE_SLACKS ? 2 * cfg->m : cfg->m;
  if (cfg->equality_handling == IPMZ_EQ_NONE && B > 1 && cfg->n + mk + cfg->p > IPMZ_BK_NMAX)
    return fail(IPMZ_ERR_INVALID, "EqualityHandling::None in batches factors with Bunch-Kaufman one workgroup per "
                                  "system: N <= " + std::to_string(IPMZ_BK_NMAX));
  const int ih = cfg->inequality_handling, ib = cfg->inequality_bounds, vb = cfg->variable_bounds;
  if (ih != IPMZ_INEQ_SLACKED_SLACKS && ih != IPMZ_INEQ_SLACKS && ih != IPMZ_INEQ_NAIVE_SLACKS)
    return fail(IPMZ_ERR_INVALID, "unknown inequality handling");
  if (ih == IPMZ_INEQ_NAIVE_SLACKS && cfg->m > 0 && ib != IPMZ_BOUNDS_BOTH)
    return fail(IPMZ_ERR_INVALID, "InequalityHandling::NaiveSlacks: both inequality bounds");
  if (cfg->equality_handling == IPMZ_EQ_NAIVE_SLACKS && (ih != IPMZ_INEQ_NAIVE_SLACKS || ib != IPMZ_BOUNDS_BOTH))
    return fail(IPMZ_ERR_INVALID, "EqualityHandling::NaiveSlacks: with InequalityHandling::NaiveSlacks and both "
                                  "inequality bounds");
  if (cfg->equality_handling == IPMZ_EQ_SLACKED_SLACKS && (ih != IPMZ_INEQ_SLACKED_SLACKS || ib != IPMZ_BOUNDS_BOTH))
    return fail(IPMZ_ERR_INVALID, "EqualityHandling::SlackedSlacks: with InequalityHandling::SlackedSlacks and both "
                                  "inequality bounds");
  if (ib < IPMZ_BOUNDS_BOTH || ib > IPMZ_BOUNDS_NONE || vb < IPMZ_BOUNDS_BOTH || vb > IPMZ_BOUNDS_NONE)
    return fail(IPMZ_ERR_INVALID, "unknown bounds setting");
  if (cfg->m > 0 && ib == IPMZ_BOUNDS_NONE)
    return fail(IPMZ_ERR_INVALID, "inequality rows need a lower or an upper bound (inequality_bounds != NONE)");
  if (ih == IPMZ_INEQ_SLACKS && ((cfg->m > 0 && ib != IPMZ_BOUNDS_BOTH) || vb != IPMZ_BOUNDS_BOTH))
    return fail(IPMZ_ERR_INVALID, "InequalityHandling::Slacks is built on both bounds (the reference's Slacks "
                                  "formulation drops one-sided bounds inconsistently)");
  HIP_OK(hipSetDevice(ctx->device));
  auto* s = new ipmz_qp();
  s->ctx = ctx;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mutex);
    if (ctx->closed) {
      delete s;
      return fail(IPMZ_ERR_STATE, "context already destroyed");
    }
    ++ctx->users;
  }
  s->B = B;
  s->n = cfg->n;
  s->m_usr = cfg->m;
  s->p_usr = cfg->p;
  // equality SlackedSlacks / NaiveSlacks: the p rows appended to the
  // inequality block of the same handling with l = u = d
  s->eqss = cfg->equality_handling == IPMZ_EQ_SLACKED_SLACKS || cfg->equality_handling == IPMZ_EQ_NAIVE_SLACKS;
  s->m = s->eqss ? cfg->m + cfg->p : cfg->m;
  s->p = s->eqss ? 0 : cfg->p;
  s->N = cfg->equality_handling == IPMZ_EQ_NAIVE_SLACKS ? cfg->n + 2 * (cfg->m + cfg->p) : cfg->n + mk + cfg->p;
  s->delta = cfg->delta > 0 ? cfg->delta : 1e-4;
  s->eqnone = cfg->equality_handling == IPMZ_EQ_NONE;
  s->eqpen = cfg->equality_handling == IPMZ_EQ_PENALTY || cfg->equality_handling == IPMZ_EQ_PENALTY_EXTRA_DUAL;
  s->slacks = ih == IPMZ_INEQ_SLACKS;
  s->naive = ih == IPMZ_INEQ_NAIVE_SLACKS;
  s->vlo = vb == IPMZ_BOUNDS_BOTH || vb == IPMZ_BOUNDS_LOWER;
  s->vup = vb == IPMZ_BOUNDS_BOTH || vb == IPMZ_BOUNDS_UPPER;
  s->alo = ib == IPMZ_BOUNDS_BOTH || ib == IPMZ_BOUNDS_LOWER;
  s->aup = ib == IPMZ_BOUNDS_BOTH || ib == IPMZ_BOUNDS_UPPER;
  s->ldn = round_up(s->n, 8);
  s->ldk = round_up(s->N, 64);
  s->state_len = 0;
  for (int k = 0; k < NSLOT; ++k) s->state_len += slot_len(s, k);
  const int n = s->n, m = s->m, p = s->p, N = s->N;
  int64_t sQ, sA, sC, sn, sm, sp, sS, sNb, sScal, sPart, sT;
  double* Q = dev_array(s, (int64_t)n * s->ldn, &sQ);
  double* A = dev_array(s, (int64_t)m * s->ldn, &sA);
  double* C = dev_array(s, (int64_t)p * s->ldn, &sC);  // (eqss: C is rows m_usr.. of A)
  double* c = dev_array(s, n, &sn);
  double* lx = dev_array(s, n);
  double* ux = dev_array(s, n);
  double* Qx = dev_array(s, n);
  double* ATl = dev_array(s, n);
  double* CTl = dev_array(s, n);
  double* lA = dev_array(s, m, &sm);
  double* uA = dev_array(s, m);
  double* Ax = dev_array(s, m);
  double* d = dev_array(s, s->p_usr, &sp);
  double* Cx = dev_array(s, p);
  double* Cx0 = dev_array(s, p);
  double* v = dev_array(s, s->state_len, &sS);
  double* r = dev_array(s, s->state_len);
  double* da = dev_array(s, s->state_len);
  double* di = dev_array(s, s->state_len);
  double* v0 = dev_array(s, s->state_len);
  double* r0 = dev_array(s, s->state_len);
  double* bvec = dev_array(s, N, &sNb);
  double* scal = dev_array(s, SC_COUNT, &sScal);
  double* scal0 = dev_array(s, SC_COUNT);
  double* part = dev_array(s, 4 * 1024, &sPart);
  double* tpart = dev_array(s, (int64_t)((m > p ? m : p) + IPMZ_TCHUNK - 1) / IPMZ_TCHUNK * n + 8, &sT);
  int64_t sDone;
  double* done = dev_array(s, 1, &sDone, true);
  s->K = dev_array(s, (int64_t)N * s->ldk, &s->sK);
  if (B > 1 && N <= IPMZ_FUSED_NMAX && !s->eqnone) {
    int64_t sK0 = 0;
    s->K0 = dev_array(s, (int64_t)N * s->ldk, &sK0);
  }
  s->D = dev_array(s, N, &s->sD);
  s->sb = sNb;
  if (B == 1) {
    s->ws = dev_alloc<char>(s, (size_t)ldlt_ws(nullptr, N, nbo_for(ctx, N), ctx->nbi).total, true);
  } else {
    const int64_t nblk = (N + ctx->nbi - 1) / ctx->nbi;
    // zeroed once: the wave-specialized small factor writes only the lower
    // triangle of every inverse (the step's single-vector solve reads no
    // more), and no factor writes a nonzero above the diagonal; the blocked
    // multi-right-hand-side solve (ipmz_batch_kkt_solve, trsm.hip) reads whole
    // blocks and needs the zeros there, as a single QP's workspace has them
    s->bLinv = dev_array(s, nblk * ctx->nbi * ctx->nbi, &s->sL, true);
    s->bW = dev_array(s, (int64_t)N * nbo_for(ctx, N), &s->sW);
    s->binfo = dev_alloc<int>(s, B > 64 ? B : 64, false);  // one info per QP
    // flags of the two-workgroup small factor (B <= #CU)
    s->pflags = dev_alloc<unsigned>(s, (size_t)B * IPMZ_PAIR_FLAGS + 1, true);
  }
  if (s->eqnone) {
    s->sP = round_up(N, 16);
    s->ipiv = dev_alloc<int>(s, (size_t)(s->sP * B), false);
    if (!s->binfo) s->binfo = dev_alloc<int>(s, 64, false);
    if (path_of(s) == Path::BkGrid) {
      s->bkws = dev_alloc<char>(s, bk_grid_ws_bytes(N), false);
      s->bklt = dev_alloc<double>(s, (size_t)N * N, false);
      s->bkfws = dev_alloc<char>(s, (size_t)bk_ws(nullptr, N).total, true);
    }
  }
  s->dq = dev_alloc<QPDev>(s, B, false);
  s->verdict = dev_alloc<unsigned long long>(s, 8, false);
  // every failure from here on leaves through ipmz_qp_destroy: it frees what
  // was allocated and gives the context's user count back
  auto bail = [&](int rc) {
    ipmz_qp_destroy(s);
    return rc;
  };
  if (s->alloc_failed) return bail(fail(IPMZ_ERR_NOMEM, "device allocation failed"));
  s->hq.resize(B);
  for (int i = 0; i < B; ++i) {
    QPDev& q = s->hq[i];
    q = QPDev{};
    q.n = n;
    q.m = m;
    q.p = p;
    q.N = N;
    q.ldn = s->ldn;
    q.ldk = s->ldk;
    q.state_len = s->state_len;
    q.delta = s->delta;
    q.eqnone = s->eqnone ? 1 : 0;
    q.eqpen = s->eqpen ? 1 : 0;
    q.slacks = s->slacks ? 1 : 0;
    q.naive = s->naive ? 1 : 0;
    q.eqss = s->eqss ? 1 : 0;
    q.m_usr = s->m_usr;
    q.p_usr = s->p_usr;
    q.mk = s->naive ? 2 * m : m;
    q.vlo = s->vlo ? 1 : 0;
    q.vup = s->vup ? 1 : 0;
    q.alo = s->alo ? 1 : 0;
    q.aup = s->aup ? 1 : 0;
    q.Q = Q + i * sQ;
    q.A = A + i * sA;
    q.C = s->eqss ? q.A + (int64_t)s->m_usr * s->ldn : C + i * sC;
    q.c = c + i * sn;
    q.lx = lx + i * sn;
    q.ux = ux + i * sn;
    q.Qx = Qx + i * sn;
    q.ATl = ATl + i * sn;
    q.CTl = CTl + i * sn;
    q.lA = lA + i * sm;
    q.uA = uA + i * sm;
    q.Ax = Ax + i * sm;
    q.d = d + i * sp;
    q.Cx = Cx + i * sp;
    q.Cx0 = Cx0 + i * sp;
    carve(s, v + i * sS, q.v);
    carve(s, r + i * sS, q.r);
    carve(s, da + i * sS, q.daff);
    carve(s, di + i * sS, q.dir);
    q.v0 = v0 + i * sS;
    q.r0 = r0 + i * sS;
    q.b = bvec + i * sNb;
    q.scal = scal + i * sScal;
    q.scal0 = scal0 + i * sScal;
    q.part = part + i * sPart;
    q.tpart = tpart + i * sT;
    q.K = s->K + i * s->sK;
    q.K0 = s->K0 ? s->K0 + i * s->sK : nullptr;
    q.done = reinterpret_cast<unsigned*>(done + i * sDone);
  }
  s->qb = QPBatch{s->dq, s->hq[0], B};
  hipError_t e = hipMemcpy(s->dq, s->hq.data(), sizeof(QPDev) * B, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(scal, 0, (size_t)sScal * B * 8, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(s->K, 0, (size_t)s->sK * B * 8, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return bail(hip_fail(e, "create_solver: descriptor upload / clear", __FILE__, __LINE__));
  *out = s;
  return IPMZ_OK;
}

int check_index(ipmz_qp* s, int i) {
  if (!s || i < 0 || i >= s->B) return fail(IPMZ_ERR_INVALID, "QP index out of range");
  return IPMZ_OK;
}

int load_one(ipmz_qp* s, int i, const double* Q, const double* c, const double* A, const double* lA, const double* uA,
             const double* C, const double* d, const double* lx, const double* ux) {
  if (!Q || !c || !lx || !ux || (s->m_usr && (!A || !lA || !uA)) || (s->p_usr && (!C || !d)))
    return fail(IPMZ_ERR_INVALID, "load: missing data block");
  // EnvironmentBuilder.cpp:12-17 (the reference ASSERTs; here an error code)
  for (int k = 0; k < s->n; ++k)
    if (!(lx[k] < ux[k])) return fail(IPMZ_ERR_INVALID, "l_x < u_x violated at " + std::to_string(k));
  for (int k = 0; k < s->m_usr; ++k)
    if (!(lA[k] <= uA[k])) return fail(IPMZ_ERR_INVALID, "l_A <= u_A violated at " + std::to_string(k));
  HIP_OK(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  const QPDev& q = s->hq[i];
  const size_t rowb = (size_t)s->n * 8, ldb = (size_t)s->ldn * 8;
  HIP_OK(hipMemcpy2DAsync((void*)q.Q, ldb, Q, rowb, rowb, s->n, hipMemcpyHostToDevice, st));
  if (s->m_usr) HIP_OK(hipMemcpy2DAsync((void*)q.A, ldb, A, rowb, rowb, s->m_usr, hipMemcpyHostToDevice, st));
  if (s->p_usr) HIP_OK(hipMemcpy2DAsync((void*)q.C, ldb, C, rowb, rowb, s->p_usr, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync((void*)q.c, c, rowb, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync((void*)q.lx, lx, rowb, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync((void*)q.ux, ux, rowb, hipMemcpyHostToDevice, st));
  if (s->m_usr) {
    HIP_OK(hipMemcpyAsync((void*)q.lA, lA, (size_t)s->m_usr * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync((void*)q.uA, uA, (size_t)s->m_usr * 8, hipMemcpyHostToDevice, st));
  }
  if (s->p_usr) HIP_OK(hipMemcpyAsync((void*)q.d, d, (size_t)s->p_usr * 8, hipMemcpyHostToDevice, st));
  if (s->eqss && s->p_usr) {  // the equality rows as l = u = d
    HIP_OK(hipMemcpyAsync((void*)(q.lA + s->m_usr), d, (size_t)s->p_usr * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync((void*)(q.uA + s->m_usr), d, (size_t)s->p_usr * 8, hipMemcpyHostToDevice, st));
  }
  HIP_OK(hipStreamSynchronize(st));
  return IPMZ_OK;
}

// Does the step's factorization fork onto the look-ahead streams?  Such a
// step is enqueued eagerly even when IPMZ_STEP_GRAPH is asked for: its graph
// replay is slower than the eager launches (tools/graph_ab.py, profiles/r03_s3:
// C2 2.4-3.0 vs 1.75 ms, C3 16.7 vs 14.6, C5 35.3 vs 25.7 ms per step -- the
// replayed look-ahead loses its stream priorities and overlap), and a
// multi-millisecond step hides its launch latency anyway.  The capture itself
// is correct (debug bit IPMZ_INJECT_GRAPH_FORKS; tests/test_gpu_graph.py:
// bitwise the eager step): it once crashed inside hipStreamEndCapture of the
// HIP runtime torch bundles, fixed by ldlt.hip's stream_record / stream_wait.
bool step_forks(const ipmz_qp* s) {
  if (s->eqnone || s->B > 1) return false;
  if (debug_inject_mask() & IPMZ_INJECT_GRAPH_FORKS) return false;
  // the augmented factor and the normal equations' pipelined factor are both
  // one factor_impl of order N (= n + m + p): it forks from 3 outer panels
  const int nbo = nbo_for(s->ctx, s->N);
  return (s->N + nbo - 1) / nbo >= 3;
}

// a forked step still in flight (queue depth 1, step_impl) reads the storage,
// and takes the events of the context's pool, that a factor enqueued now would
int wait_pending_step(ipmz_qp* s) {
  if (s->step_pending) HIP_OK(hipEventSynchronize(s->step_done));
  s->step_pending = false;
  return IPMZ_OK;
}

// IPMZ_STEP_SKIP_CONVERGED on a step that cannot serve it, or with the restart: refused before anything is enqueued
int refuse_skip(const ipmz_qp* s, int flags, const char* who) {
  if (!(flags & IPMZ_STEP_SKIP_CONVERGED)) return IPMZ_OK;
  if (flags & IPMZ_STEP_RESTART_IF_CONVERGED)
    return fail(IPMZ_ERR_INVALID, std::string(who) + ": IPMZ_STEP_SKIP_CONVERGED with IPMZ_STEP_RESTART_IF_CONVERGED "
                                                     "(a converged QP cannot both restart and sit out)");
  if (can_skip_converged(s)) return IPMZ_OK;
  const char* why = s->B == 1 ? "a solver of one QP (ipmz_qp_solve stops at convergence already)"
                    : s->N > IPMZ_FUSED_NMAX ? "N > 1024 (the panel factor is not per QP)"
                    : s->ctx->nbi != 64 ? "inner block 128 (its batched factor is not per QP)"
                                        : "this factor path";
  return fail(IPMZ_ERR_INVALID, std::string(who) + ": IPMZ_STEP_SKIP_CONVERGED is not served for " + why +
                                    "; ask ipmz_batch_can_skip_converged");
}

int step_impl(ipmz_qp* s, int flags) {
  if (s) {
    const int rc = refuse_skip(s, flags, "ipmz_qp_step");
    if (rc) return rc;
  }
  if (!s || !s->loaded) return fail(IPMZ_ERR_STATE, "load or generate the QP first");
  HIP_OK(hipSetDevice(s->ctx->device));
  s->last_step_graph = 0;
  {
    // The caller's stream is capturing (torch.cuda.graph around step()): the
    // whole step goes into the caller's capture on that stream -- no hop to
    // the own stream, no host wait, no nested capture (the look-ahead
    // streams order through capture dependencies, ldlt.hip stream_wait; the
    // mixed solve enqueues all its passes, mixed.hip)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(s->ctx->stream, &cs));
    if (cs != hipStreamCaptureStatusNone) {
      if (s->timing) return fail(IPMZ_ERR_STATE, "phase timing inside a caller's graph capture");
      set_capture_origin(s->ctx->stream);
      const int rc = run_step(s, flags & ~IPMZ_STEP_GRAPH);
      set_capture_origin(nullptr);
      return rc;
    }
  }
  if (step_forks(s) && (!s->timing || s->ctx->stream != s->ctx->own)) {  // timing: phase events on own, below
    // A factorization that forks onto the look-ahead streams is enqueued
    // eagerly (~130-160 launches and event waits over four queues); with
    // the next step's packets already queued behind it the command processor
    // slows the running step down (C2: 3.9 vs 3.1 ms per step back to back;
    // tools/step_sync_ab.py), so at most one such step is in flight: the host
    // waits for the previous one before enqueuing the next.
    if (!s->step_done) HIP_OK(hipEventCreateWithFlags(&s->step_done, hipEventDisableTiming));
    int rc = wait_pending_step(s);
    if (rc) return rc;
    // On a stream the caller made (torch's default or side streams) the step
    // runs on the context's own stream, forked from the caller's, and the host
    // waits for it before the caller's stream is joined to it: a join left
    // pending on the caller's stream while the step runs cost ~1.2 ms per C3
    // step (15.7 vs 14.5 ms; the step on the caller's stream itself the same),
    // profiles/r03_s5/origin_stream_ab.log.  The host would wait for the step
    // before enqueuing the next one anyway (queue depth 1).
    hipStream_t caller = s->ctx->stream, own = s->ctx->own;
    const bool hop = caller != own;
    if (hop) {
      if (!s->step_in) HIP_OK(hipEventCreateWithFlags(&s->step_in, hipEventDisableTiming));
      HIP_OK(hipEventRecord(s->step_in, caller));
      HIP_OK(hipStreamWaitEvent(own, s->step_in, 0));
      s->ctx->stream = own;
    }
    rc = run_step(s, flags);
    s->ctx->stream = caller;
    if (rc) return rc;
    HIP_OK(hipEventRecord(s->step_done, own));
    if (hop) {
      HIP_OK(hipEventSynchronize(s->step_done));
      HIP_OK(hipStreamWaitEvent(caller, s->step_done, 0));  // complete: orders nothing pending
      return IPMZ_OK;
    }
    s->step_pending = true;
    return IPMZ_OK;
  }
  if (!(flags & IPMZ_STEP_GRAPH) || s->timing) return run_step(s, flags);
  hipStream_t st = s->ctx->stream;
  if (!s->gexec || s->graph_flags != flags) {
    drop_graph(s);
    // capture on the context's own stream: the caller's stream may be the
    // legacy default stream (torch's), which cannot be captured; the graph
    // is then launched on the caller's stream
    hipStream_t cap = s->ctx->own;
    IPMZ_TRACE("capture: begin");
    set_capture_origin(cap);  // ldlt.hip stream_wait: the look-ahead streams' ordering inside the capture
    HIP_OK(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
    s->ctx->stream = cap;
    int rc = run_step(s, flags);
    s->ctx->stream = st;
    IPMZ_TRACE("capture: step enqueued rc=%d", rc);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(cap, &g);
    set_capture_origin(nullptr);
    IPMZ_TRACE("capture: ended %d", (int)e);
    if (rc) {
      if (g) hipGraphDestroy(g);
      return rc;
    }
    if (e != hipSuccess) return fail(IPMZ_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
    s->graph = g;
    HIP_OK(hipGraphInstantiate(&s->gexec, g, nullptr, nullptr, 0));
    IPMZ_TRACE("capture: instantiated");
    s->graph_flags = flags;
  }
  HIP_OK(hipGraphLaunch(s->gexec, st));
  IPMZ_TRACE("graph launched");
  s->last_step_graph = 1;
  return IPMZ_OK;
}

// The sticky error words a path's kernels raise on a spin timeout (pe: the
// factor's, se: the persistent solve's; null where the path has none), the
// sentence for each, and the info word -- of a Newton step (step: no info), or
// of the factor and prepared solve that the *_kkt_solve* / *_newton_solve_multi
// calls enqueue (kkt_finish; never Path::Normal or Path::Mixed)
struct ErrWords {
  const int* info = nullptr;
  const unsigned *pe = nullptr, *se = nullptr;
  const char *pe_text = PANEL_TIMEOUT, *se_text = SOLVE_TIMEOUT;
};
ErrWords err_words(const ipmz_qp* s, bool step) {
  ErrWords e;
  if (!step) e.info = s->binfo;
  switch (path_of(s)) {
    case Path::Mixed:
      e.pe = s->mw.pctrl + PANEL_ERR_WORD;
      e.se = s->mw.ctrl + SOLVE_ERR_WORD;
      e.pe_text = e.se_text = ": a hand-off inside a persistent kernel of the mixed-precision factor / solve timed out; "
                              "the step is invalid";
      break;
    case Path::Normal:
    case Path::Ldlt: {
      const LdltWs w = s->normal ? normal_ws_of(s).k : ldlt_ws_of(s);  // (kkt_finish: through read_info)
      e.pe = w.pctrl + PANEL_ERR_WORD;
      e.se = w.ctrl + SOLVE_ERR_WORD;
      break;
    }
    case Path::LdltBatch:
      // only a factor that ran the two-workgroup kernel has a word to read (its launch zeroes it; the default
      // wave-specialized factor at C4's N = 320 has no cross-workgroup hand-off and needs no sync for it)
      if (s->ctx->nbi == 64 && small_pair_used(s->small_kernel, s->pflags != nullptr, s->B, s->N))
        e.pe = s->pflags + (size_t)s->B * IPMZ_PAIR_FLAGS;
      e.pe_text = step ? ": a hand-off of the two-workgroup batched factor timed out; the step is invalid"
                       : ": a hand-off of the two-workgroup batched factor timed out; the factor is invalid";
      break;
    case Path::BkGrid:
      e.pe = bk_grid_err_word(s->bkws, s->N);
      e.se = bk_ws(s->bkfws, s->N).ctrl + SOLVE_ERR_WORD;
      e.pe_text = step ? ": a grid barrier of the whole-device Bunch-Kaufman factor timed out; the step is invalid"
                       : ": a grid barrier of the whole-device Bunch-Kaufman factor timed out; the factor is invalid";
      if (step)
        e.se_text = ": a hand-off inside the persistent triangular solve of the Bunch-Kaufman factor timed out; the "
                    "step is invalid";
      break;
    case Path::BkSmall:  // the one-workgroup kernels have no cross-workgroup spins; the prepared solve's sweeps have
      if (!step) e.se = bk_solve_ws(s->bkpws.p, s->N).k.ctrl + SOLVE_ERR_WORD;
      break;
    case Path::BkBatch: break;  // no cross-workgroup spins; an info word per system (bk_batch_info)
  }
  return e;
}

// sticky error words of every persistent-kernel workspace the step uses
int qp_status(ipmz_qp* s) {
  const ErrWords e = err_words(s, true);
  if (!e.pe && !e.se) return IPMZ_OK;
  return ws_result(s->ctx->stream, nullptr, e.pe, e.se, s->normal ? "Newton step (normal equations)" : "Newton step",
                   e.pe_text, e.se_text);
}

// the B scalar blocks are one allocation with a stride: bytes between two QPs'
size_t scal_pitch(const ipmz_qp* s) { return (s->B > 1 ? (s->hq[1].scal - s->hq[0].scal) : SC_COUNT) * 8; }

int scalars_impl(ipmz_qp* s, double* out, int count) {
  HIP_OK(hipSetDevice(s->ctx->device));
  HIP_OK(hipMemcpy2DAsync(out, SC_COUNT * 8, s->hq[0].scal, scal_pitch(s), SC_COUNT * 8, count, hipMemcpyDeviceToHost,
                          s->ctx->stream));
  HIP_OK(hipStreamSynchronize(s->ctx->stream));
  return s->loaded ? qp_status(s) : IPMZ_OK;
}

// EqualityHandling::SlackedSlacks / NaiveSlacks: perm[k] = the step-vector index of reference-order element k
// (eqss_source, kernels.h: the map the device read-back gathers by)
std::vector<int64_t> eqss_perm(const ipmz_qp* s) {
  std::vector<int64_t> perm((size_t)s->state_len);
  for (int64_t k = 0; k < s->state_len; ++k) perm[(size_t)k] = eqss_source(k, s->hq[0]);
  return perm;
}

int get_state_impl(ipmz_qp* s, int i, int which, double* out) {
  if (which < 0 || which > 3 || !out) return fail(IPMZ_ERR_INVALID, "bad arguments");
  HIP_OK(hipSetDevice(s->ctx->device));
  const QPDev& q = s->hq[i];
  const double* src = which == 0 ? q.v[0] : which == 1 ? q.daff[0] : which == 2 ? q.dir[0] : q.r[0];
  if (s->eqss) {
    std::vector<double> tmp((size_t)s->state_len);
    HIP_OK(hipMemcpyAsync(tmp.data(), src, s->state_len * 8, hipMemcpyDeviceToHost, s->ctx->stream));
    HIP_OK(hipStreamSynchronize(s->ctx->stream));
    const auto perm = eqss_perm(s);
    for (int64_t k = 0; k < s->state_len; ++k) out[k] = tmp[(size_t)perm[(size_t)k]];
    return IPMZ_OK;
  }
  HIP_OK(hipMemcpyAsync(out, src, s->state_len * 8, hipMemcpyDeviceToHost, s->ctx->stream));
  HIP_OK(hipStreamSynchronize(s->ctx->stream));
  return IPMZ_OK;
}

// a host iterate in the reference's order -> the step's order
std::vector<double> state_in(const ipmz_qp* s, const double* in) {
  std::vector<double> v(in, in + s->state_len);
  if (s->eqss) {
    const auto perm = eqss_perm(s);
    for (int64_t k = 0; k < s->state_len; ++k) v[(size_t)perm[(size_t)k]] = in[k];
  }
  return v;
}

// The bodies of the ipmz_qp_* / ipmz_batch_* accessor pairs (arguments checked by the callers).
// The scalar blocks of the first count QPs to dst (device), dense; asynchronous
int copy_scalars_impl(ipmz_qp* s, double* dst, int count) {
  HIP_OK(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  HIP_OK(count == 1 ? hipMemcpyAsync(dst, s->hq[0].scal, SC_COUNT * 8, hipMemcpyDeviceToDevice, st)
                    : hipMemcpy2DAsync(dst, SC_COUNT * 8, s->hq[0].scal, scal_pitch(s), SC_COUNT * 8, count,
                                       hipMemcpyDeviceToDevice, st));
  return IPMZ_OK;
}
// the iterate `in` (host, the reference's order) into QPs [first, last), then every QP evaluated; synchronizes
int set_state_impl(ipmz_qp* s, int first, int last, const double* in) {
  HIP_OK(hipSetDevice(s->ctx->device));
  const std::vector<double> v = state_in(s, in);
  for (int i = first; i < last; ++i)
    HIP_OK(hipMemcpyAsync(s->hq[i].v[0], v.data(), s->state_len * 8, hipMemcpyHostToDevice, s->ctx->stream));
  HIP_OK(qp_evaluate(s->qb, s->ctx->stream));
  HIP_OK(hipStreamSynchronize(s->ctx->stream));
  return IPMZ_OK;
}
// the assembled KKT matrix of QP i (lower triangle, zeros above) to out (host, N x N)
int get_kkt_impl(ipmz_qp* s, int i, double* out) {
  HIP_OK(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  // (the whole matrix of every QP into K, as the non-fused step's assembly: the kept K0 is not touched)
  HIP_OK(qp_assemble(s->qb, st));
  HIP_OK(hipMemcpy2DAsync(out, (size_t)s->N * 8, s->hq[i].K, s->ldk * 8, (size_t)s->N * 8, s->N, hipMemcpyDeviceToHost,
                          st));
  HIP_OK(hipStreamSynchronize(st));
  for (int r = 0; r < s->N; ++r)
    for (int c = r + 1; c < s->N; ++c) out[(int64_t)r * s->N + c] = 0.0;
  return IPMZ_OK;
}
}  // namespace

extern "C" {

int ipmz_qp_create(ipmz_ctx* ctx, const ipmz_qp_config* cfg, ipmz_qp** out) { return create_solver(ctx, cfg, 1, out); }

int ipmz_qp_destroy(ipmz_qp* s) {
  if (!s) return IPMZ_OK;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  drop_graph(s);
  for (auto e : s->ev) hipEventDestroy(e);
  if (s->step_done) hipEventDestroy(s->step_done);
  if (s->step_in) hipEventDestroy(s->step_in);
  if (s->tr_pairs) {
    for (int i = 0; i < s->tr_cap; ++i) {
      hipEventDestroy(s->tr_pairs[i][0]);
      hipEventDestroy(s->tr_pairs[i][1]);
    }
    delete[] s->tr_pairs;
  }
  for (void* p : s->allocs) hipFree(p);  // (the GrowBufs' too)
  if (s->mw.hev) hipEventDestroy(s->mw.hev);
  if (s->mw.hst) hipHostFree(s->mw.hst);
  ipmz_ctx* ctx = s->ctx;
  delete s;
  bool last;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mutex);
    last = --ctx->users == 0 && ctx->closed;
  }
  if (last) ctx_free(ctx);
  return IPMZ_OK;
}

int ipmz_qp_load_host(ipmz_qp* s, const double* Q, const double* c, const double* A, const double* lA,
                      const double* uA, const double* C, const double* d, const double* lx, const double* ux) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  for (int i = 0; i < s->B; ++i) {
    int rc = load_one(s, i, Q, c, A, lA, uA, C, d, lx, ux);
    if (rc) return rc;
  }
  s->held = HELD_ALL;
  return initialize(s);
}

int ipmz_qp_generate(ipmz_qp* s, uint64_t seed) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  HIP_OK(hipSetDevice(s->ctx->device));
  HIP_OK(qp_generate(s->qb, seed, s->ctx->stream));
  s->held = HELD_ALL;
  return initialize(s);
}

int ipmz_qp_step(ipmz_qp* s, int flags) { return step_impl(s, flags); }

int ipmz_qp_last_step_graph(ipmz_qp* s) { return s ? s->last_step_graph : 0; }

int ipmz_qp_scalars(ipmz_qp* s, double* out) {
  if (!s || !out) return fail(IPMZ_ERR_INVALID, "null argument");
  return scalars_impl(s, out, 1);  // QP 0 (the ipmz_qp_* accessors address QP 0)
}

int ipmz_qp_device_scalars(ipmz_qp* s, double** out) {
  if (!s || !out) return fail(IPMZ_ERR_INVALID, "null argument");
  *out = s->hq[0].scal;
  return IPMZ_OK;
}

int ipmz_qp_copy_scalars(ipmz_qp* s, double* dst) {
  if (!s || !dst) return fail(IPMZ_ERR_INVALID, "null argument");
  return copy_scalars_impl(s, dst, 1);  // QP 0
}

int ipmz_qp_solve(ipmz_qp* s, int max_iter, double* trace, int* iterations) {
  if (!s || !s->loaded) return fail(IPMZ_ERR_STATE, "load or generate the QP first");
  double sc[SC_COUNT];
  int rc = scalars_impl(s, sc, 1);
  if (rc) return rc;
  int it = 0;
  for (; it < max_iter; ++it) {  // Optimizer.cpp:127-135
    double* row = trace ? trace + 8 * (int64_t)it : nullptr;
    if (row) {
      row[0] = sc[SC_F];
      row[1] = sc[SC_RES];
      row[2] = sc[SC_MU];
      row[7] = sc[SC_CONVERGED];
      row[3] = row[4] = row[5] = row[6] = 0.0;
    }
    if (sc[SC_CONVERGED] != 0.0) break;
    rc = step_impl(s, 0);
    if (rc) return rc;
    rc = scalars_impl(s, sc, 1);
    if (rc) return rc;
    if (row) {
      row[3] = sc[SC_ALPHA_AFF];
      row[4] = sc[SC_MU_AFF];
      row[5] = sc[SC_SIGMA];
      row[6] = sc[SC_ALPHA];
    }
  }
  if (iterations) *iterations = it;
  return IPMZ_OK;
}

int64_t ipmz_qp_state_len(ipmz_qp* s) { return s ? s->state_len : 0; }

int ipmz_qp_get_state(ipmz_qp* s, int which, double* out) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  return get_state_impl(s, 0, which, out);
}

int ipmz_qp_set_state(ipmz_qp* s, const double* in) {
  if (!s || !in) return fail(IPMZ_ERR_INVALID, "bad arguments");
  const int rc = set_state_impl(s, 0, s->B, in);  // every QP
  if (!rc) s->loaded = true;
  return rc;
}

int ipmz_qp_kkt_dim(ipmz_qp* s) { return s ? s->N : 0; }

int ipmz_qp_get_kkt(ipmz_qp* s, double* out) {
  if (!s || !out) return fail(IPMZ_ERR_INVALID, "bad arguments");
  return get_kkt_impl(s, 0, out);
}

int ipmz_qp_get_factor(ipmz_qp* s, double* L, double* D, double* P, int64_t* p_len) {
  if (!s) return fail(IPMZ_ERR_INVALID, "bad arguments");
  if (path_of(s) != Path::Ldlt || s->ctx->nbi != 64)
    return fail(IPMZ_ERR_STATE, "ipmz_qp_get_factor: single QPs on the fp64 augmented LDL^T with nbi = 64");
  HIP_OK(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  const int N = s->N;
  const int64_t q = solve_prep_elems(N) / 4;
  if (p_len) *p_len = 4 * q;
  const LdltWs w = ldlt_ws_of(s);
  if (L) HIP_OK(hipMemcpy2DAsync(L, (size_t)N * 8, s->K, s->ldk * 8, (size_t)N * 8, N, hipMemcpyDeviceToHost, st));
  if (D) HIP_OK(hipMemcpyAsync(D, s->D, (size_t)N * 8, hipMemcpyDeviceToHost, st));
  if (P) HIP_OK(hipMemcpyAsync(P, w.P, (size_t)(4 * q) * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (L)
    for (int r = 0; r < N; ++r)
      for (int c = r + 1; c < N; ++c) L[(int64_t)r * N + c] = 0.0;
  if (P) {  // M of the first block row and Q of the last are never built
    const int64_t blk = (int64_t)IPMZ_SOLVE_BLOCK * IPMZ_SOLVE_BLOCK;
    for (int64_t i = 0; i < blk; ++i) P[2 * q + i] = P[4 * q - blk + i] = 0.0;
  }
  return IPMZ_OK;
}

int ipmz_batch_get_kkt(ipmz_qp* s, int index, double* out) {
  int rc = check_index(s, index);
  if (rc) return rc;
  if (!out) return fail(IPMZ_ERR_INVALID, "bad arguments");
  return get_kkt_impl(s, index, out);
}

// Batched multi-right-hand-side solve (trsm.hip): which of the three paths
// serves nrhs rows per QP.
//
// BATCH_MULTI_CROSSOVER: the number of right-hand sides from which the blocked
// paths run; below it every row is one launch of the step's own batched
// single-vector solve (ldlt_solve_batched), all QPs at once.  From
// tools/batch_multi_bench.py (profiles/batch_multi/bench.json, DESIGN.md
// "Batched multi-right-hand-side solve"), solve alone = call(nrhs) - call(0):
// a looped row costs 0.148 ms (C4, N = 320, batch 1024) / 0.032 ms (batch
// 128), the one-launch solve 0.256 / 0.060 ms for up to 16 rows, so they break
// even at 1.7 / 1.9 rows.  At 2 rows the blocked path leads by 1.12x at batch
// 1024 but by 0.005 ms at batch 128, inside the loop's spread there (0.007
// ms); 4 is the first measured count at which it leads by more than the
// spread at both (2.3x / 2.2x).  3 rows were not measured (the loop would
// cost 0.44 / 0.10 ms against about 0.26 / 0.06): they stay looped.
//
// Fused or panels: where a QP's slab fits the LDS the one-launch solve is
// never slower than the panel chain at both C4 batch sizes (at 16 rows 0.28 vs
// 0.39-0.46 ms and 0.06 vs 0.08-0.12 ms), so eligibility alone decides.  Only
// at 128 rows and batch 1024 (and N = 832, batch 128) do 128-column panels
// lead it, by 4-6 %; at batch 128 they lose by 16 %.
static constexpr int BATCH_MULTI_CROSSOVER = 4;

static int batch_multi_impl(ipmz_qp* s, double* B, int64_t ldb, int64_t sB, int nrhs) {
  hipStream_t st = s->ctx->stream;
  const int nbi = s->ctx->nbi;
  const MultiPlan plan =
      multi_plan(nrhs, BATCH_MULTI_CROSSOVER, IPMZ_SOLVE_MULTI_PANEL, debug_inject_mask(), MultiKind::Batch);
  if (!plan.blocked) {
    for (int r = 0; r < nrhs; ++r)
      HIP_OK(ldlt_solve_batched(s->K, s->ldk, s->N, s->D, s->bLinv, nbi, B + (int64_t)r * ldb, s->B, s->sK, s->sD,
                                s->sL, sB, st));
    return IPMZ_OK;
  }
  const TrsmBatch tb = trsm_batch(s, sB);
  // one launch per batch where a system's slab fits a workgroup's LDS, unless
  // a panel width is forced; else the panel chain over all QPs
  if (plan.fused && ldlt_solve_fused_eligible(s->N, nbi)) {
    HIP_OK(ldlt_solve_fused(s->K, s->ldk, s->N, s->D, s->bLinv, nbi, B, ldb, nrhs, st, tb));
    return IPMZ_OK;
  }
  HIP_OK(ldlt_solve_multi<double>(s->K, s->ldk, s->N, s->D, s->bLinv, nbi, B, ldb, nrhs, plan.width, st, tb));
  return IPMZ_OK;
}

// What every call that takes a block of right-hand sides checks first: the data is loaded, and the block `name`
// -- per QP nrhs rows of len (`len_name`) elements, ld apart, the QPs' blocks sB apart -- is what the blocked
// kernels' 16-byte loads can address (aligned false: handed on to an entry point with its own alignment rule)
static int check_rhs_block(const ipmz_qp* s, const std::string& who, int nrhs, const char* name, const void* p,
                           int64_t ld, int64_t sB, int64_t len, const char* len_name, bool aligned = true) {
  if (!s->loaded) return fail(IPMZ_ERR_STATE, who + ": load (and initialize) the QP first");
  if (nrhs < 0 || ld < len || (ld & 1) || (nrhs > 0 && !p) ||
      (s->B > 1 && (sB < (int64_t)nrhs * ld || (sB & 1))))
    return fail(IPMZ_ERR_INVALID, who + ": bad arguments (nrhs >= 0; " + name + ": not null, row stride >= " + len_name +
                                      " and even" + (s->B > 1 ? ", QP stride >= nrhs * row stride and even)" : ")"));
  if (aligned && nrhs > 0 && ((uintptr_t)p & 15))
    return fail(IPMZ_ERR_INVALID, who + ": " + name + " must be 16-byte aligned");
  if (path_of(s) == Path::BkBatch && (s->N > IPMZ_BK_NMAX || s->B > 65535))  // the batched prepared solve's grid
    return fail(IPMZ_ERR_INVALID, who + ": EqualityHandling::None batches: N <= 4096 and batch <= 65535");
  return IPMZ_OK;
}

// What the four *_kkt_solve* calls and the two *_newton_solve_multi calls
// share, by the solver's path:
// kkt_ws_ensure  the Bunch-Kaufman prepared solves' workspace, on first use;
// kkt_enqueue    the step's own assembly and factor on the storage the next
//                step overwrites anyway (it assembles and factors again: the
//                iterate is only read), then the nrhs rows of B <- K^{-1} row;
//                asynchronous;
// kkt_finish     the one synchronize: the sticky error words, then the info
//                word(s).  info (host, batch ints, may be null) is filled per
//                QP for Bunch-Kaufman batches only.
static int kkt_ws_ensure(ipmz_qp* s) {  // (kept: the steps of these two paths solve on F itself)
  const Path path = path_of(s);
  if (path == Path::BkSmall) return grow(s, s->bkpws, (size_t)bk_solve_ws(nullptr, s->N).total);
  if (path == Path::BkBatch) return grow(s, s->bkpws, (size_t)bk_batch_ws(nullptr, s->N, s->B).total);
  return IPMZ_OK;  // (Path::BkGrid: every step prepares its solve)
}

static int kkt_enqueue(ipmz_qp* s, double* B, int64_t ldb, int64_t sB, int nrhs) {
  hipStream_t st = s->ctx->stream;
  // The whole matrix of every QP goes into K and is factored there in place
  // (factor_batch without K0), as the non-fused step does.  The fused step's
  // kept matrix K0 -- its off-diagonal part written once per load -- is
  // neither read nor written; that step rewrites K0's diagonal and all of L in
  // K itself.
  HIP_OK(qp_assemble(s->qb, st));
  int rc = factor_batch(s, nullptr, false);
  if (rc) return rc;
  switch (path_of(s)) {
    case Path::Ldlt:
      rc = ipmz_ldlt_solve_multi(s->ctx, s->N, s->K, s->ldk, s->D, s->ws, B, ldb, nrhs);
      break;
    case Path::LdltBatch: return batch_multi_impl(s, B, ldb, sB, nrhs);
    case Path::BkGrid:  // factor_batch left LT in bklt, L' in K and the operators in bkfws
      rc = bk_multi_impl(s->ctx, s->N, s->K, s->ldk, s->ipiv, s->bklt, s->K, s->ldk, bk_ws(s->bkfws, s->N), B, ldb, nrhs);
      break;
    case Path::BkSmall: {
      const BkSolveWs w = bk_solve_ws(s->bkpws.p, s->N);
      HIP_OK(bk_transpose(s->K, s->ldk, s->N, w.LT, st));
      HIP_OK(bk_setup(s->K, s->ldk, s->N, s->ipiv, s->binfo, w.LT, w.Lp, w.ldp, w.k, st));
      rc = bk_multi_impl(s->ctx, s->N, s->K, s->ldk, s->ipiv, w.LT, w.Lp, w.ldp, w.k, B, ldb, nrhs);
      break;
    }
    case Path::BkBatch: {
      if (nrhs == 0) return IPMZ_OK;
      const BkBatchWs w = bk_batch_ws(s->bkpws.p, s->N, s->B);
      if ((rc = bk_batch_prepare(s->ctx, s->N, s->B, s->K, s->ldk, s->sK, s->ipiv, s->sP, s->binfo, w))) return rc;
      return bk_batch_multi_impl(s->ctx, s->N, s->B, s->K, s->ldk, s->sK, s->ipiv, s->sP, w, B, ldb, sB, nrhs);
    }
    default: break;  // (Path::Normal, Path::Mixed: rejected by every caller)
  }
  unwatch(s->ctx);  // the single paths' workspace is the solver's: checked in kkt_finish, not at a later sync
  return rc;
}

static int kkt_finish(ipmz_qp* s, const char* what, int* info) {
  const Path path = path_of(s);
  if (path == Path::Ldlt) return read_info(s->ctx, ldlt_ws_of(s));  // checks the error words of s->ws itself
  if (path == Path::BkBatch) return bk_batch_info(s->ctx->stream, s->binfo, s->B, info);
  const ErrWords e = err_words(s, false);
  return ws_result(s->ctx->stream, e.info, e.pe, e.se, what, e.pe_text, e.se_text);
}

// the four *_kkt_solve* calls behind their own checks of the solver's path
static int kkt_solve(ipmz_qp* s, const char* who, int nrhs, double* B, int64_t ldb, int64_t sB, int* info) {
  const Path path = path_of(s);
  // (Path::Ldlt hands B on to ipmz_ldlt_solve_multi: its alignment rule, K and B from 2 rows on)
  int rc = check_rhs_block(s, who, nrhs, "B", B, ldb, sB, s->N, "N", path != Path::Ldlt);
  if (rc) return rc;
  HIP_OK(hipSetDevice(s->ctx->device));
  // (as the four stood before they shared this body: the batch calls check for a capture, _qp_kkt_solve_bk waits)
  if (s->B > 1 && (rc = not_capturing(s->ctx, who))) return rc;
  if ((path == Path::BkGrid || path == Path::BkSmall) && (rc = wait_pending_step(s))) return rc;
  if ((rc = kkt_ws_ensure(s))) return rc;
  if ((rc = kkt_enqueue(s, B, ldb, sB, nrhs))) return rc;
  return kkt_finish(s, who, info);  // synchronizes
}

int ipmz_batch_kkt_solve(ipmz_qp* s, int nrhs, double* B, int64_t ldb, int64_t sB) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B == 1) return ipmz_qp_kkt_solve(s, nrhs, B, ldb);
  if (s->eqnone)
    return fail(IPMZ_ERR_INVALID, "ipmz_batch_kkt_solve: EqualityHandling::None batches factor with Bunch-Kaufman, "
                                  "which has no batched multi-right-hand-side solve (fp64 LDL^T batches only)");
  return kkt_solve(s, "ipmz_batch_kkt_solve", nrhs, B, ldb, sB, nullptr);
}

int ipmz_batch_kkt_solve_bk(ipmz_qp* s, int nrhs, double* B, int64_t ldb, int64_t sB, int* info) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B == 1) {
    const int rc = ipmz_qp_kkt_solve_bk(s, nrhs, B, ldb);
    if (info) info[0] = rc;
    return rc;
  }
  if (!s->eqnone)
    return fail(IPMZ_ERR_INVALID, "ipmz_batch_kkt_solve_bk: EqualityHandling::None batches only (the Bunch-Kaufman "
                                  "factor); the LDL^T handlings solve with ipmz_batch_kkt_solve");
  return kkt_solve(s, "ipmz_batch_kkt_solve_bk", nrhs, B, ldb, sB, info);
}

int ipmz_qp_kkt_solve(ipmz_qp* s, int nrhs, double* B, int64_t ldb) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B != 1)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve: single QPs only, this is a batch (ipmz_batch_kkt_solve)");
  if (s->eqnone)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve: EqualityHandling::None factors with Bunch-Kaufman: its "
                                  "multi-right-hand-side solve is ipmz_qp_kkt_solve_bk");
  if (s->normal)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve: the normal-equations reduction is enabled (augmented LDL^T only)");
  if (s->mixed)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve: mixed precision is enabled (fp64 LDL^T only)");
  return kkt_solve(s, "ipmz_qp_kkt_solve", nrhs, B, ldb, 0, nullptr);
}

int ipmz_qp_kkt_solve_bk(ipmz_qp* s, int nrhs, double* B, int64_t ldb) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B != 1) return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve_bk: single QPs only, this is a batch");
  if (!s->eqnone)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve_bk: EqualityHandling::None only (the Bunch-Kaufman factor); "
                                  "the LDL^T handlings solve with ipmz_qp_kkt_solve");
  return kkt_solve(s, "ipmz_qp_kkt_solve_bk", nrhs, B, ldb, 0, nullptr);
}

// compute_search_direction_ for a block of residual vectors: rhs_elem's
// reduction of every row into the solver's workspace, the formulation's own
// factor and blocked solve there (kkt_enqueue), backsub_elem's
// back-substitution into Dir and ratio_elem's step length per row.
// adjoint: the transposed map instead (ipmz_*_newton_adjoint_multi) -- R is the
// block of cotangents G, Dir is Out = M^T G: E^T of every row into the
// workspace, the same factor and solves (K is symmetric), then F^T g + G_r^T y.
static int newton_multi(ipmz_qp* s, const char* who, bool adjoint, int nrhs, const double* R, int64_t ldr, int64_t sR,
                        double* Dir, int64_t ldd, int64_t sD, double* alpha, int* info) {
  const std::string w(who);
  int rc = refuse_unless_newton_order(s, w);
  if (!rc) rc = check_rhs_block(s, w, nrhs, adjoint ? "G" : "R", R, ldr, sR, s->state_len, "state_len");
  if (!rc) rc = check_rhs_block(s, w, nrhs, adjoint ? "Out" : "Dir", Dir, ldd, sD, s->state_len, "state_len");
  if (rc) return rc;
  HIP_OK(hipSetDevice(s->ctx->device));
  if ((rc = not_capturing(s->ctx, who))) return rc;
  if ((rc = wait_pending_step(s))) return rc;
  if ((rc = kkt_ws_ensure(s))) return rc;
  // the reduced right-hand sides: not Dir itself (the solves see rows of this
  // stride whatever ldd is, and nothing relies on the head of a Newton-order
  // row being the KKT order).  Every call ends synchronized, so growing it
  // here is safe
  const int64_t ldw = round_up(s->N, 2), sW = (int64_t)nrhs * ldw;
  if ((rc = grow(s, s->nmws, (size_t)(sW * s->B) * sizeof(double)))) return rc;
  hipStream_t st = s->ctx->stream;
  double* W = reinterpret_cast<double*>(s->nmws.p);
  if (nrhs > 0)
    HIP_OK(adjoint ? qp_adj_reduce_multi(s->qb, R, ldr, sR, W, ldw, sW, nrhs, st)
                   : qp_rhs_multi(s->qb, R, ldr, sR, W, ldw, sW, nrhs, st));
  if ((rc = kkt_enqueue(s, W, ldw, sW, nrhs))) return rc;
  if (nrhs > 0) {
    HIP_OK(adjoint ? qp_adj_expand_multi(s->qb, R, ldr, sR, W, ldw, sW, Dir, ldd, sD, nrhs, st)
                   : qp_backsub_multi(s->qb, R, ldr, sR, W, ldw, sW, Dir, ldd, sD, nrhs, st));
    if (alpha) HIP_OK(qp_ratio_multi(s->qb, Dir, ldd, sD, alpha, nrhs, st));
  }
  rc = kkt_finish(s, who, info);  // synchronizes
  if (info && path_of(s) != Path::BkBatch)
    for (int q = 0; q < s->B; ++q) info[q] = rc;
  return rc;
}

int ipmz_qp_newton_solve_multi(ipmz_qp* s, int nrhs, const double* R, int64_t ldr, double* Dir, int64_t ldd,
                               double* alpha) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B != 1)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_newton_solve_multi: single QPs only, this is a batch "
                                  "(ipmz_batch_newton_solve_multi)");
  return newton_multi(s, "ipmz_qp_newton_solve_multi", false, nrhs, R, ldr, 0, Dir, ldd, 0, alpha, nullptr);
}

int ipmz_batch_newton_solve_multi(ipmz_qp* s, int nrhs, const double* R, int64_t ldr, int64_t sR, double* Dir,
                                  int64_t ldd, int64_t sD, double* alpha, int* info) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B == 1) {
    const int rc = ipmz_qp_newton_solve_multi(s, nrhs, R, ldr, Dir, ldd, alpha);
    if (info) info[0] = rc;
    return rc;
  }
  return newton_multi(s, "ipmz_batch_newton_solve_multi", false, nrhs, R, ldr, sR, Dir, ldd, sD, alpha, info);
}

int ipmz_qp_newton_adjoint_multi(ipmz_qp* s, int nrhs, const double* G, int64_t ldg, double* Out, int64_t ldo) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B != 1)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_newton_adjoint_multi: single QPs only, this is a batch "
                                  "(ipmz_batch_newton_adjoint_multi)");
  return newton_multi(s, "ipmz_qp_newton_adjoint_multi", true, nrhs, G, ldg, 0, Out, ldo, 0, nullptr, nullptr);
}

int ipmz_batch_newton_adjoint_multi(ipmz_qp* s, int nrhs, const double* G, int64_t ldg, int64_t sG, double* Out,
                                    int64_t ldo, int64_t sO, int* info) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B == 1) {
    const int rc = ipmz_qp_newton_adjoint_multi(s, nrhs, G, ldg, Out, ldo);
    if (info) info[0] = rc;
    return rc;
  }
  return newton_multi(s, "ipmz_batch_newton_adjoint_multi", true, nrhs, G, ldg, sG, Out, ldo, sO, nullptr, info);
}

// Damped Newton toward the central-path point r(z; mu = kappa) = 0 of every QP (newton.hip "Centering on the
// central path").  One iteration is newton_multi's map for one row per QP with the solver's own slots as its
// block -- R the residual slots, Dir the direction slot, both contiguous in Newton order and aligned by
// construction, so the public checks of strides and alignment are not gone through -- between the test
// (qp_center_test) and the gated update (qp_center_update).  The host looks at the device once per iteration: the
// summary's two doubles, copied ahead of the synchronize in which kkt_finish reads the factor's words.
int ipmz_batch_center(ipmz_qp* s, double kappa, double tol, int max_iter, int* iterations, int* centered_count) {
  const std::string who = "ipmz_batch_center";
  if (!s) return fail(IPMZ_ERR_INVALID, who + ": null qp");
  if (!(kappa > 0.0 && kappa < INFINITY)) return fail(IPMZ_ERR_INVALID, who + ": kappa must be finite and > 0");
  if (!(tol > 0.0 && tol < INFINITY)) return fail(IPMZ_ERR_INVALID, who + ": tol must be finite and > 0");
  if (max_iter < 0) return fail(IPMZ_ERR_INVALID, who + ": max_iter < 0");
  if (s->normal) return fail(IPMZ_ERR_INVALID, who + ": the normal-equations reduction is enabled (augmented system only)");
  if (s->mixed) return fail(IPMZ_ERR_INVALID, who + ": mixed precision is enabled (fp64 factors only)");
  if (s->eqss)
    return fail(IPMZ_ERR_INVALID, who + ": EqualityHandling::SlackedSlacks / NaiveSlacks keep a permuted, merged view of "
                                        "the Newton order on the device; not served");
  if (s->eqpen)
    return fail(IPMZ_ERR_INVALID, who + ": EqualityHandling::PenaltyFunction puts the environment's mu into the KKT "
                                        "matrix; centering would have to own that mu; not served");
  if (s->slacks)
    return fail(IPMZ_ERR_INVALID, who + ": InequalityHandling::Slacks never converges (the reference's corrector "
                                        "defect): there is no solved iterate to center; not served");
  if (path_of(s) == Path::BkBatch && (s->N > IPMZ_BK_NMAX || s->B > 65535))
    return fail(IPMZ_ERR_INVALID, who + ": EqualityHandling::None batches: N <= 4096 and batch <= 65535");
  if (!s->loaded) return fail(IPMZ_ERR_STATE, who + ": load (and initialize) the QP first");
  HIP_OK(hipSetDevice(s->ctx->device));
  int rc;
  if ((rc = not_capturing(s->ctx, who.c_str()))) return rc;
  if ((rc = wait_pending_step(s))) return rc;
  if ((rc = kkt_ws_ensure(s))) return rc;
  // (every call ends synchronized, so growing the two buffers here is safe)
  const int64_t ldw = round_up(s->N, 2);
  if ((rc = grow(s, s->nmws, (size_t)(ldw * s->B) * sizeof(double)))) return rc;
  const int nb = qp_center_blocks(s->qb);
  if ((rc = grow(s, s->cws, (size_t)center_ws(nullptr, s->B, nb).total))) return rc;
  const CenterWs w = center_ws(s->cws.p, s->B, nb);
  hipStream_t st = s->ctx->stream;
  double* W = reinterpret_cast<double*>(s->nmws.p);
  const double* R = q0(s).r[0];
  double* Dir = q0(s).dir[0];
  const int64_t ldv = round_up(s->state_len, 2), sV = s->B > 1 ? s->hq[1].r[0] - s->hq[0].r[0] : 0;
  HIP_OK(hipMemsetAsync(w.frozen, 0, sizeof(int) * (size_t)s->B, st));
  HIP_OK(hipMemsetAsync(w.iters, 0, sizeof(int) * (size_t)s->B, st));
  double sum[2] = {0.0, 0.0};
  HIP_OK(qp_center_test(s->qb, kappa, tol, w, st));
  HIP_OK(hipMemcpyAsync(sum, w.sum, sizeof sum, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  int info = IPMZ_OK;
  for (int it = 0; it < max_iter && sum[0] != 0.0; ++it) {
    HIP_OK(qp_rhs_multi(s->qb, R, ldv, sV, W, ldw, ldw, 1, st));
    if ((rc = kkt_enqueue(s, W, ldw, ldw, 1))) return rc;
    HIP_OK(qp_backsub_multi(s->qb, R, ldv, sV, W, ldw, ldw, Dir, ldv, sV, 1, st));
    HIP_OK(qp_ratio_multi(s->qb, Dir, ldv, sV, w.alpha, 1, st));
    HIP_OK(qp_center_update(s->qb, w, st));
    HIP_OK(qp_center_test(s->qb, kappa, tol, w, st));
    HIP_OK(hipMemcpyAsync(sum, w.sum, sizeof sum, hipMemcpyDeviceToHost, st));
    rc = kkt_finish(s, who.c_str(), nullptr);  // synchronizes
    if (rc < 0) return rc;
    if (rc > 0 && (info == IPMZ_OK || rc < info)) info = rc;
  }
  // every QP evaluated as ipmz_batch_set_state does: the residual slots back at mu = 0, the scalar block's
  // evaluated entries those of the iterate
  HIP_OK(qp_evaluate(s->qb, st));
  if (iterations) HIP_OK(hipMemcpyAsync(iterations, w.iters, sizeof(int) * (size_t)s->B, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (centered_count) *centered_count = s->B - (int)sum[0];
  return info;
}

// the QP's mixed-precision workspace, allocated once (a captured step keeps its addresses)
static int ensure_mixed_ws(ipmz_qp* s) {
  if (s->mw.hst) return IPMZ_OK;
  // s->mw is filled last: a failure leaves mw.hst null, and the next call tries again (with the mws it has)
  const int nbo = nbo_for(s->ctx, s->N);
  const int rc = grow(s, s->mws, (size_t)mixed_ws_bytes(s->N, nbo), true);  // zeroed: sticky error words start clear
  if (rc) return rc;
  void *h = nullptr, *hd = nullptr;
  hipEvent_t hev = nullptr;
  // the stop test's host-mapped word (eager solves wait on it)
  if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
    return fail(IPMZ_ERR_NOMEM, "host allocation failed");
  hipError_t e = hipHostGetDevicePointer(&hd, h, 0);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&hev, hipEventDisableTiming);
  if (e != hipSuccess) {
    hipHostFree(h);
    return hip_fail(e, "ensure_mixed_ws", __FILE__, __LINE__);
  }
  mixed_ws_carve(s->mws.p, s->N, nbo, s->mw);
  s->mw.hst = static_cast<unsigned*>(h);
  s->mw.hst[0] = s->mw.hst[1] = 0u;
  s->mw.hst_dev = static_cast<unsigned*>(hd);
  s->mw.hev = hev;
  return IPMZ_OK;
}

int ipmz_qp_kkt_solve_mixed(ipmz_qp* s, int nrhs, double* B, int64_t ldb, double tol, int max_refine, double* stat) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (s->B != 1) return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve_mixed: single QPs only, this is a batch");
  if (s->eqnone)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve_mixed: EqualityHandling::None factors with Bunch-Kaufman, which "
                                  "has no mixed-precision form");
  if (s->eqpen)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve_mixed: EqualityHandling::PenaltyFunction has no mixed-precision "
                                  "form");
  if (s->normal)
    return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve_mixed: the normal-equations reduction is enabled (augmented "
                                  "system only)");
  int rc = check_rhs_block(s, "ipmz_qp_kkt_solve_mixed", nrhs, "B", B, ldb, 0, s->N, "N");
  if (rc) return rc;
  if (max_refine < 0) return fail(IPMZ_ERR_INVALID, "ipmz_qp_kkt_solve_mixed: bad arguments (max_refine >= 0)");
  ipmz_ctx* ctx = s->ctx;
  HIP_OK(hipSetDevice(ctx->device));
  if ((rc = not_capturing(ctx, "ipmz_qp_kkt_solve_mixed"))) return rc;
  if ((rc = wait_pending_step(s))) return rc;
  if ((rc = ensure_mixed_ws(s))) return rc;
  const int cap = std::max(nrhs, 1);
  MixedMultiWs m;
  const size_t mbytes = (size_t)mixed_multi_ws_carve(nullptr, s->N, cap, m);
  if (mbytes > s->mmws.bytes) HIP_OK(hipStreamSynchronize(ctx->stream));  // earlier solves may still read the old one
  if ((rc = grow(s, s->mmws, mbytes))) return rc;
  // the step's own assembly, and the fp32 factor in the workspace a mixed step
  // factors into again before it solves: the iterate is only read
  hipStream_t st = ctx->stream;
  HIP_OK(qp_assemble(s->qb, st));
  MixedWs w = s->mw;
  w.hst = nullptr;  // looped solves enqueue all passes: the steps' learned pass count stays theirs
  w.hst_dev = nullptr;
  w.hev = nullptr;
  if ((rc = mixed_factor_impl(ctx, s->K, s->ldk, w, nullptr))) return rc;
  mixed_multi_ws_carve(s->mmws.p, s->N, cap, m);
  if (nrhs == 1) {
    HIP_OK(mixed_solve(s->K, s->ldk, w, B, tol, max_refine, st));
    HIP_OK(hipMemcpyAsync(m.stat, w.stat, 2 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (stat) HIP_OK(hipMemcpyAsync(stat, m.stat, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  } else if (nrhs > 1) {
    if ((rc = mixed_multi_impl(ctx, s->K, s->ldk, w, m, B, ldb, nrhs, tol, max_refine, stat))) return rc;
  }
  const char* text = ": a hand-off inside a persistent kernel of the mixed-precision factor / solve timed out; the "
                     "result is invalid";
  return ws_result(st, w.info, w.pctrl + PANEL_ERR_WORD, w.ctrl + SOLVE_ERR_WORD, "ipmz_qp_kkt_solve_mixed", text,
                   text);
}

int ipmz_qp_set_mixed_precision(ipmz_qp* s, int enable, double tol, int max_refine) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (enable && (s->B != 1 || !(tol > 0.0) || max_refine < 0 || s->normal || s->eqnone || s->eqpen))
    return fail(IPMZ_ERR_INVALID, "mixed precision: single QPs, tol > 0, max_refine >= 0, augmented reduction, "
                                  "Regularization equalities");
  HIP_OK(hipSetDevice(s->ctx->device));
  if (enable) {
    const int rc = ensure_mixed_ws(s);
    if (rc) return rc;
  }
  s->mixed = enable != 0;
  s->ir_tol = tol;
  s->ir_max = max_refine;
  drop_graph(s);  // the captured step has the other solver baked in
  return IPMZ_OK;
}

int ipmz_qp_set_reduction(ipmz_qp* s, int reduction) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (reduction != IPMZ_REDUCTION_AUGMENTED && reduction != IPMZ_REDUCTION_NORMAL)
    return fail(IPMZ_ERR_INVALID, "unknown reduction");
  if (reduction == IPMZ_REDUCTION_NORMAL && (s->B != 1 || s->mixed || s->eqnone || s->eqpen || s->naive))
    return fail(IPMZ_ERR_INVALID, "normal equations: single QPs, not with mixed precision, Regularization equalities");
  HIP_OK(hipSetDevice(s->ctx->device));
  // (s->nws empty: normal_ws_of gives sizes only; no NaiveSlacks here, N = n + m + p.  Zeroed: sticky error words)
  if (reduction == IPMZ_REDUCTION_NORMAL && !s->nws.p && grow(s, s->nws, (size_t)normal_ws_of(s).total, true))
    return IPMZ_ERR_NOMEM;
  s->normal = reduction == IPMZ_REDUCTION_NORMAL;
  drop_graph(s);
  return IPMZ_OK;
}

int ipmz_qp_set_timing(ipmz_qp* s, int enable) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  HIP_OK(hipSetDevice(s->ctx->device));
  s->timing = enable != 0;
  if (s->timing && s->ev.empty()) {
    s->ev.resize(8);
    for (size_t i = 0; i < s->ev.size(); ++i) HIP_OK(hipEventCreate(&s->ev[i]));
    s->tr_cap = (s->N + 63) / 64 + 8;
    s->tr_pairs = new hipEvent_t[s->tr_cap][2];
    for (int i = 0; i < s->tr_cap; ++i) {
      HIP_OK(hipEventCreate(&s->tr_pairs[i][0]));
      HIP_OK(hipEventCreate(&s->tr_pairs[i][1]));
    }
  }
  for (double& x : s->ph_ms) x = 0.0;
  s->tr_flops = 0.0;
  s->tr_launches = 0;
  return IPMZ_OK;
}

int ipmz_qp_phase_times(ipmz_qp* s, double* ms, double* flops, int64_t* launches) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (ms)
    for (int i = 0; i < IPMZ_PH_COUNT; ++i) ms[i] = s->ph_ms[i];
  if (flops) *flops = s->tr_flops;
  if (launches) *launches = s->tr_launches;
  return IPMZ_OK;
}

// ---- batches of independent QPs (config C4) ---------------------------------
int ipmz_batch_create(ipmz_ctx* ctx, const ipmz_qp_config* cfg, int batch, ipmz_qp** out) {
  return create_solver(ctx, cfg, batch, out);
}
int ipmz_batch_size(ipmz_qp* s) { return s ? s->B : 0; }
int ipmz_batch_load_host(ipmz_qp* s, int index, const double* Q, const double* c, const double* A, const double* lA,
                         const double* uA, const double* C, const double* d, const double* lx, const double* ux) {
  int rc = check_index(s, index);
  if (rc) return rc;
  if ((rc = load_one(s, index, Q, c, A, lA, uA, C, d, lx, ux))) return rc;
  // (every block is held once each QP has been filled)
  if (s->host_filled.empty()) s->host_filled.assign((size_t)s->B, 0);
  if (!s->host_filled[(size_t)index]) {
    s->host_filled[(size_t)index] = 1;
    if (++s->host_filled_count == s->B) s->held = HELD_ALL;
  }
  // the kept KKT matrix K0 (off-diagonal part written only by
  // initialize) and the residuals still hold the old data: no step
  // until ipmz_batch_initialize rebuilds them
  s->loaded = false;
  return IPMZ_OK;
}
int ipmz_batch_initialize(ipmz_qp* s) {
  return s ? initialize(s) : fail(IPMZ_ERR_INVALID, "null qp");
}
int ipmz_batch_scalars(ipmz_qp* s, double* out) {
  if (!s || !out) return fail(IPMZ_ERR_INVALID, "null argument");
  return scalars_impl(s, out, s->B);
}
int ipmz_batch_get_state(ipmz_qp* s, int index, int which, double* out) {
  int rc = check_index(s, index);
  if (rc) return rc;
  return get_state_impl(s, index, which, out);
}
int ipmz_batch_set_state(ipmz_qp* s, int index, const double* in) {
  int rc = check_index(s, index);
  if (rc) return rc;
  if (!in) return fail(IPMZ_ERR_INVALID, "null state");
  return set_state_impl(s, index, index + 1, in);
}
int ipmz_batch_copy_scalars(ipmz_qp* s, double* dst) {
  if (!s || !dst) return fail(IPMZ_ERR_INVALID, "null argument");
  return copy_scalars_impl(s, dst, s->B);
}
int ipmz_batch_summary(ipmz_qp* s, double* dst) {
  if (!s || !dst) return fail(IPMZ_ERR_INVALID, "null argument");
  HIP_OK(hipSetDevice(s->ctx->device));
  HIP_OK(qp_batch_summary(s->qb, dst, s->ctx->stream));
  return IPMZ_OK;
}
// Steps until every QP converged or max_iter; a converged QP keeps its
// iterate.  converged_count: host, may be NULL.
int ipmz_batch_solve(ipmz_qp* s, int max_iter, int* iterations, int* converged_count) {
  if (!s || !s->loaded) return fail(IPMZ_ERR_STATE, "load or generate the batch first");
  std::vector<double> sc((size_t)s->B * SC_COUNT);
  int it = 0, nconv = 0;
  for (;; ++it) {
    int rc = scalars_impl(s, sc.data(), s->B);
    if (rc) return rc;
    nconv = 0;
    for (int i = 0; i < s->B; ++i) nconv += sc[(size_t)i * SC_COUNT + SC_CONVERGED] != 0.0;
    if (nconv == s->B || it >= max_iter) break;
    if ((rc = step_impl(s, 0))) return rc;
  }
  if (iterations) *iterations = it;
  if (converged_count) *converged_count = nconv;
  return IPMZ_OK;
}
int ipmz_batch_can_skip_converged(ipmz_qp* s) { return s && can_skip_converged(s) ? 1 : 0; }
// The same loop with the step's flags, looking at the device every check_every steps: a look is the batch's
// summary (one launch) and a copy of its 3 doubles
int ipmz_batch_solve_ex(ipmz_qp* s, int max_iter, int step_flags, int check_every, int* iterations,
                        int* converged_count) {
  const char* who = "ipmz_batch_solve_ex";
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (max_iter < 0 || check_every < 1 || (step_flags & ~(IPMZ_STEP_SKIP_CONVERGED | IPMZ_STEP_GRAPH)))
    return fail(IPMZ_ERR_INVALID, std::string(who) + ": bad arguments (max_iter >= 0, check_every >= 1, step_flags of "
                                                     "IPMZ_STEP_SKIP_CONVERGED and IPMZ_STEP_GRAPH only)");
  int rc = refuse_skip(s, step_flags, who);
  if (rc) return rc;
  if (!s->loaded) return fail(IPMZ_ERR_STATE, "load or generate the batch first");
  HIP_OK(hipSetDevice(s->ctx->device));
  if ((rc = not_capturing(s->ctx, who))) return rc;
  if (!s->summary && !(s->summary = dev_alloc<double>(s, 3, false))) {  // (every look writes all three)
    s->alloc_failed = false;  // (create_solver's flag)
    (void)hipGetLastError();
    return fail(IPMZ_ERR_NOMEM, "device allocation failed");
  }
  hipStream_t st = s->ctx->stream;
  double sum[3];
  int it = 0;
  for (;;) {
    HIP_OK(qp_batch_summary(s->qb, s->summary, st));
    HIP_OK(hipMemcpyAsync(sum, s->summary, sizeof(sum), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if ((rc = qp_status(s))) return rc;
    if (sum[2] == 0.0 || it >= max_iter) break;
    for (const int end = max_iter - it < check_every ? max_iter : it + check_every; it < end; ++it)
      if ((rc = step_impl(s, step_flags))) return rc;
  }
  if (iterations) *iterations = it;
  if (converged_count) *converged_count = s->B - (int)sum[2];
  return IPMZ_OK;
}
int ipmz_batch_set_factor_kernel(ipmz_qp* s, int kernel) {
  if (!s || kernel < IPMZ_BATCH_FACTOR_AUTO || kernel > IPMZ_BATCH_FACTOR_LEFT)
    return fail(IPMZ_ERR_INVALID, "ipmz_batch_set_factor_kernel: bad arguments");
  if (kernel == IPMZ_BATCH_FACTOR_PAIR && !(s->pflags && small_pair_eligible(s->B, s->N)))
    return fail(IPMZ_ERR_INVALID, "ipmz_batch_set_factor_kernel: two workgroups per QP need a batch of small systems "
                                  "(N <= 1024) with 2 * batch <= #CU");
  drop_graph(s);  // the captured step has the other kernel baked in
  s->small_kernel = kernel;
  return IPMZ_OK;
}

// build_environment for the whole batch from device memory: the bound check
// (one launch, one synchronize for its verdict), the copy of every supplied
// block (io.hip), then initialize().  A captured step graph stays: it holds the
// addresses of the solver's storage and the kernel selection, neither of which
// a load changes, and reads the data and the kept matrix K0 -- whose
// off-diagonal part initialize() rewrites from the new data -- when replayed.
int ipmz_batch_load_device(ipmz_qp* s, const ipmz_qp_device_data* data) {
  const std::string who = "ipmz_batch_load_device";
  if (!s || !data) return fail(IPMZ_ERR_INVALID, who + ": null argument");
  const int dims[3] = {s->n, s->m_usr, s->p_usr};
  const QpBlocksIn in = data_blocks<const double>(*data, nullptr, dims);
  BlockFacts facts;
  if (int rc = check_blocks(s, who, in, dims, BlockRules{"shared", -1, false, false}, &facts)) return rc;
  const unsigned supplied = facts.supplied;
  const unsigned absent = (dims[1] ? 0 : HELD_A | HELD_LA | HELD_UA) | (dims[2] ? 0 : HELD_CEQ | HELD_D);
  if (const unsigned missing = HELD_ALL & ~(supplied | absent | s->held)) {
    std::string names;
    for (const DataBlockInfo& b : DATA_BLOCKS)
      if (missing & b.held) names += std::string(names.empty() ? "" : ", ") + b.name;
    return fail(IPMZ_ERR_STATE, who + ": not supplied and never loaded or generated: " + names);
  }
  HIP_OK(hipSetDevice(s->ctx->device));
  int rc = not_capturing(s->ctx, "ipmz_batch_load_device");
  if (rc) return rc;
  if ((rc = wait_pending_step(s))) return rc;
  hipStream_t st = s->ctx->stream;
  unsigned long long verdict = IPMZ_IO_VALID;
  HIP_OK(qp_io_validate(s->qb, in, s->verdict, st));
  HIP_OK(hipMemcpyAsync(&verdict, s->verdict, sizeof verdict, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (verdict != IPMZ_IO_VALID)  // nothing was written
    return fail(IPMZ_ERR_INVALID, who + ": QP " + std::to_string(verdict >> 33) +
                                      ((verdict >> 32 & 1) ? ": l_A <= u_A violated at " : ": l_x < u_x violated at ") +
                                      std::to_string(verdict & 0xffffffffull));
  HIP_OK(qp_io_pack(s->qb, in, st));
  // the scalar blocks as a new solver has them: the last step's entries belong to the data just replaced
  HIP_OK(hipMemsetAsync(s->hq[0].scal, 0, scal_pitch(s) * (size_t)s->B, st));
  s->held |= supplied;
  return initialize(s);
}

int ipmz_batch_copy_state(ipmz_qp* s, int which, double* dst, int64_t ld) {
  if (!s) return fail(IPMZ_ERR_INVALID, "null qp");
  if (which < IPMZ_STATE_VARS || which > IPMZ_STATE_RES || !dst || ld < s->state_len)
    return fail(IPMZ_ERR_INVALID, "ipmz_batch_copy_state: bad arguments (which: IPMZ_STATE_*; dst: not null, row stride "
                                  ">= state_len)");
  if (!s->loaded) return fail(IPMZ_ERR_STATE, "ipmz_batch_copy_state: load or generate the QP first");
  HIP_OK(hipSetDevice(s->ctx->device));
  HIP_OK(qp_gather_state(s->qb, which, dst, ld, s->ctx->stream));
  return IPMZ_OK;
}

// ipmz_batch_set_state for the whole batch from device memory (io.hip): the check of the pushed rows (one kernel,
// one synchronize for its verdict; not with IPMZ_SET_STATE_UNCHECKED), the scatter with the push, then
// set_state_impl's evaluation of every QP.  Besides the iterate, the residuals and the scalar block's evaluated
// entries nothing moves: the direction slots, the last step's scalars, the kept matrix K0, the restart snapshot,
// a captured step graph and the blocking are the host call's to leave alone and this one's.
int ipmz_batch_set_state_device(ipmz_qp* s, const double* src, int64_t ld, const int32_t* take, double floor,
                                int flags) {
  const std::string who = "ipmz_batch_set_state_device";
  if (!s || !src) return fail(IPMZ_ERR_INVALID, who + ": null argument");
  if (ld < s->state_len)
    return fail(IPMZ_ERR_INVALID, who + ": row stride " + std::to_string(ld) + " < state_len " +
                                      std::to_string(s->state_len));
  if (flags & ~IPMZ_SET_STATE_UNCHECKED) return fail(IPMZ_ERR_INVALID, who + ": unknown flag bit");
  if (!(floor >= 0.0 && floor < INFINITY))
    return fail(IPMZ_ERR_INVALID, who + ": floor must be finite and >= 0");
  if (floor > 0.0 && s->slacks)
    return fail(IPMZ_ERR_INVALID, who + ": floor > 0 with InequalityHandling::Slacks (its positivity is x - l_x, "
                                        "u_x - x, s - l_A, u_A - s, not a slot a push could raise)");
  if (!s->loaded) return fail(IPMZ_ERR_STATE, who + ": load (and initialize) the QP first");
  HIP_OK(hipSetDevice(s->ctx->device));
  const bool checked = !(flags & IPMZ_SET_STATE_UNCHECKED);
  int rc;
  if (checked && (rc = not_capturing(s->ctx, who.c_str()))) return rc;
  if ((rc = wait_pending_step(s))) return rc;
  hipStream_t st = s->ctx->stream;
  if (checked) {
    unsigned long long verdict = IPMZ_IO_VALID;
    HIP_OK(qp_scatter_validate(s->qb, src, ld, take, floor, s->verdict, st));
    HIP_OK(hipMemcpyAsync(&verdict, s->verdict, sizeof verdict, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (verdict != IPMZ_IO_VALID) {  // nothing was written
      const unsigned long long L = (unsigned long long)s->state_len;
      return fail(IPMZ_ERR_INVALID, who + ": QP " + std::to_string(verdict / L) + ": not an interior iterate at index " +
                                        std::to_string(verdict % L) +
                                        " (NaN, a non-positive slack or multiplier, or x / s not strictly inside its "
                                        "bounds)");
    }
  }
  HIP_OK(qp_scatter_state(s->qb, src, ld, take, floor, st));
  HIP_OK(qp_evaluate(s->qb, st));
  return IPMZ_OK;
}

// (d r / d data)^T w into a caller's blocks (grad.hip): ipmz_batch_load_device's
// block description and checks with writable blocks, refused like the adjoint
// pair (newton_multi).  Launches only: no synchronize, and an allocation only
// when a shared matrix block is first asked for.
int ipmz_batch_data_vjp(ipmz_qp* s, const double* W, int64_t sW, const ipmz_qp_device_grad* grad) {
  const std::string who = "ipmz_batch_data_vjp";
  if (!s || !W || !grad) return fail(IPMZ_ERR_INVALID, who + ": null argument");
  int rc = refuse_unless_newton_order(s, who);
  if (rc) return rc;
  if (s->B > 1 && sW < s->state_len)
    return fail(IPMZ_ERR_INVALID, who + ": W: QP stride " + std::to_string(sW) + " < state_len");
  const int dims[3] = {s->n, s->m, s->p};
  const QpBlocksOut o = data_blocks<double>(reinterpret_cast<const ipmz_qp_device_data&>(*grad), nullptr, dims);
  BlockFacts facts;
  if ((rc = check_blocks(s, who, o, dims, BlockRules{"summed over the batch", -1, false, false}, &facts))) return rc;
  HIP_OK(hipSetDevice(s->ctx->device));
  if ((rc = wait_pending_step(s))) return rc;  // (a forked step still in flight writes the iterate this call reads)
  if (facts.shared_matrix) {  // once per solver: the size follows from the shape alone
    const size_t need = (size_t)vjp_ws(nullptr, qp_grad_part_elems(s->qb)).total;
    if ((rc = grow_unless_capturing(s, s->vjpws, need, who, "the shared blocks' workspace is not allocated yet (make "
                                                            "one call outside the capture first)")))
      return rc;
  }
  HIP_OK(qp_data_vjp(s->qb, 1, W, 0, s->B > 1 ? sW : 0, o, vjp_ws(s->vjpws.p, 0).part, s->ctx->stream));
  return IPMZ_OK;
}

// The call above for ncot cotangent rows per QP: W's rows checked as the adjoint
// pair checks its Out, the blocks as ipmz_batch_data_jvp checks its tangents (a
// row stride per block), with the gradient's rule for a solver of one QP.  The
// workspace holds a slab of IPMZ_VJP_SLAB rows' partials, never all of them.
int ipmz_batch_data_vjp_multi(ipmz_qp* s, int ncot, const double* W, int64_t ldw, int64_t sW,
                              const ipmz_qp_device_grad_multi* grad) {
  const std::string who = "ipmz_batch_data_vjp_multi";
  if (!s || !W || !grad) return fail(IPMZ_ERR_INVALID, who + ": null argument");
  int rc = refuse_unless_newton_order(s, who);
  if (rc) return rc;
  if (ncot < 0) return fail(IPMZ_ERR_INVALID, who + ": ncot < 0");
  if (ldw < s->state_len) return fail(IPMZ_ERR_INVALID, who + ": W: row stride " + std::to_string(ldw) + " < state_len");
  if (s->B > 1 && ncot > 0 && sW < (int64_t)(ncot - 1) * ldw + s->state_len)
    return fail(IPMZ_ERR_INVALID, who + ": W: QP stride " + std::to_string(sW) + " < (ncot - 1) * row stride + state_len");
  const int dims[3] = {s->n, s->m, s->p};
  const int64_t tq[DB_COUNT] = {grad->tQ, grad->tA, grad->tC, grad->tc, grad->tlx, grad->tux, grad->tlA, grad->tuA, grad->td};
  const QpBlocksOut o = data_blocks<double>(reinterpret_cast<const ipmz_qp_device_data&>(grad->g), tq, dims);
  BlockFacts facts;
  if ((rc = check_blocks(s, who, o, dims, BlockRules{"summed over the batch", ncot, false, true}, &facts))) return rc;
  if (ncot == 0) return IPMZ_OK;
  HIP_OK(hipSetDevice(s->ctx->device));
  if ((rc = wait_pending_step(s))) return rc;  // (a forked step still in flight writes the iterate this call reads)
  if (facts.shared_matrix) {
    const size_t need = (size_t)vjp_ws(nullptr, qp_grad_part_elems(s->qb, ncot)).total;
    if ((rc = grow_unless_capturing(s, s->vjpws, need, who, "the shared blocks' workspace is too small for this call "
                                                            "(make one such call outside the capture first)")))
      return rc;
  }
  HIP_OK(qp_data_vjp(s->qb, ncot, W, ldw, s->B > 1 ? sW : 0, o, vjp_ws(s->vjpws.p, 0).part, s->ctx->stream));
  return IPMZ_OK;
}

// (d r / d data) applied to ntan tangents of the data per QP (jvp.hip): the
// block description and checks of the call above with a tangent stride per
// block, R checked as ipmz_batch_newton_solve_multi checks its R.  Launches
// only: no synchronize, and an allocation only when the matrix products need
// more workspace than any call before.
int ipmz_batch_data_jvp(ipmz_qp* s, int ntan, const ipmz_qp_device_tangent* tan, double* R, int64_t ldr, int64_t sR) {
  const std::string who = "ipmz_batch_data_jvp";
  if (!s || !tan || !R) return fail(IPMZ_ERR_INVALID, who + ": null argument");
  int rc = refuse_unless_newton_order(s, who);
  if (rc) return rc;
  if (ntan < 0) return fail(IPMZ_ERR_INVALID, who + ": ntan < 0");
  if (ldr < s->state_len || (ldr & 1))
    return fail(IPMZ_ERR_INVALID, who + ": R: row stride " + std::to_string(ldr) + " must be >= state_len and even");
  if (s->B > 1 && (sR < (int64_t)ntan * ldr || (sR & 1)))
    return fail(IPMZ_ERR_INVALID, who + ": R: QP stride " + std::to_string(sR) + " must be >= ntan * row stride and even");
  if ((uintptr_t)R & 15) return fail(IPMZ_ERR_INVALID, who + ": R must be 16-byte aligned");
  const int dims[3] = {s->n, s->m, s->p};
  const int64_t tq[DB_COUNT] = {tan->tQ, tan->tA, tan->tC, tan->tc, tan->tlx, tan->tux, tan->tlA, tan->tuA, tan->td};
  QpBlocksIn in = data_blocks<const double>(tan->d, tq, dims);
  BlockFacts facts;
  // (a solver of one QP ignores the QP strides, a call with one tangent the tangent strides)
  if ((rc = check_blocks(s, who, in, dims, BlockRules{"shared", ntan, true, true}, &facts))) return rc;
  if (ntan == 0) return IPMZ_OK;
  if (s->B == 1)
    for (int64_t& sq : in.sq) sq = 0;
  HIP_OK(hipSetDevice(s->ctx->device));
  if ((rc = wait_pending_step(s))) return rc;  // (a forked step still in flight writes the iterate this call reads)
  const int64_t elems = (int64_t)s->B * ntan * qp_jvp_plan(s->qb, in).seg;
  if ((rc = grow_unless_capturing(s, s->jvpws, (size_t)jvp_ws(nullptr, elems).total, who,
                                  "the products' workspace is too small for this call (make one such call outside "
                                  "the capture first)")))
    return rc;
  HIP_OK(qp_data_jvp(s->qb, ntan, in, R, ldr, s->B > 1 ? sR : 0, jvp_ws(s->jvpws.p, 0).prod, s->ctx->stream));
  return IPMZ_OK;
}

}  // extern "C"
