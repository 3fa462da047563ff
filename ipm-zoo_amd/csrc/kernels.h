// Host-side launchers of the gfx950 kernels (internal to libipmz).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <functional>

#define IPMZ_NBO_MAX 512
#define IPMZ_PANEL_CTRL_WORDS 320
// fused factor: largest N whose chain launches start beside the previous
// panel's rows launch (ldlt.hip)
#define IPMZ_EARLY_CHAIN_MAX_N 4096
// rows per partial sum of the transposed mat-vecs A^T y, C^T y (newton.hip)
#define IPMZ_TCHUNK 32
#define IPMZ_CHAIN_STAMP_BLOCKS 512  // (debug stamps: N <= 32768)
#define IPMZ_SOLVE_BLOCK 128     // rows per block of the persistent solve
#define IPMZ_SOLVE_CTRL_WORDS 8  // its control words (error, tickets, sweep counters)

namespace ipmz {

// Fault injection for the tests of the spin-timeout path (ipmz_debug_inject):
// a persistent kernel launched while its bit is set drops its first
// hand-off, so every consumer times out and raises the sticky error word.
// IPMZ_INJECT_GRAPH_FORKS: not a fault -- IPMZ_STEP_GRAPH captures steps whose
// factor forks onto the look-ahead streams too (the capture experiment of
// tests/test_gpu_graph.py, bitwise the eager step) instead of enqueuing them
// eagerly (the production choice: graph replay of a forked step is slower).
// DEBUG bits (determinism experiments): 16 = the mixed factor stops after
// the scale + fp32 conversion, 32 = factors run on one stream (no look-ahead)
// 64 = trace the host calls of a step to stderr (the capture experiment),
// 128 = the fp32 trailing and strip updates on the gemm.h engine instead of gemm32.h (A/B),
// 256 = the fp32 factor's look-ahead strip on the trailing stream before the trailing update (no fourth stream),
// 512 = the eager mixed-precision solve enqueues all max_refine + 1 passes (no host stop test),
// 1024 = the fp64 trailing and strip updates on gemm.h's register-staged kernel instead of gemm64.h's (A/B),
// 2048 = an early chain launch (started beside the previous panel's rows launch) never sees that
//        launch's RDONE flags: it gives its roles back after 1 ms and the rows launch takes them
//        (the serialized-dispatch path, tests/test_gpu_panel_forms.py),
// 4096 = the chain launch draws no ticket: the rows launch runs every chain role in its 4-wave form
//        (what a serialized dispatch order can produce; the forms must factor bitwise alike),
// 8192 = batches assemble the whole KKT into K every step (not the kept K0) (A/B),
// 16384 = batches run the two solves and the phases between them as separate launches (A/B),
// 65536 = every multi-right-hand-side solve runs its blocked path from 2 right-hand sides on (no looped
//         single-vector solves below the crossover) (A/B, tools/*_multi_bench.py),
// 131072 / 262144 = ... with 512- / 128-column panels instead of its default width (A/B); the batched solves
//         then take the panel chain where the one-launch solve is eligible (capi.h multi_plan: the rule per path),
// 524288 / 1048576 = the persistent solve splits every 128-row block over 2 / 4 workgroups, whatever
//         its table says; both bits = the unsplit solve (all three bitwise alike,
//         tests/test_gpu_solve_split.py),
// 2097152 / 4194304 = ipmz_*_newton_solve_multi's element-wise kernels take 1 / 8 rows per thread instead
//         of IPMZ_NEWTON_MULTI_RPG; both bits = 2 (A/B, tools/newton_multi_bench.py; the same bits in every row);
//         ipmz_*_newton_adjoint_multi's two kernels launch the same way,
// 8388608 = the single-QP step keeps the serial order around its forked factor: the whole assembly before
//         it, the affine right-hand side, solve_prep and the whole forward sweep after it (A/B and
//         tests/test_gpu_step_edges.py: bitwise the overlapped order, DESIGN.md §4 "The factor's idle edges"),
// bits 24-29 = v > 0: the early forward sweep of that step covers (v - 1) * 128 rows instead of the rows
//         that are final when the factor turns chain-bound (tests: the split at every boundary),
enum { IPMZ_INJECT_SOLVE = 1, IPMZ_INJECT_PANEL = 2, IPMZ_INJECT_GRAPH_FORKS = 4, IPMZ_DEBUG_CONVERT_ONLY = 16,
       IPMZ_DEBUG_ONE_STREAM = 32, IPMZ_DEBUG_TRACE = 64, IPMZ_DEBUG_F32_ENGINE = 128,
       IPMZ_DEBUG_NO_FOURTH = 256, IPMZ_DEBUG_IR_FULL = 512,
       IPMZ_DEBUG_F64_ENGINE = 1024, IPMZ_DEBUG_GIVEBACK = 2048, IPMZ_DEBUG_ROWS_CHAIN = 4096,
       IPMZ_DEBUG_NO_K0 = 8192, IPMZ_DEBUG_NO_FUSED_SOLVES = 16384, IPMZ_DEBUG_READY_LATE = 32768,
       IPMZ_DEBUG_MULTI_BLOCKED = 65536, IPMZ_DEBUG_MULTI_W512 = 131072,
       IPMZ_DEBUG_MULTI_W128 = 262144, IPMZ_DEBUG_SOLVE_H2 = 524288, IPMZ_DEBUG_SOLVE_H4 = 1048576,
       IPMZ_DEBUG_NEWTON_RPG1 = 2097152, IPMZ_DEBUG_NEWTON_RPG8 = 4194304, IPMZ_DEBUG_SERIAL_EDGES = 8388608,
       IPMZ_DEBUG_EDGE_ROWS_SHIFT = 24, IPMZ_DEBUG_EDGE_ROWS_MASK = 63 << 24 };
#define IPMZ_TRACE(...)                                                  \
  do {                                                                   \
    if (::ipmz::debug_inject_mask() & ::ipmz::IPMZ_DEBUG_TRACE) {        \
      fprintf(stderr, "[ipmz] " __VA_ARGS__);                            \
      fputc('\n', stderr);                                              \
      fflush(stderr);                                                    \
    }                                                                    \
  } while (0)
int debug_inject_mask();
// cross-stream ordering that a capture on the HIP runtime torch bundles can
// end (ldlt.hip): event records / waits of the factor's look-ahead streams
hipError_t stream_record(hipEvent_t e, hipStream_t s);
hipError_t stream_wait(hipStream_t s, hipEvent_t e);
void set_capture_origin(hipStream_t s);  // the stream a capture began on (nullptr: none)
void set_debug_inject_mask(int mask);
// error words the persistent kernels raise on a spin timeout (sync.h): the
// panel kernel's ctrl[PANEL_ERR_WORD], the solve's ctrl[1]
constexpr int PANEL_ERR_WORD = 2;
constexpr int SOLVE_ERR_WORD = 1;

// Host-side carving of one allocation into a workspace's members, in call
// order, each aligned to 256 bytes.  base == nullptr: sizes only (every take
// returns nullptr, off still advances to the total).
struct Carver {
  char* base;
  int64_t off = 0;
  template <typename T>
  T* take(int64_t count) {  // count elements of T
    char* p = base ? base + off : nullptr;
    off += (count * (int64_t)sizeof(T) + 255) / 256 * 256;
    return reinterpret_cast<T*>(p);
  }
};

// IPMZ_STEP_SKIP_CONVERGED (ipmz.h): the convergence words of a batch as the
// per-QP kernels outside newton.hip take them -- QP 0's SC_CONVERGED and the
// elements between two QPs' scalar blocks; conv == nullptr: nobody skips.  A
// kernel asks skips(its QP) first of all and returns when it holds: the word
// was written by an earlier launch, so every workgroup of a QP reads the same.
struct SkipGate {
  const double* conv = nullptr;
  int64_t sScal = 0;
  __device__ __forceinline__ bool skips(int64_t qp) const { return conv && conv[qp * sScal] != 0.0; }
};

// ldlt.hip -------------------------------------------------------------------
// Batched factorization: element strides between consecutive QPs' K, D,
// L^{-1} blocks and W panels.
struct BatchStrides {
  int B = 1;
  int64_t sK = 0, sD = 0, sL = 0, sW = 0;
  // small batched factor: B * IPMZ_PAIR_FLAGS + 1 words for the two-workgroup
  // factor (B <= #CU; W then needs 2 x N x 64 per QP), nullptr = one workgroup
  unsigned* pflags = nullptr;
  // small batched factor: the assembled KKT's first touch (block column 0's
  // steps) read from K0 (strides sK) instead of K -- the off-diagonal part
  // kept across Newton steps, only its diagonal rewritten per step; nullptr =
  // K holds the assembled matrix
  const double* K0 = nullptr;
  // small batched factor: IPMZ_BATCH_FACTOR_* (ipmz.h)
  int small_kernel = 0;
  // small batched factor: the QPs that take no part (their K, D, L^{-1} keep
  // their bits; info is then the minimum over the QPs that were factored)
  SkipGate skip;
};
#define IPMZ_PAIR_FLAGS 32  // per QP: LW[16], DONE[16] (N <= IPMZ_SMALL_NMAX)
// the batched factor of order N runs two workgroups per QP (given flags)
bool small_pair_eligible(int B, int N);
bool small_pair_used(int kern, bool have_flags, int B, int N);
// small.hip: whole factor per workgroup (N <= IPMZ_SMALL_NMAX, nbi = 64;
// W: N x 64 per QP)
#define IPMZ_SMALL_NMAX 1024
hipError_t ldlt_factor_small_batched(double* K, int64_t ld, int N, double* D, double* Linv, double* W, int* info,
                                     hipStream_t st, const BatchStrides& bs);
hipError_t ldlt_factor_small_variant(int snw, double* K, int64_t ld, int N, double* D, double* Linv, double* W,
                                     int* info, hipStream_t st, const BatchStrides& bs);  // kbench only
hipError_t ldlt_factor_batched(double* K, int64_t ld, int N, double* D, double* Linv, double* W, int nbo, int nbi,
                               int* info, hipStream_t st, const BatchStrides& bs);
// In-place blocked LDL^T of the lower triangle of K (row-major, ld).
// Linv: (ceil(N/nbi)) blocks of nbi x nbi (inverse unit-lower diagonal
// blocks, consumed by ldlt_solve); W: N x nbo workspace.  info: device int,
// preset to INT_MAX-ish; receives min(1-based index of a non-finite pivot).
// trailing updates of order <= this run on 64 x 64 tiles, larger ones on the
// 128 x 128 kernel (the one TrailTimer times: the roofline kernel of bench.py)
#define IPMZ_TRAIL_SMALL_M 3072
struct TrailTimer {  // HIP-event pairs around every dominant trailing-update launch
  hipEvent_t (*pairs)[2] = nullptr;
  int cap = 0, used = 0;
  double flops = 0.0;
  hipEvent_t* next() { return used < cap ? pairs[used++] : nullptr; }
};
// Look-ahead when st2 (and, for the panel path, st3) and ev (>= 4 *
// ceil(N/nbo) + 2 events) are given; W must then hold 3 * N * nbo doubles
// (else N * nbo).  pctrl: panel_ctrl_words(N, nbo) zeroed words for the
// panel path of panel.hip (nbi == 64); nullptr selects the diag / TRSM /
// strip kernel chain.
// Work of the caller's that the look-ahead factor places in its two idle
// edges (it knows nothing about that work; the Newton step's: capi.cpp
// factor_impl).  Needs one event more: nev >= 5 * ceil(N/nbo) + 4.
//   before_b: enqueued on stream B after everything the caller enqueued on st
//     and before B's first update.  It may write columns >= nbo of K (the first
//     panel reads none of them); every other stream waits for it before its
//     first touch of those columns.  The single-stream factor calls it on st
//     before anything else.
//   rows_final: called once with `final_st` made to wait until the rows
//     < final_rows of L, D and the L^{-1} blocks are final, at the first outer
//     panel whose completion makes them so; `fired` then.  The caller joins
//     final_st back to st after the factor.  Not called by the single-stream
//     factor, nor with final_rows <= 0.
struct FactorHooks {
  std::function<hipError_t(hipStream_t)> before_b;
  int final_rows = 0;
  hipStream_t final_st = nullptr;
  std::function<hipError_t(hipStream_t)> rows_final;
  bool fired = false;
};
hipError_t ldlt_factor(double* K, int64_t ld, int N, double* D, double* Linv, double* W, int nbo, int nbi,
                       int* info, hipStream_t st, TrailTimer* timer = nullptr, hipStream_t st2 = nullptr,
                       hipStream_t st3 = nullptr, hipEvent_t* ev = nullptr, int nev = 0, unsigned* pctrl = nullptr,
                       hipStream_t st4 = nullptr, FactorHooks* hooks = nullptr);
// the same blocked LDL^T in fp32 (fp32 MFMA trailing update): the factor of
// the mixed-precision solve (C5)
hipError_t ldlt_factor(float* K, int64_t ld, int N, float* D, float* Linv, float* W, int nbo, int nbi, int* info,
                       hipStream_t st, TrailTimer* timer, hipStream_t st2, hipStream_t st3, hipEvent_t* ev, int nev,
                       unsigned* pctrl = nullptr, hipStream_t st4 = nullptr);
// ctrl words of the panel path: a shared area (sticky error word) + one
// area per outer panel, then three 64 x 64 (8-byte) tiles: the next panel's
// block (0, 0) look-ahead update, pre-accumulated by the rows launch (three,
// so a rows launch never waits for the chain launch that read the slot it
// reuses)
#define IPMZ_PANEL_PRE00_WORDS (3 * 64 * 64 * 2)
inline int64_t panel_ctrl_words(int N, int nbo) {
  return (int64_t)IPMZ_PANEL_CTRL_WORDS * (1 + (N + nbo - 1) / nbo) + IPMZ_PANEL_PRE00_WORDS;
}
// one outer panel [k0, k0 + bo) of the panel path (panel.hip): the chain
// launch on st_chain, the rows launch on st_rows (flags in `area`, sticky
// error word `err`).  Lb0: L^{-1} block of the panel's first inner block; Wp:
// the panel's W buffer (N x ldw, row-indexed).  Wprev != nullptr: the chain
// launch first applies the look-ahead update with the previous panel
// [kprev, kprev + boprev) (W_prev rows, ld ldw) to the panel's diagonal
// region (and, rows_prev, the rows launch to its rows).
hipError_t panel_factor(double* K, int64_t ld, int N, int k0, int bo, double* D, double* Lb0, double* Wp, int ldw,
                        const double* pre00_in, double* pre00_out,
                        int* info, unsigned* area, unsigned* err, const double* Wprev, int kprev, int boprev,
                        bool rows_prev, hipStream_t st_chain, hipStream_t st_rows,
                        const unsigned* parea = nullptr, bool wait_ready = false);
hipError_t panel_factor(float* K, int64_t ld, int N, int k0, int bo, float* D, float* Lb0, float* Wp, int ldw,
                        const float* pre00_in, float* pre00_out,
                        int* info, unsigned* area, unsigned* err, const float* Wprev, int kprev, int boprev,
                        bool rows_prev, hipStream_t st_chain, hipStream_t st_rows,
                        const unsigned* parea = nullptr, bool wait_ready = false);
// wait_ready: the chain roles of the panel's chain launch first wait for the
// panel's READY-TO-FACTOR word, raised by panel_ready on the stream of the
// look-ahead update the panel's columns needed last (instead of a
// cross-stream wait before that launch), then acquire (agent scope)
hipError_t panel_ready(unsigned* area, hipStream_t st);
// batch systems behind one launch: L and Linv of consecutive systems sL and sLinv elements apart
hipError_t linv_from_l(const double* L, int64_t ld, int N, int nbi, double* Linv, hipStream_t st, int batch = 1,
                       int64_t sL = 0, int64_t sLinv = 0);
hipError_t gemm_nt_sub(int M, int N, int Kd, const double* A, int64_t lda, const double* B, int64_t ldb,
                       double* C, int64_t ldc, int64_t row0, int64_t col0, bool square_lower, hipStream_t st,
                       const BatchStrides* bs = nullptr);

// trsv.hip -------------------------------------------------------------------
// In-place b <- L^{-T} D^{-1} L^{-1} b; side: 2*nbi doubles of scratch.
hipError_t ldlt_solve(const double* K, int64_t ld, int N, const double* D, const double* Linv, int nbi, double* b,
                      double* side, hipStream_t st);

// trsm.hip: the same solve for nrhs right-hand sides at once.  B: nrhs rows of
// length N (row r = right-hand side r, stride ldb >= N), solved in place;
// blocked over column panels of width w (a multiple of 128, <=
// IPMZ_TRSM_PANEL_MAX) on fp64 / fp32 MFMA.  Stream-ordered launches only: no
// cross-workgroup waiting.  Instantiated for
//   double  the fp64 factor (nbi 64 or 128): ld and ldb even, K and B 16-byte
//           aligned;
//   float   the fp32 factor of the mixed-precision path (nbi == 64): ld a
//           multiple of 64, ldb of 4, K / Linv / B 16-byte aligned.
#define IPMZ_TRSM_PANEL_MAX 512
// A batch of B systems of one order behind the same launches (fp64 only): a
// grid dimension is the system, and K, D, Linv and the right-hand sides of
// consecutive systems lie sK, sD, sL and sB elements apart (sK, sL, sB even:
// the 16-byte loads).  The default is one system.
struct TrsmBatch {
  int B = 1;
  int64_t sK = 0, sD = 0, sL = 0, sB = 0;
  int64_t sG = 0;  // trsm_sweep's gate: words between consecutive systems' gate words (0: one word for all)
};
template <typename T>
hipError_t ldlt_solve_multi(const T* K, int64_t ld, int N, const T* D, const T* Linv, int nbi, T* B, int64_t ldb,
                            int nrhs, int w, hipStream_t st, const TrsmBatch& tb = TrsmBatch());

// one of its sweeps alone: forward B <- B L^{-T}, backward B <- B L^{-1} (the
// middle stage is the caller's; same argument rules).  gate (device word, may
// be null): when set, every launch ends at once if *gate != 0 -- per system of
// a batch when tb.sG != 0 (system q reads gate[q * tb.sG])
template <typename T>
hipError_t trsm_sweep(const T* K, int64_t ld, int N, const T* Linv, int nbi, T* B, int64_t ldb, int nrhs, int w,
                      bool backward, hipStream_t st, const unsigned* gate, const TrsmBatch& tb = TrsmBatch());

// The whole fp64 solve of small systems in ONE launch: a workgroup keeps 16
// right-hand sides of one system in LDS through the forward sweep, the division
// by D and the backward sweep (B read once and written once, L once per sweep).
// Eligible when the 16 x round_up(N, nbi) slab, T and the stage buffers fit
// the LDS of a workgroup on this device; same argument rules as above.
bool ldlt_solve_fused_eligible(int N, int nbi);
hipError_t ldlt_solve_fused(const double* K, int64_t ld, int N, const double* D, const double* Linv, int nbi,
                            double* B, int64_t ldb, int nrhs, hipStream_t st, const TrsmBatch& tb = TrsmBatch());

// one workgroup per QP of a batch (small N); b: batch of rhs, stride sb
// skip: the QPs whose b keeps its bits
hipError_t ldlt_solve_batched(const double* K, int64_t ld, int N, const double* D, const double* Linv, int nbi,
                              double* b, int B, int64_t sK, int64_t sD, int64_t sL, int64_t sb, hipStream_t st,
                              const SkipGate& skip = SkipGate());

// trsv_persist.hip: the same solve as ONE persistent launch on 128-row
// blocks (nbi == 64 factors).  P: solve_prep_elems(N) elements written by
// solve_prep from the factor's 64 x 64 inverses (once per factorization);
// ybuf, xbuf: solve_vec_elems(N) elements each (the block vectors, then the
// slices the parts of a split block exchange); ctrl: IPMZ_SOLVE_CTRL_WORDS
// unsigned, all set up by solve_reset once per factorization
// (ctrl[SOLVE_ERR_WORD] is sticky).
int64_t solve_prep_elems(int N);
int64_t solve_vec_elems(int N);
// the persistent solve's state after a factorization: control words zero,
// y / x buffers (solve_vec_elems(N) elements of size elem) all-ones sentinels; the solve
// launches keep it so for the next solve.  Optionally in the same launch:
// info / info2 words set to 0x7f7f7f7f ("no failed pivot") and nwords words
// zeroed (a factor's panel ctrl words)
hipError_t solve_reset(void* ybuf, void* xbuf, size_t elem, int N, unsigned* ctrl, hipStream_t st,
                       int* info = nullptr, unsigned* words = nullptr, int64_t nwords = 0, int* info2 = nullptr);
hipError_t solve_stamps(unsigned long long* out);  // DEBUG
hipError_t chain_stamps(unsigned long long* c, unsigned long long* h);  // DEBUG (-DIPMZ_CHAIN_STAMPS)
hipError_t solve_prep(const double* K, int64_t ld, int N, const double* Linv, double* P, hipStream_t st);
hipError_t solve_prep(const float* K, int64_t ld, int N, const float* Linv, float* P, hipStream_t st);
hipError_t ldlt_solve_persistent(const double* K, int64_t ld, int N, const double* D, const double* P, double* b,
                                 double* ybuf, double* xbuf, unsigned* ctrl, hipStream_t st);
// The same preparation and solve in two parts around R rows (a multiple of
// 128, 0 < R < N) that are final before the rest of the factor is:
//   head: the operators that read only rows < R (X_J, M_J of the block rows
//     below R and Q_J of all but the last of them), then the forward sweep
//     over the leading R rows of b -- the leading principal block of the
//     forward substitution, the same arithmetic;
//   tail (after the factor and the head): the other operators; then
//     ldlt_solve_persistent_tail: the forward sweep over the block rows from
//     R / 128 on (their bulk sums over all earlier blocks, as ever), and the
//     backward sweep.
// Every element goes through the operations of the unsplit calls in the same
// order (the parts per block are those of the whole N): bitwise alike.
hipError_t solve_prep_split(const double* K, int64_t ld, int N, const double* Linv, double* P, int R, bool head,
                            hipStream_t st);
hipError_t ldlt_solve_persistent_head(const double* K, int64_t ld, int N, const double* D, const double* P,
                                      const double* b, double* ybuf, double* xbuf, unsigned* ctrl, int R,
                                      hipStream_t st);
hipError_t ldlt_solve_persistent_tail(const double* K, int64_t ld, int N, const double* D, const double* P, double* b,
                                      double* ybuf, double* xbuf, unsigned* ctrl, int R, hipStream_t st);
// one sweep (forward: ybuf = L^{-1} b; backward: b = L^{-T} (ybuf / D)); skip
// (device flag, may be null): return at once when set
hipError_t ldlt_solve_persistent_sweep(const double* K, int64_t ld, int N, const double* D, const double* P,
                                       double* b, double* ybuf, double* xbuf, unsigned* ctrl, bool backward,
                                       hipStream_t st, const unsigned* skip);
// fp32 variant; skip (device flag, may be null): return at once when set
hipError_t ldlt_solve_persistent(const float* K, int64_t ld, int N, const float* D, const float* P, float* b,
                                 float* ybuf, float* xbuf, unsigned* ctrl, hipStream_t st,
                                 const unsigned* skip = nullptr);

// mixed.hip: fp32 factor of S K S + fp64 iterative refinement (config C5) ----
struct MixedWs {
  int N = 0, nbo = 256;
  int64_t ld32 = 0;
  float *K32 = nullptr, *D32 = nullptr, *Linv32 = nullptr, *W32 = nullptr, *P32 = nullptr;
  float *y32 = nullptr, *z32 = nullptr, *r32 = nullptr;
  unsigned *ctrl = nullptr, *state = nullptr, *pctrl = nullptr;
  int* info = nullptr;
  double *s = nullptr, *x = nullptr, *colp = nullptr, *rowp = nullptr, *part = nullptr;
  double* stat = nullptr;  // {||r||_inf / ||b||_inf, corrections} of the last solve
  // host-mapped {done, corrections} written by the stop test, and the event
  // the host waits on before reading it (eager solves only: mixed_solve)
  unsigned *hst = nullptr, *hst_dev = nullptr;
  hipEvent_t hev = nullptr;
  int last_iters = 2;  // refinement passes the previous eager solve ran
};
int64_t mixed_ws_bytes(int N, int nbo);
int64_t mixed_ws_carve(char* base, int N, int nbo, MixedWs& w);  // base == nullptr: size only
// scale + convert + fp32 factor of the lower triangle of K (fp64, row-major)
hipError_t mixed_factor(const double* K, int64_t ld, MixedWs& w, hipStream_t st, hipStream_t st2, hipStream_t st3,
                        hipEvent_t* ev, int nev, TrailTimer* timer = nullptr, hipStream_t st4 = nullptr);
// b <- K^{-1} b by iterative refinement (device-side stop test)
hipError_t mixed_solve(const double* K, int64_t ld, MixedWs& w, double* b, double tol, int max_refine,
                       hipStream_t st);

// mixed_multi.hip: the refinement of mixed_solve for nrhs right-hand sides
// (rows of B) around the blocked fp32 solve, per-row stop test, frozen rows
struct MixedMultiWs {
  int64_t ldx = 0, ld32 = 0;
  int ntiles = 0;
  double* x = nullptr;       // nrhs x ldx: the solutions
  float* r32 = nullptr;      // nrhs x ld32: the fp32 right-hand sides / corrections
  double* part = nullptr;    // nrhs x ntiles x {max|r|, max|b|}
  double* stat = nullptr;    // nrhs x {ratio reached, corrections applied}
  unsigned* done = nullptr;  // nrhs: the row is frozen
  unsigned* word = nullptr;  // every row is frozen
};
int64_t mixed_multi_ws_carve(char* base, int N, int nrhs, MixedMultiWs& m);  // base == nullptr: size only
// rows of B <- K^{-1} row; blocks the host (reads the all-stopped word after
// every pass); pw: panel width of the fp32 solve.  ld even, K 16-byte aligned.
hipError_t mixed_solve_multi(const double* K, int64_t ld, const MixedWs& w, const MixedMultiWs& m, double* B,
                             int64_t ldb, int nrhs, double tol, int max_refine, int pw, hipStream_t st);
// R = B - X K, K symmetric from its lower triangle (fp64 MFMA); R may alias B.
// ld, ldx even, K and X 16-byte aligned.
hipError_t sym_residual_multi(const double* K, int64_t ld, int N, const double* X, int64_t ldx, const double* B,
                              int64_t ldb, double* R, int64_t ldr, int nrhs, hipStream_t st);

// normal.hip: normal-equations reduction (config C2) -------------------------
hipError_t ne_check_sign(const double* D, int N, int offset, double sign, int* info, hipStream_t st);


// bk.hip: Bunch-Kaufman factor / solve (one workgroup per matrix) -----------
#ifndef IPMZ_BK_NMAX  // (include/ipmz.h publishes the same limit for the batch entry points)
#define IPMZ_BK_NMAX 4096
#endif
// skip: the systems of the batch that take no part (factor, pivots, info word and b keep their bits)
hipError_t bk_factor(double* A, int64_t ld, int n, int* ipiv, int* info, int fix_kp, int batch, int64_t sA,
                     int64_t sP, hipStream_t st, const SkipGate& skip = SkipGate());
hipError_t bk_solve(const double* F, int64_t ld, int n, const int* ipiv, double* b, int batch, int64_t sA, int64_t sP,
                    int64_t sb, hipStream_t st, const SkipGate& skip = SkipGate());
// the whole-device factor of ONE matrix (any n; one workgroup per CU, a grid
// barrier per step): workspace bytes, launch, and its sticky error word
// (nonzero after a barrier spin timed out -- the factor is then invalid)
#define IPMZ_BK_GRID_MIN 512  // auto: the grid factor from this order up (single matrices)
size_t bk_grid_ws_bytes(int n);
hipError_t bk_factor_grid(double* A, int64_t ld, int n, int* ipiv, int* info, int fix_kp, void* ws, hipStream_t st);
const unsigned* bk_grid_err_word(const void* ws, int n);
// A transposed copy of the factor's lower triangle (LT: n x n doubles, row j =
// column j of L; bk_transpose once per factor): the device-wide solve's input
// and its fallbacks' factor (coalesced sweeps, the same arithmetic as bk_solve).
// A batch of B systems of one order behind the prepared solve's launches (the
// system is a grid dimension): the factors, pivots, LT, L' and right-hand
// sides of consecutive systems lie sA, sP, sLT, sLp and sB elements apart;
// the bookkeeping (meta) of system q starts bk_fast_meta_bytes(n) * q bytes
// into meta, with a fallback flag of its own.  The default is one system.
struct BkBatch {
  int B = 1;
  int64_t sA = 0, sP = 0, sLT = 0, sLp = 0, sB = 0;
};
hipError_t bk_transpose(const double* F, int64_t ld, int n, double* LT, hipStream_t st,
                        const BkBatch& bb = BkBatch());
// Device-wide solve: A^{-1} b = P^T L'^{-T} D^{-1} L'^{-1} P b, L' = L with every
// later interchange folded into its columns (once per factor, bk_fast_prepare:
// from F, ipiv, the factor's info word and LT = bk_transpose(F); LT is
// permuted in place, L' written to the strict lower triangle of Lp, which may
// be F itself; meta: bk_fast_meta_bytes).  Then the persistent solve's
// operators are built from Lp (linv_from_l, solve_prep, solve_reset) and a
// solve is gather -> forward sweep -> dsolve (ybuf) -> backward sweep (D =
// ones) -> scatter, all gated on meta's fallback flag, + bk_fast_fallback
// (the one-workgroup sweeps on the untouched LT, run only when the flag is
// set: a singular factor, or n > 16384).
size_t bk_fast_meta_bytes(int n);
const unsigned* bk_fast_flag(const void* meta);
const double* bk_fast_ones(const void* meta, int n);
double* bk_fast_tmp(void* meta, int n);
hipError_t bk_fast_prepare(const double* F, int64_t ld, int n, const int* ipiv, const int* info, double* LT,
                           double* Lp, int64_t ldp, void* meta, hipStream_t st, const BkBatch& bb = BkBatch());
hipError_t bk_fast_gather(const double* b, int n, void* meta, hipStream_t st);
hipError_t bk_fast_dsolve(double* y, int n, void* meta, hipStream_t st);
hipError_t bk_fast_scatter(double* b, int n, void* meta, hipStream_t st);
hipError_t bk_fast_fallback(const double* LT, int n, const int* ipiv, double* b, const void* meta, hipStream_t st);
// The same solve for the nrhs rows of B (stride ldb, even; B 16-byte aligned),
// in place: bk_multi_gather -> trsm_sweep forward on L' (gate = the fallback
// flag) -> bk_multi_dsolve -> trsm_sweep backward -> bk_multi_scatter, then
// bk_multi_fallback (one launch, a workgroup per row, run only when the flag
// is set).  Stream-ordered, nothing waits across workgroups; columns
// [n, ldb) of B are never written.
hipError_t bk_multi_gather(double* B, int64_t ldb, int nrhs, int n, void* meta, hipStream_t st,
                           const BkBatch& bb = BkBatch());
hipError_t bk_multi_dsolve(double* B, int64_t ldb, int nrhs, int n, void* meta, hipStream_t st,
                           const BkBatch& bb = BkBatch());
hipError_t bk_multi_scatter(double* B, int64_t ldb, int nrhs, int n, void* meta, hipStream_t st,
                            const BkBatch& bb = BkBatch());
hipError_t bk_multi_fallback(const double* LT, int n, const int* ipiv, double* B, int64_t ldb, int nrhs,
                             const void* meta, hipStream_t st);
// What the one-launch solve of trsm.hip reads of the bookkeeping (system 0's;
// system q's lies sM bytes x q further): the fallback flag, the composite
// interchange, the pivot kinds (0 = 1x1, 1 / 2 = first / second row of a 2x2)
// and the pivot blocks of D
struct BkFusedMeta {
  const unsigned* flag;
  const int *perm, *kind;
  const double *d11, *d21, *d22;
  int64_t sM;
  __host__ __device__ BkFusedMeta of(unsigned q) const {
    const int64_t o = (int64_t)q * sM;
    auto adv = [o](auto* p) { return reinterpret_cast<decltype(p)>(reinterpret_cast<const char*>(p) + o); };
    return {adv(flag), adv(perm), adv(kind), adv(d11), adv(d21), adv(d22), sM};
  }
};
BkFusedMeta bk_fused_meta(const void* meta, int n, const BkBatch& bb);
// The whole prepared solve of small systems in ONE launch per batch
// (trsm_bk_fused_kernel: gather, forward sweep, D solve, backward sweep and
// scatter on a slab that stays in LDS), eligible as ldlt_solve_fused is with
// inner block 64; Lp, Linv as trsm_sweep's K, Linv (tb.sK, tb.sL), tb.sB the
// systems' right-hand sides.  Flagged systems are skipped (bk_multi_fallback_batch).
bool bk_solve_fused_eligible(int N);
hipError_t bk_solve_fused(const double* Lp, int64_t ldp, int N, const double* Linv, double* B, int64_t ldb, int nrhs,
                          const BkFusedMeta& m, hipStream_t st, const TrsmBatch& tb);
// the batch's fallback: one workgroup per (system, row), the reference's
// interleaved sweeps on that system's LT, run only where the system's flag is set
hipError_t bk_multi_fallback_batch(const double* LT, int n, const int* ipiv, double* B, int64_t ldb, int nrhs,
                                   const void* meta, hipStream_t st, const BkBatch& bb);

// newton.hip -----------------------------------------------------------------
enum Slot { X = 0, LA, LC, S, P, LG, LH, LY, LZ, G, H, Y, Z, NSLOT };

// device scalar block
enum Scalar {
  SC_F = 0,
  SC_RES,
  SC_MU,
  SC_ALPHA_AFF,
  SC_MU_AFF,
  SC_SIGMA,
  SC_ALPHA,
  SC_CONVERGED,
  SC_MU_NEW,
  SC_RESTARTS,
  SC_STEPS = 14,  // IPMZ_SC_STEPS: the steps with IPMZ_STEP_SKIP_CONVERGED this QP took part in
  SC_COUNT = 16
};

struct QPDev {
  int n, m, p;
  int N;
  int64_t ldn;  // leading dimension of Q, A, C (multiple of 8)
  int64_t ldk;  // leading dimension of K
  int64_t state_len;
  double delta;
  int eqnone;  // EqualityHandling::None: no p, zero (lambda_C, lambda_C) block
  int eqpen;   // EqualityHandling::PenaltyFunction: no p, -mu (lambda_C, lambda_C) block
  // Settings (oracle/ipmz_oracle.cpp QP): InequalityHandling::Slacks, and the
  // Lower / Upper halves of Settings::variable_bounds and ::inequalities
  int slacks, vlo, vup, alo, aup;
  int naive;  // InequalityHandling::NaiveSlacks: no s / lambda_A; lambda_g, lambda_h are KKT rows
  // EqualityHandling::SlackedSlacks: the p equality rows run as inequality
  // rows with l = u = d (m = m_usr + p_usr, p = 0 inside the step; the
  // formulas are the same, formulations.txt), t starting at 1
  // (EnvironmentBuilder.cpp: s_A_eq = 1).  m_usr / p_usr: the data's rows.
  int eqss, m_usr, p_usr;
  int mk;     // KKT rows of the inequalities: m, or 2 m (NaiveSlacks); N = n + mk + p
  // problem data (row-major, ld = ldn)
  const double *Q, *c, *A, *lA, *uA, *C, *d, *lx, *ux;
  double* v[NSLOT];
  double* r[NSLOT];
  double* daff[NSLOT];
  double* dir[NSLOT];
  double *Qx, *ATl, *CTl, *Ax, *Cx;
  double* b;      // augmented rhs / solution, length N
  double* scal;   // SC_COUNT doubles
  double* part;   // reduction partials
  double* tpart;  // transposed-GEMV partials: ceil(max(m, p) / IPMZ_TCHUNK) x n
  double* K;      // KKT / factor (N x ldk)
  double* K0;     // batches of small systems: the assembled KKT kept across steps (the factor reads it, writes L to K); nullptr: none
  double *v0, *r0, *scal0;  // initial iterate snapshot (benchmark restarts)
  double* Cx0;              // ... and its C x, which PenaltyFunction's corrector row reads (corrector_elem)
  unsigned* done;           // fused evaluation: arrival counter of the QP's workgroups (0 between launches)
};

// Elements the step's O(N) passes walk (element t of a pass: the *_elem functions of newton.hip).  Every launcher's
// grid and every kernel's loop takes its bound from these; the KKT rows n + mk + p = N are another quantity.
__host__ __device__ __forceinline__ int residual_rows(const QPDev& q) { return q.n + q.m + q.p; }  // residual_elem
__host__ __device__ __forceinline__ int comp_rows(const QPDev& q) { return q.n + q.m; }  // ratio_elem, mu_aff_elem
__host__ __device__ __forceinline__ int corrector_rows(const QPDev& q) {  // corrector_elem: PenaltyFunction's r_lambda_C too
  return comp_rows(q) + (q.eqpen ? q.p : 0);
}
__host__ __device__ __forceinline__ int update_rows(const QPDev& q) {  // update_elem: t indexes the n, m and p blocks at once
  const int mp = q.m > q.p ? q.m : q.p;
  return q.n > mp ? q.n : mp;
}

// EqualityHandling::SlackedSlacks / NaiveSlacks run the p_usr equality rows as inequality rows, so the step's slots
// hold [lambda_g lambda_v], [lambda_h lambda_w], [g v], [h w] while the reference's Newton order is lambda_g,
// lambda_h, lambda_v, lambda_w, ..., g, h, v, w (formulations.txt).  eqss_source(k, q): the step-vector index of
// reference-order element k, from the segment lengths alone -- the one statement of the map, for the device gather
// (io.hip) and the host read-back and load (qp.cpp).
__host__ __device__ __forceinline__ int64_t eqss_block(int64_t k, int64_t m, int64_t p) {
  const int64_t mp = m + p;                      // in: [a m][b m][a' p][b' p]; stored: [a m a' p][b m b' p]
  if (k < m) return k;                           // a
  if (k < 2 * m) return mp + (k - m);            // b
  if (k < 2 * m + p) return m + (k - 2 * m);     // a'
  return mp + m + (k - 2 * m - p);               // b'
}
__host__ __device__ __forceinline__ int64_t eqss_source(int64_t k, const QPDev& q) {
  const int64_t n = q.n, m = q.m_usr, p = q.p_usr, mp = m + p;
  const int64_t duals = q.naive ? n : n + 2 * mp;  // after x (NaiveSlacks) or x, [lambda_A lambda_C], [s t]
  if (k < duals) return k;
  if (k < duals + 2 * mp) return duals + eqss_block(k - duals, m, p);
  const int64_t slacks = duals + 2 * mp + (q.vlo ? n : 0) + (q.vup ? n : 0);  // after lambda_y, lambda_z
  if (k < slacks) return k;
  if (k < slacks + 2 * mp) return slacks + eqss_block(k - slacks, m, p);
  return k;  // y, z
}

// The order the slots lie in within one contiguous step vector (qp.cpp carve: v[X] is its base and the slot pointers
// ascend in this order, absent slots having length 0): the enum's, except that NaiveSlacks puts its duals lambda_g,
// lambda_h ahead of lambda_C (formulations.txt).
__host__ __device__ __forceinline__ int slot_in_order(bool naive, int k) {
  constexpr int naive_order[NSLOT] = {X, LG, LH, LC, P, LY, LZ, G, H, Y, Z, LA, S};
  return naive ? naive_order[k] : k;
}
// What ratio_elem (newton.hip) holds an iterate to, stated once for the warm start's push and check (io.hip): the
// slots it keeps non-negative -- lambda_g, lambda_h, lambda_y, lambda_z and, where they are Newton variables, g, h,
// y, z: the enum's tail -- and the explicit bounds l_x < x < u_x, l_A < s < u_A it applies when neither g nor h is one.
__host__ __device__ __forceinline__ bool nonneg_slot(int slot) { return slot >= LG; }
__host__ __device__ __forceinline__ bool explicit_bounds(const QPDev& q) { return q.slacks || q.m == 0; }

// A batch of QPs with identical (n, m, p): d = device array of B
// descriptors (kernels index it with blockIdx.y), h = host copy of QP 0.
// skip != 0 (a copy of the batch made for one step with IPMZ_STEP_SKIP_CONVERGED): in the fused per-QP phases below
// a QP whose SC_CONVERGED is set returns at the top of the kernel -- before any barrier, LDS use or arrival counter
// -- and keeps every bit; the pre phase counts the others' SC_STEPS
struct QPBatch {
  const QPDev* d;
  QPDev h;
  int B;
  int skip = 0;
};

hipError_t qp_generate(const QPBatch& qb, uint64_t seed0, hipStream_t st);  // QP b: seed0 + b
hipError_t qp_init_iterate(const QPBatch& qb, hipStream_t st);
// residual vectors of the current iterate at mu = 0, plus f, res, mu,
// converged into scal (the head of Optimizer.cpp:127-135)
hipError_t qp_evaluate(const QPBatch& qb, hipStream_t st);
hipError_t qp_assemble(const QPBatch& qb, hipStream_t st);
// ... in two launches that together write what qp_assemble writes: head = columns < c, else columns >= c
hipError_t qp_assemble_cols(const QPBatch& qb, int c, bool head, hipStream_t st);
// predictor / corrector pieces; which: 0 = affine direction, 1 = corrector
hipError_t qp_rhs(const QPBatch& qb, hipStream_t st);
hipError_t qp_backsub(const QPBatch& qb, int which, hipStream_t st);
hipError_t qp_ratio(const QPBatch& qb, int which, int out_index, hipStream_t st);
// The same three for a block of residual vectors per QP (ipmz_*_newton_solve_multi):
// row r of QP z of R (at R + z sR + r ldr, Newton order) -> its augmented rhs
// in row r of W; the solved W and R -> the full direction in row r of D (may
// be R, same strides); get_max_step_ of every row -> alpha[z nrhs + r].
// IPMZ_NEWTON_MULTI_RPG: rows one thread takes at once (one row group of the grid).
#define IPMZ_NEWTON_MULTI_RPG 4
hipError_t qp_rhs_multi(const QPBatch& qb, const double* R, int64_t ldr, int64_t sR, double* W, int64_t ldw, int64_t sW,
                        int nrhs, hipStream_t st);
hipError_t qp_backsub_multi(const QPBatch& qb, const double* R, int64_t ldr, int64_t sR, const double* W, int64_t ldw,
                            int64_t sW, double* D, int64_t ldd, int64_t sD, int nrhs, hipStream_t st);
hipError_t qp_ratio_multi(const QPBatch& qb, const double* D, int64_t ldd, int64_t sD, double* alpha, int nrhs,
                          hipStream_t st);
// The transposed map of the first two (ipmz_*_newton_adjoint_multi), same grid and row groups: row r of QP z of
// Cot (the caller's G: a cotangent of a direction, Newton order) -> E^T g in row r of W; the solved W and Cot ->
// M^T g in row r of Out (may be Cot, same strides), every slot the formulation has.
hipError_t qp_adj_reduce_multi(const QPBatch& qb, const double* Cot, int64_t ldg, int64_t sG, double* W, int64_t ldw,
                               int64_t sW, int nrhs, hipStream_t st);
hipError_t qp_adj_expand_multi(const QPBatch& qb, const double* Cot, int64_t ldg, int64_t sG, const double* W,
                               int64_t ldw, int64_t sW, double* Out, int64_t ldo, int64_t sO, int nrhs, hipStream_t st);
hipError_t qp_mu_aff(const QPBatch& qb, hipStream_t st);
hipError_t qp_corrector_residuals(const QPBatch& qb, hipStream_t st);
hipError_t qp_update(const QPBatch& qb, int freeze, hipStream_t st);
hipError_t qp_restart_if_converged(const QPBatch& qb, hipStream_t st);
hipError_t qp_save_initial(const QPBatch& qb, hipStream_t st);
// out (device, 3 doubles) = {max res, max mu, unconverged count} over the batch
hipError_t qp_batch_summary(const QPBatch& qb, double* out, hipStream_t st);
// Fused per-QP phases for batches of small systems (one workgroup per QP):
// pre = restart-if-converged + assembly + affine rhs (+ info word reset),
// mid = predictor back-substitution .. corrector rhs, post = corrector
// back-substitution + update + evaluation.  N <= IPMZ_FUSED_NMAX.
#define IPMZ_FUSED_NMAX 1024
// kmode: 0 = the whole lower triangle into K; 1 = the diagonal into K0 (its
// off-diagonal part is already there); 2 = only the off-diagonal part into
// K0 (once per data load; no restart, no rhs)
enum { KMODE_K = 0, KMODE_K0_DIAG = 1, KMODE_K0_OFFDIAG = 2 };
hipError_t qp_fused_pre(const QPBatch& qb, int restart, int* info, hipStream_t st, int kmode = KMODE_K);
hipError_t qp_fused_mid(const QPBatch& qb, hipStream_t st);
hipError_t qp_fused_post(const QPBatch& qb, int freeze, hipStream_t st);  // (+ the evaluation)
// predictor solve + mid + corrector solve + post in one workgroup per QP
// (the small batched solve, ldlt_solve_batched's nbi = 64 path: N <=
// TRSV_SMALL_NMAX, even ld), then the evaluation alone
inline bool fused_solves_ok(int N, int64_t ld) { return N <= 4096 && !(ld & 1); }
hipError_t qp_fused_solves(const QPBatch& qb, const double* K, int64_t ld, int N, const double* D, const double* Linv,
                           double* b, int64_t sK, int64_t sD, int64_t sL, int64_t sb, int freeze, hipStream_t st);
hipError_t qp_fused_eval(const QPBatch& qb, hipStream_t st);
// Centering on the central path (ipmz_batch_center): the solver's small device
// buffer (capi.h center_ws carves it) and the two launch groups the loop adds
// to the Newton-solve path.  nb = qp_center_blocks: the norm's workgroups per QP.
struct CenterWs {
  double* part = nullptr;   // B x nb: the workgroups' partial maxima of |r_v(z; kappa)|
  double* e = nullptr;      // B: the QP's norm at its last test
  double* alpha = nullptr;  // B: the step length of the QP's direction (before the 0.995)
  double* sum = nullptr;    // the host's look: {QPs not centered, the largest e among them}
  int* frozen = nullptr;    // B: 1 from the test the QP passed on
  int* iters = nullptr;     // B: updates the QP received
  int nb = 0;
  int64_t total = 0;
};
int qp_center_blocks(const QPBatch& qb);
// Q x, A x, ... of the iterate, r_v(z; mu = kappa) into the residual slots (the evaluation's own launch), the
// infinity norm over all state_len of them per QP not yet frozen, then one launch: e, the flag raised where
// e <= tol (a NaN never passes), and w.sum
hipError_t qp_center_test(const QPBatch& qb, double kappa, double tol, const CenterWs& w, hipStream_t st);
// z <- z + 0.995 alpha[QP] dir for the QPs not frozen (qp_update's kernel behind its gate), iters[QP] += 1
hipError_t qp_center_update(const QPBatch& qb, const CenterWs& w, hipStream_t st);

// io.hip, grad.hip, jvp.hip ---------------------------------------------------
// The nine blocks of a QP's data as a caller hands them over in device memory (ipmz_qp_device_data, _grad and
// _tangent of the public header), described once for the load, the gradient and the tangents: this index, one row
// of DATA_BLOCKS per block, and one descriptor type.  HELD_*: ipmz_qp::held, a bit per block the solver holds.
enum DataBlock { DB_Q = 0, DB_A, DB_CEQ, DB_C, DB_LX, DB_UX, DB_LA, DB_UA, DB_D, DB_COUNT, DB_MATS = DB_C };
enum : unsigned {
  HELD_Q = 1, HELD_C = 2, HELD_A = 4, HELD_LA = 8, HELD_UA = 16, HELD_CEQ = 32, HELD_D = 64, HELD_LX = 128,
  HELD_UX = 256, HELD_ALL = 511
};
struct DataBlockInfo {
  const char* name;  // as the messages print it
  bool matrix;       // rows of n elements with a row stride; else a vector
  int dim;           // which of the solver's dimensions (0 / 1 / 2: n / m / p) gives its rows, or a vector's length
  unsigned held;
};
constexpr DataBlockInfo DATA_BLOCKS[DB_COUNT] = {
    {"Q", true, 0, HELD_Q},      {"A", true, 1, HELD_A},      {"C", true, 2, HELD_CEQ},
    {"c", false, 0, HELD_C},     {"l_x", false, 0, HELD_LX},  {"u_x", false, 0, HELD_UX},
    {"l_A", false, 1, HELD_LA},  {"u_A", false, 1, HELD_UA},  {"d", false, 2, HELD_D}};
// The blocks of one call (those it does not take -- null, not wanted, or of dimension 0 -- null): block k of QP z,
// tangent t starts at p[k] + z sq[k] + t tq[k], row i of a matrix ld[k] elements further each; strides in elements.
// A QP stride of 0 (batches) is one block for every QP: shared data or tangents, a gradient summed over the batch.
// T: const double for the load and the tangents, double for the gradient; tq: the tangents only (else 0).
// A kernel indexes the members with literal or fully unrolled constants only: a by-value kernel argument indexed
// at run time is copied to scratch.
template <class T>
struct QpBlocks {
  T* p[DB_COUNT];
  int64_t sq[DB_COUNT], tq[DB_COUNT], ld[DB_MATS];
};
typedef QpBlocks<const double> QpBlocksIn;
typedef QpBlocks<double> QpBlocksOut;
// The bound check's verdict word: IPMZ_IO_VALID, or the smallest key of a
// violated bound in the order (QP, l_x < u_x before l_A <= u_A, index)
constexpr unsigned long long IPMZ_IO_VALID = ~0ull;
constexpr unsigned long long io_key(int qp, int kind, int k) {
  return ((unsigned long long)(unsigned)qp << 33) | ((unsigned long long)kind << 32) | (unsigned)k;
}
// build_environment's check (!(l_x < u_x), !(l_A <= u_A): NaN is a violation)
// of the bound pairs of which `in` supplies a side, the other side being the
// solver's; resets and fills *verdict (device).  Independent of scheduling.
hipError_t qp_io_validate(const QPBatch& qb, const QpBlocksIn& in, unsigned long long* verdict, hipStream_t st);
// every supplied block into the solver's storage: exactly the elements the
// host load writes (columns [n, ldn) and the space between QPs keep their bits)
hipError_t qp_io_pack(const QPBatch& qb, const QpBlocksIn& in, hipStream_t st);
// row z of dst (device, row stride ld >= state_len) <- QP z's state `which`
// (IPMZ_STATE_*) in the reference's Newton order; one launch, no allocation
hipError_t qp_gather_state(const QPBatch& qb, int which, double* dst, int64_t ld, hipStream_t st);
// The other direction (ipmz_batch_set_state_device): the iterate of every QP z with take[z] != 0 (take == nullptr:
// every QP) <- row z of src (device, row stride ld >= state_len, the reference's Newton order), each component of a
// slot ratio_elem keeps non-negative raised to at least `floor` on the way.  One launch, no allocation; rows of QPs
// not taken and columns [state_len, ld) are never read.
hipError_t qp_scatter_state(const QPBatch& qb, const double* src, int64_t ld, const int32_t* take, double floor,
                            hipStream_t st);
// The check of those rows after the same push: a NaN anywhere, !(v > 0) in a non-negative slot, or, where
// explicit_bounds holds, x outside (l_x, u_x) or s outside (l_A, u_A) of the data the solver holds.  Resets and fills
// *verdict (device): IPMZ_IO_VALID, or the smallest z * state_len + k of a violating component k (the caller's
// order) of QP z.  Independent of scheduling; writes nothing else.
hipError_t qp_scatter_validate(const QPBatch& qb, const double* src, int64_t ld, const int32_t* take, double floor,
                               unsigned long long* verdict, hipStream_t st);

// grad.hip -------------------------------------------------------------------
// QPs per chunk of the shared matrix blocks' sum over the batch: every chunk's
// partial product is one tile set of the workspace, summed in chunk order
#define IPMZ_VJP_KCHUNK 64
// cotangent rows per QP whose partials the workspace holds at a time (ipmz_batch_data_vjp_multi): the rows of a call
// pass through it in slabs of this many, one slab after the other on the stream
#define IPMZ_VJP_SLAB 16
// elements of that workspace for a call with ncot rows per QP: ceil(B / IPMZ_VJP_KCHUNK) x min(ncot, IPMZ_VJP_SLAB)
// x max(n, m, p) x n (one matrix block and one slab at a time)
int64_t qp_grad_part_elems(const QPBatch& qb, int ncot = 1);
// (d r / d data)^T w of every QP and each of its ncot cotangent rows, w = the
// row at W + z sW + r ldw in the layout of IPMZ_STATE_RES, into the blocks of
// o (row r of QP z of block k at p[k] + z sq[k] + r tq[k]; one row: ldw and tq
// are not looked at); part: the workspace above, read and written only when a
// matrix block is shared (may be null otherwise).  Every row's result has the
// bits of a call with that row alone.  Stream-ordered launches, no atomics;
// reads the iterate and W only
hipError_t qp_data_vjp(const QPBatch& qb, int ncot, const double* W, int64_t ldw, int64_t sW, const QpBlocksOut& o,
                       double* part, hipStream_t st);

// jvp.hip --------------------------------------------------------------------
// gridDim.y of the launches that loop over the rows (q, t) of R
#define IPMZ_JVP_ROWS_GY 16384
// Where one matrix block's products lie in a row's segment of the workspace,
// and how they were cut (jvp.hip's header: the summation order).  mode 0: no
// such block, 1: per-QP tangents, 2: shared.  Row products (dM x): nct partials
// of `rows` doubles at off_row; column products (dM^T y, A and C only): nchunk
// partials of n doubles at off_col (chunks of rch rows).
struct JvpMat {
  int mode, rch, nchunk, nct;
  int64_t off_row, off_col;
};
struct JvpPlan {
  JvpMat mat[3];  // Q, A, C
  int64_t seg;    // doubles per row (q, t); the workspace holds batch * ntan segments
};
// a function of the shape, of which blocks are given and of which are shared -- not of ntan or the batch size
JvpPlan qp_jvp_plan(const QPBatch& qb, const QpBlocksIn& in);
// column pairs per lane of k_jvp_matrix's column tile (128 of them columns each), by n
int jvp_pairs(int n);
// row (z, t) of R (at R + z sR + t ldr, the layout of IPMZ_STATE_RES, all
// state_len elements) <- (d r / d data) applied to tangent t of QP z; ws: the
// workspace above (may be null when no matrix block is given).  Stream-ordered
// launches, no atomics; reads the iterate and the tangents only
hipError_t qp_data_jvp(const QPBatch& qb, int ntan, const QpBlocksIn& in, double* R, int64_t ldr, int64_t sR, double* ws,
                       hipStream_t st);

}  // namespace ipmz
