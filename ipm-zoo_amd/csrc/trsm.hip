// Multi-right-hand-side solve with the LDL^T factor: every row of B (one
// right-hand side per row, stride ldb) becomes x = L^{-T} D^{-1} L^{-1} b
// (LinearSolvers.cpp:44-74 applied to each row), i.e. B <- B K^{-1}.  One
// template for the fp64 factor and for the fp32 factor of the mixed-precision
// path (mixed.hip, mixed_multi.hip).
//
// Blocked, right-looking over column panels of width w (a multiple of the
// factor's inner block nbi), everything on v_mfma_f64_16x16x4_f64 /
// v_mfma_f32_16x16x4_f32:
//
//   forward, panels ascending:
//     panel solve  Y[:, P] = B[:, P] L_PP^{-T}        (trsm_panel_kernel<.., false>)
//     update       B[:, p1:] -= Y[:, P] L[p1:, P]^T   (trsm_update_kernel<T, false>, NT)
//   B[:, j] /= D[j]                                   (trsm_scale_kernel)
//   backward, panels descending:
//     panel solve  X[:, P] = Z[:, P] L_PP^{-1}        (trsm_panel_kernel<.., true>)
//     update       B[:, :p0] -= X[:, P] L[P, :p0]     (trsm_update_kernel<T, true>, NN)
//
// The panel solve walks the panel's diagonal blocks J with the inverted
// diagonal blocks the factor left (Linv, nbi x nbi each, identity-padded):
//   forward   T = B[:, J] - sum_{K < J in P} Y[:, K] L_JK^T,  Y[:, J] = T Linv_J^T
//   backward  T = Z[:, J] - sum_{K > J in P} X[:, K] L_KJ,    X[:, J] = T Linv_J
//
// A batch of systems of one order (TrsmBatch, fp64) runs behind the same
// launches: the system is a grid dimension of every kernel, and K, D, Linv and
// B advance by per-system strides; one system is a grid of height 1 and zero
// strides.  Small systems have a whole-solve kernel besides
// (trsm_fused_kernel, ldlt_solve_fused): all N columns as ONE panel whose slab
// goes through the forward stream, the division by D and the backward stream
// without leaving LDS -- one launch per batch.
//
// Every panel-solve and update launch takes a gate (a device word, may be
// null): a non-null gate whose word is not 0 ends the kernel before any load
// (the Bunch-Kaufman solve's fallback flag, bk.hip; a batch's systems have a
// flag each, TrsmBatch::sG words apart); the LDL^T callers pass null.
//
// No kernel here waits for another workgroup: right-hand sides are
// independent, a panel-solve workgroup owns 16 of them, an update workgroup
// one output tile, and the order between launches is stream order.  No spins,
// flags, tickets or atomics -- results are deterministic.
//
// L is only read strictly below the diagonal blocks (the diagonal blocks go
// through Linv), with row-contiguous 16-byte loads staged through LDS; an L
// tile is shared by all right-hand-side rows of its workgroup.  A 16-byte
// load carries V = 2 doubles or 4 floats (Mfma<T>::V): column offsets, k
// offsets and every leading dimension are multiples of V, K and B 16-byte
// aligned and K allocated as N rows of ld elements.
//
// What the element type changes besides V:
//   * the accumulator holds rows (lane >> 4) + 4 r in fp64 and 4 (lane >> 4) + r
//     in fp32 (Mfma<T>::row);
//   * the LDS row pads are one vector.  A fragment read has lanes (c = lane &
//     15, q = lane >> 4) at c * stride + q ([n][k] stages, the slab, T) or
//     q * stride + c ([k][n] stages).  In fp32 (64 banks of 4 bytes) c * 36 mod
//     64 runs over the 16 multiples of 4 and q fills the gaps; q * 80 mod 64 =
//     16 q.  So [n][k] rows are BK + V elements (slab w + V, T nbi + V) and
//     [k][n] rows 64 + 16 in both types, all multiples of V for the 16-byte
//     stores;
//   * the fp32 factor's inner block is always 64, a compile-time constant of
//     its panel solve (PanelNbi).
#include "common.h"
#include "kernels.h"

namespace ipmz {

namespace {

constexpr int TM_NT = 256;                 // threads: 4 waves
constexpr int TM_G = 16;                   // right-hand sides per panel-solve workgroup (the MFMA M)
constexpr int TM_SB = 64;                  // columns per sub-block: 4 waves x one 16-column tile
constexpr int TM_BK = 32;                  // k-depth of one staged L tile
constexpr int TM_PADN = TM_SB + 16;        // NN stage [k][n]: row stride (k rows 32 banks apart in fp64)
constexpr int TM_STAGE = TM_BK * TM_PADN;  // elements per stage buffer
constexpr int TM_PD = 4;  // L chunks in flight (a register ring): hides the load latency of the product chain
// NT stage [n][k]: row stride (conflict-free fragment reads)
template <typename T>
constexpr int TM_PADK = TM_BK + Mfma<T>::V;
static_assert(TM_STAGE >= TM_SB * TM_PADK<float>, "stage buffer holds either form");

// The inner block as a template parameter of the panel solve: 0 = the
// run-time nbi (fp64: 64 or 128).  The fp32 factor's is the constant 64 = one
// sub-block, which folds the sub-block index away (66 VGPRs and no spills
// against 118-120 and up to 27 SGPR spills with a run-time nbi).
template <typename T>
constexpr int PanelNbi = std::is_same<T, float>::value ? TM_SB : 0;

// One 64 (n) x TM_BK (k) tile of the operator Op[k][n], global -> registers
// -> LDS.  NT: Op[k][n] = M[n * ldm + k] (rows n contiguous along k), NN:
// Op[k][n] = M[k * ldm + n] (rows k contiguous along n); n < nlim, k < kd,
// zero outside.
template <typename T, bool NN>
struct OpStage {
  typedef typename Mfma<T>::vec16_t vec_t;
  static constexpr int V = Mfma<T>::V, Q = TM_SB * TM_BK / V / TM_NT;  // vectors per thread
  vec_t r[Q];
  __device__ __forceinline__ void load(const T* __restrict__ M, int64_t ldm, int nlim, int kd, int kk) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = threadIdx.x + TM_NT * q;
      if (NN) {
        const int k = kk + ch / (TM_SB / V), n = (ch % (TM_SB / V)) * V;
        r[q] = fetch16(M + (int64_t)k * ldm + n, M, k < kd && n < nlim, nlim - n);
      } else {
        const int n = ch / (TM_BK / V), k = kk + (ch % (TM_BK / V)) * V;
        r[q] = fetch16(M + (int64_t)n * ldm + k, M, n < nlim && k < kd, kd - k);
      }
    }
  }
  __device__ __forceinline__ void store(T* Ls) const {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = threadIdx.x + TM_NT * q;
      const int off = NN ? (ch / (TM_SB / V)) * TM_PADN + (ch % (TM_SB / V)) * V
                         : (ch / (TM_BK / V)) * TM_PADK<T> + (ch % (TM_BK / V)) * V;
      *reinterpret_cast<vec_t*>(&Ls[off]) = r[q];
    }
  }
};

// dynamic LDS of the panel solve: the 16 x w slab of B, T of one diagonal
// block, two stage buffers (fp32: 57.9 KB at w = 512; fp64: up to 90 KB)
template <typename T>
inline size_t panel_lds_bytes(int w, int nbi) {
  return (size_t)(TM_G * (w + Mfma<T>::V) + TM_G * (nbi + Mfma<T>::V) + 2 * TM_STAGE) * sizeof(T);
}

// The panel solve as a stream of products acc (16 x 64) = A (16 x kd, LDS) *
// Op (kd x 64, global): per diagonal block J (size bj, 64-column sub-blocks
// u), phase 0 the columns already solved in this panel times L's block row
// (forward) / block column (backward) of J, phase 1 T times Linv_J.  Where the
// operands are depends only on (J, phase, u), never on data, so the L chunks
// of later products are loaded while earlier ones are still multiplied.
template <typename T>
struct PanelGeom {
  const T* K;
  int64_t ld;
  int N;
  const T* Linv;
  int nbi, p0, p1, SP, TP;
};
template <typename T>
struct Prod {
  const T* M;  // Op's first element
  int64_t ldm;
  int nlim, kd;   // valid columns (of 64) and depth
  int aofs, lda;  // A: offset and row stride in the slab (phase 0) or in T (phase 1)
};
template <typename T, bool BWD>
__device__ __forceinline__ Prod<T> panel_prod(const PanelGeom<T>& g, int j0, int phase, int u) {
  Prod<T> p;
  const int bj = g.N - j0 < g.nbi ? g.N - j0 : g.nbi;
  const int ko = TM_SB * u;
  if (phase == 0) {
    const int s0 = j0 + ko;
    p.nlim = g.N - s0 < TM_SB ? g.N - s0 : TM_SB;
    p.ldm = g.ld;
    p.lda = g.SP;
    if (BWD) {  // rows below the block, inside the panel
      const int je = j0 + g.nbi;
      p.M = g.K + (int64_t)je * g.ld + s0;
      p.kd = g.p1 > je ? g.p1 - je : 0;
      p.aofs = je - g.p0;
    } else {  // columns of the panel left of the block
      p.M = g.K + (int64_t)s0 * g.ld + g.p0;
      p.kd = j0 - g.p0;
      p.aofs = 0;
    }
  } else {
    const T* LinvJ = g.Linv + (int64_t)(j0 / g.nbi) * g.nbi * g.nbi;
    p.nlim = bj - ko < TM_SB ? bj - ko : TM_SB;
    p.ldm = g.nbi;
    p.lda = g.TP;
    if (BWD) {  // X[:, n] = sum_{k >= n} T[:, k] Linv[k][n]
      p.M = LinvJ + (int64_t)ko * g.nbi + ko;
      p.kd = bj - ko;
      p.aofs = ko;
    } else {  // Y[:, n] = sum_{k <= n} T[:, k] Linv[n][k]
      p.M = LinvJ + (int64_t)ko * g.nbi;
      p.kd = ko + TM_SB < bj ? ko + TM_SB : bj;
      p.aofs = 0;
    }
  }
  return p;
}
// position in the stream: chunk t of product (j0, phase, u)
template <typename T>
struct Cursor {
  int j0, phase, u, t, nch;
  bool valid;
  Prod<T> p;
};
// NBI: the panel kernel's; a constant inner block is one sub-block, and u stays 0
template <typename T, int NBI, bool BWD>
__device__ __forceinline__ void cursor_next(const PanelGeom<T>& g, Cursor<T>& c) {
  if (++c.t < c.nch) return;
  c.t = 0;
  for (;;) {
    const int bj = g.N - c.j0 < g.nbi ? g.N - c.j0 : g.nbi;
    if (NBI == TM_SB || ++c.u >= (bj + TM_SB - 1) / TM_SB) {
      c.u = 0;
      if (++c.phase > 1) {
        c.phase = 0;
        c.j0 += BWD ? -g.nbi : g.nbi;
        if (BWD ? c.j0 < g.p0 : c.j0 >= g.p1) {
          c.valid = false;
          return;
        }
      }
    }
    c.p = panel_prod<T, BWD>(g, c.j0, c.phase, c.u);
    c.nch = (c.p.kd + TM_BK - 1) / TM_BK;
    if (c.nch > 0) return;  // (only the first block's phase 0 is empty, and the stream starts after it)
  }
}

// The 16 x w slab of B[r0 .. r0 + 16, p0 .. p0 + w) <-> LDS (row stride SP);
// rows >= nrhs and columns >= p1 are zero in LDS and never stored.
template <typename T>
__device__ __forceinline__ void slab_load(const T* B, int64_t ldb, int nrhs, int r0, int p0, int p1, int w, T* slab,
                                          int SP) {
  typedef typename Mfma<T>::vec16_t vec_t;
  constexpr int V = Mfma<T>::V;
  const int vw = w / V;
  for (int idx = threadIdx.x; idx < TM_G * vw; idx += TM_NT) {
    const int r = idx / vw, c = (idx % vw) * V;
    const bool rok = r0 + r < nrhs;
    const vec_t v = fetch16(B + (int64_t)(r0 + r) * ldb + p0 + c, B + (int64_t)r0 * ldb + p0, rok && p0 + c < p1,
                            p1 - p0 - c);
    *reinterpret_cast<vec_t*>(&slab[r * SP + c]) = v;
  }
}
template <typename T>
__device__ __forceinline__ void slab_store(T* B, int64_t ldb, int nrhs, int r0, int p0, int p1, int w, const T* slab,
                                           int SP) {
  typedef typename Mfma<T>::vec16_t vec_t;
  constexpr int V = Mfma<T>::V;
  const int vw = w / V;
  for (int idx = threadIdx.x; idx < TM_G * vw; idx += TM_NT) {
    const int r = idx / vw, c = (idx % vw) * V;
    if (r0 + r >= nrhs || p0 + c >= p1) continue;
    T* dst = B + (int64_t)(r0 + r) * ldb + p0 + c;
    const T* src = &slab[r * SP + c];
    if (p0 + c + V - 1 < p1) *reinterpret_cast<vec_t*>(dst) = *reinterpret_cast<const vec_t*>(src);
    else
      for (int e = 0; p0 + c + e < p1; ++e) dst[e] = src[e];
  }
}

// One sweep of the stream over the panel g, on a slab that stays in LDS: both
// sweeps of trsm_fused_kernel.  It is trsm_panel_kernel's stream, statement by
// statement, as a device function; that kernel keeps its own inline copy,
// because built from this function its instantiations take 3-4 more VGPRs and
// drop one wave of occupancy each (fp64 118 / 120 -> 122 / 123 with 8 AGPRs,
// occupancy 4 -> 3; fp32 66 / 67 -> 70 / 69, 7 -> 6; DESIGN.md "Batched
// multi-right-hand-side solve").  A change to one belongs in the other.  One
// barrier per chunk: chunk c is written to LDS buffer c & 1, the barrier
// passed, the ring slot refilled with chunk c + TM_PD, chunk c multiplied; a
// product's result is written (T, or the slab) right after its last chunk, one
// barrier before anything reads it.  fill(): whatever has to reach the slab
// before the first product (the load of B; nothing when the slab already holds
// the sweep's input), issued behind the ring's first loads; a barrier follows
// it, and one ends the sweep.  NBI: the inner block as a constant, or 0 for
// g.nbi.
template <typename T, int NBI, bool BWD, typename Fill>
__device__ __forceinline__ void panel_stream(const PanelGeom<T>& g, T* slab, T* Ts, T* Ls, Fill&& fill) {
  typedef typename Mfma<T>::acc_t acc_t;
  constexpr int PADK = TM_PADK<T>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nbi = g.nbi, p0 = g.p0, p1 = g.p1, SP = g.SP, TP = g.TP;

  // the stream starts at phase 1 of the first block (its phase 0 is empty: T = B[:, J])
  const int jfirst = BWD ? p0 + ((p1 - p0 - 1) / nbi) * nbi : p0;
  Cursor<T> cc;
  cc.j0 = jfirst;
  cc.phase = 1;
  cc.u = 0;
  cc.t = 0;
  cc.valid = true;
  cc.p = panel_prod<T, BWD>(g, jfirst, 1, 0);
  cc.nch = (cc.p.kd + TM_BK - 1) / TM_BK;
  Cursor<T> lc = cc;
  OpStage<T, BWD> ring[TM_PD];
  // (past the end of the stream the ring still loads -- all lanes masked, the
  // product's first element -- and never branches around a load: only then
  // does the compiler keep the later slots in flight behind counted waits)
#pragma unroll
  for (int d = 0; d < TM_PD; ++d) {
    ring[d].load(lc.p.M, lc.p.ldm, lc.valid ? lc.p.nlim : 0, lc.p.kd, lc.t * TM_BK);
    if (lc.valid) cursor_next<T, NBI, BWD>(g, lc);
  }

  fill();
  __syncthreads();
  for (int idx = tid; idx < TM_G * TP; idx += TM_NT) {
    const int r = idx / TP, c = idx % TP;
    Ts[idx] = c < nbi ? slab[r * SP + (jfirst - p0) + c] : T(0);
  }

  const int col = 16 * wave + (lane & 15);  // this lane's column inside a sub-block
  const int frag = BWD ? (lane >> 4) * TM_PADN + col : col * PADK + (lane >> 4);
  acc_t acc = {T(0), T(0), T(0), T(0)};
  int buf = 0;
  for (;;) {
#pragma unroll
    for (int d = 0; d < TM_PD; ++d) {
      if (!cc.valid) goto done;
      T* bs = Ls + buf * TM_STAGE;
      ring[d].store(bs);
      __syncthreads();
      ring[d].load(lc.p.M, lc.p.ldm, lc.valid ? lc.p.nlim : 0, lc.p.kd, lc.t * TM_BK);
      if (lc.valid) cursor_next<T, NBI, BWD>(g, lc);
      const T* As = (cc.phase == 0 ? slab : Ts) + cc.p.aofs + (lane & 15) * cc.p.lda + (lane >> 4) + cc.t * TM_BK;
#pragma unroll
      for (int s = 0; s < TM_BK / 4; ++s)
        acc = Mfma<T>::mma(As[4 * s], bs[frag + (BWD ? 4 * s * TM_PADN : 4 * s)], acc);
      if (cc.t == cc.nch - 1) {
        const int so = cc.j0 - p0 + TM_SB * cc.u + col;  // slab column
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = Mfma<T>::row(lane, r);
          if (cc.phase == 0) Ts[row * TP + TM_SB * cc.u + col] = slab[row * SP + so] - acc[r];
          else slab[row * SP + so] = acc[r];
        }
        acc = (acc_t){T(0), T(0), T(0), T(0)};
      }
      cursor_next<T, NBI, BWD>(g, cc);
      buf ^= 1;
    }
  }
done:
  __syncthreads();
}

// Panel solve of columns [p0, min(p0 + w, N)) for right-hand sides
// [16 * blockIdx.x, +16): the slab lives in LDS from the first load to the
// last store.  One barrier per chunk: chunk c is written to LDS buffer c & 1,
// the barrier passed, the ring slot refilled with chunk c + TM_PD, chunk c
// multiplied; a product's result is written (T, or the slab) right after its
// last chunk, one barrier before anything reads it.  NBI: the inner block as a
// constant, or 0 for nbi_rt.
template <typename T, int NBI, bool BWD>
__global__ __launch_bounds__(TM_NT) void trsm_panel_kernel(const T* __restrict__ K, int64_t ld, int N,
                                                           const T* __restrict__ Linv, int nbi_rt, T* B, int64_t ldb,
                                                           int nrhs, int p0, int w, const unsigned* gate, int64_t sK,
                                                           int64_t sL, int64_t sB, int64_t sG) {
  if (gate && gate[blockIdx.y * sG] != 0u) return;
  K += blockIdx.y * sK;
  Linv += blockIdx.y * sL;
  B += blockIdx.y * sB;
  typedef typename Mfma<T>::vec16_t vec_t;
  typedef typename Mfma<T>::acc_t acc_t;
  constexpr int V = Mfma<T>::V, PADK = TM_PADK<T>;
  static_assert(NBI == 0 || NBI == TM_SB, "a constant inner block is one sub-block");
  extern __shared__ __attribute__((aligned(16))) unsigned char trsm_sm[];
  const int nbi = NBI ? NBI : nbi_rt;
  const int SP = w + V, TP = nbi + V;
  T* slab = reinterpret_cast<T*>(trsm_sm);  // [16][SP]: B[:, P], overwritten block by block with the solution
  T* Ts = slab + TM_G * SP;                 // [16][TP]: T of the current diagonal block
  T* Ls = Ts + TM_G * TP;                   // [2][TM_STAGE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * TM_G;
  const int p1 = p0 + w < N ? p0 + w : N;
  const int vw = w / V;
  const PanelGeom<T> g = {K, ld, N, Linv, nbi, p0, p1, SP, TP};

  // the stream starts at phase 1 of the first block (its phase 0 is empty: T = B[:, J])
  const int jfirst = BWD ? p0 + ((p1 - p0 - 1) / nbi) * nbi : p0;
  Cursor<T> cc;
  cc.j0 = jfirst;
  cc.phase = 1;
  cc.u = 0;
  cc.t = 0;
  cc.valid = true;
  cc.p = panel_prod<T, BWD>(g, jfirst, 1, 0);
  cc.nch = (cc.p.kd + TM_BK - 1) / TM_BK;
  Cursor<T> lc = cc;
  OpStage<T, BWD> ring[TM_PD];
  // (past the end of the stream the ring still loads -- all lanes masked, the
  // product's first element -- and never branches around a load: only then
  // does the compiler keep the later slots in flight behind counted waits)
#pragma unroll
  for (int d = 0; d < TM_PD; ++d) {
    ring[d].load(lc.p.M, lc.p.ldm, lc.valid ? lc.p.nlim : 0, lc.p.kd, lc.t * TM_BK);
    if (lc.valid) cursor_next<T, NBI, BWD>(g, lc);
  }

  for (int idx = tid; idx < TM_G * vw; idx += TM_NT) {
    const int r = idx / vw, c = (idx % vw) * V;
    const bool rok = r0 + r < nrhs;
    const vec_t v = fetch16(B + (int64_t)(r0 + r) * ldb + p0 + c, B + (int64_t)r0 * ldb + p0, rok && p0 + c < p1,
                            p1 - p0 - c);
    *reinterpret_cast<vec_t*>(&slab[r * SP + c]) = v;
  }
  __syncthreads();
  for (int idx = tid; idx < TM_G * TP; idx += TM_NT) {
    const int r = idx / TP, c = idx % TP;
    Ts[idx] = c < nbi ? slab[r * SP + (jfirst - p0) + c] : T(0);
  }

  const int col = 16 * wave + (lane & 15);  // this lane's column inside a sub-block
  const int frag = BWD ? (lane >> 4) * TM_PADN + col : col * PADK + (lane >> 4);
  acc_t acc = {T(0), T(0), T(0), T(0)};
  int buf = 0;
  for (;;) {
#pragma unroll
    for (int d = 0; d < TM_PD; ++d) {
      if (!cc.valid) goto done;
      T* bs = Ls + buf * TM_STAGE;
      ring[d].store(bs);
      __syncthreads();
      ring[d].load(lc.p.M, lc.p.ldm, lc.valid ? lc.p.nlim : 0, lc.p.kd, lc.t * TM_BK);
      if (lc.valid) cursor_next<T, NBI, BWD>(g, lc);
      const T* As = (cc.phase == 0 ? slab : Ts) + cc.p.aofs + (lane & 15) * cc.p.lda + (lane >> 4) + cc.t * TM_BK;
#pragma unroll
      for (int s = 0; s < TM_BK / 4; ++s)
        acc = Mfma<T>::mma(As[4 * s], bs[frag + (BWD ? 4 * s * TM_PADN : 4 * s)], acc);
      if (cc.t == cc.nch - 1) {
        const int so = cc.j0 - p0 + TM_SB * cc.u + col;  // slab column
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = Mfma<T>::row(lane, r);
          if (cc.phase == 0) Ts[row * TP + TM_SB * cc.u + col] = slab[row * SP + so] - acc[r];
          else slab[row * SP + so] = acc[r];
        }
        acc = (acc_t){T(0), T(0), T(0), T(0)};
      }
      cursor_next<T, NBI, BWD>(g, cc);
      buf ^= 1;
    }
  }
done:
  __syncthreads();

  for (int idx = tid; idx < TM_G * vw; idx += TM_NT) {
    const int r = idx / vw, c = (idx % vw) * V;
    if (r0 + r >= nrhs || p0 + c >= p1) continue;
    T* dst = B + (int64_t)(r0 + r) * ldb + p0 + c;
    const T* src = &slab[r * SP + c];
    if (p0 + c + V - 1 < p1) *reinterpret_cast<vec_t*>(dst) = *reinterpret_cast<const vec_t*>(src);
    else
      for (int e = 0; p0 + c + e < p1; ++e) dst[e] = src[e];
  }
}

// The whole solve of one small system in one workgroup (fp64): right-hand
// sides [16 * blockIdx.x, +16) of system blockIdx.y, all N columns as one
// "panel" of width round_up(N, nbi).  The slab is loaded once, passes through
// the forward sweep, the division by D and the backward sweep in LDS, and is
// stored once; L is read once per sweep.  No other workgroup is waited for.
// NBI: 64 = the inner block as a constant (one sub-block, as the fp32 panel
// solve's), 0 = nbi_rt (128).
template <int NBI>
__global__ __launch_bounds__(TM_NT) void trsm_fused_kernel(const double* __restrict__ K, int64_t ld, int N,
                                                           const double* __restrict__ D,
                                                           const double* __restrict__ Linv, int nbi_rt, double* B,
                                                           int64_t ldb, int nrhs, int64_t sK, int64_t sD, int64_t sL,
                                                           int64_t sB) {
  constexpr int V = Mfma<double>::V;
  static_assert(NBI == 0 || NBI == TM_SB, "a constant inner block is one sub-block");
  const int nbi = NBI ? NBI : nbi_rt;
  extern __shared__ __attribute__((aligned(16))) unsigned char trsm_sm[];
  K += blockIdx.y * sK;
  D += blockIdx.y * sD;
  Linv += blockIdx.y * sL;
  B += blockIdx.y * sB;
  const int w = (N + nbi - 1) / nbi * nbi;
  const int SP = w + V, TP = nbi + V;
  double* slab = reinterpret_cast<double*>(trsm_sm);
  double* Ts = slab + TM_G * SP;
  double* Ls = Ts + TM_G * TP;
  const int r0 = blockIdx.x * TM_G;
  const PanelGeom<double> g = {K, ld, N, Linv, nbi, 0, N, SP, TP};
  panel_stream<double, NBI, false>(g, slab, Ts, Ls, [&] { slab_load<double>(B, ldb, nrhs, r0, 0, N, w, slab, SP); });
  // Z = Y / D (a division, as trsm_scale_kernel; rows past nrhs are zero and never stored)
  for (int j = threadIdx.x; j < N; j += TM_NT) {
    const double d = D[j];
#pragma unroll 4
    for (int r = 0; r < TM_G; ++r) slab[r * SP + j] = slab[r * SP + j] / d;
  }
  panel_stream<double, NBI, true>(g, slab, Ts, Ls, [] {});  // (its first barrier orders the division before T)
  slab_store<double>(B, ldb, nrhs, r0, 0, N, w, slab, SP);
}

// The whole prepared Bunch-Kaufman solve of one small system in one workgroup
// (bk.hip "Device-wide solve": A^{-1} = P^T L'^{-T} D^{-1} L'^{-1} P): right-hand
// sides [16 * blockIdx.x, +16) of system blockIdx.y.  trsm_fused_kernel's
// design on L' (K = L', unit lower, inner block 64): the slab is loaded
// through perm (the row permutation fused into the load, 8-byte loads), goes
// through the forward stream, the D solve in the reference's arithmetic
// (bkf::k_dsolve_rows' expressions; a 2x2 pivot's two entries are both in the
// slab, wherever the pair lies against the 64-column blocks), the backward
// stream, and is stored through perm.  It shares panel_stream with
// trsm_fused_kernel -- the panel kernels keep their inline copy, so their
// registers do not change.  A system whose fallback flag is set is left to
// the fallback launch: its workgroups exit before any load.
__global__ __launch_bounds__(TM_NT) void trsm_bk_fused_kernel(const double* __restrict__ K, int64_t ld, int N,
                                                              const double* __restrict__ Linv, double* B, int64_t ldb,
                                                              int nrhs, BkFusedMeta m, int64_t sK, int64_t sL,
                                                              int64_t sB) {
  constexpr int V = Mfma<double>::V;
  m = m.of(blockIdx.y);
  if (m.flag[0] != 0u) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char trsm_sm[];
  K += blockIdx.y * sK;
  Linv += blockIdx.y * sL;
  B += blockIdx.y * sB;
  const int w = (N + TM_SB - 1) / TM_SB * TM_SB;
  const int SP = w + V, TP = TM_SB + V;
  double* slab = reinterpret_cast<double*>(trsm_sm);
  double* Ts = slab + TM_G * SP;
  double* Ls = Ts + TM_G * TP;
  const int r0 = blockIdx.x * TM_G;
  const PanelGeom<double> g = {K, ld, N, Linv, TM_SB, 0, N, SP, TP};
  // slab[r][p] = b_r[perm[p]]; rows >= nrhs and columns >= N are zero and never stored
  panel_stream<double, TM_SB, false>(g, slab, Ts, Ls, [&] {
    for (int idx = threadIdx.x; idx < TM_G * w; idx += TM_NT) {
      const int r = idx / w, c = idx % w;
      slab[r * SP + c] = (r0 + r < nrhs && c < N) ? B[(int64_t)(r0 + r) * ldb + m.perm[c]] : 0.0;
    }
  });
  // Z = D^{-1} Y: the thread on the first row of a 2x2 pivot writes both entries of its pair
  for (int k = threadIdx.x; k < N; k += TM_NT) {
    const int kd = m.kind[k];
    if (kd == 0) {
      const double d = m.d11[k];
#pragma unroll 4
      for (int r = 0; r < TM_G; ++r) slab[r * SP + k] = slab[r * SP + k] / d;
    } else if (kd == 1 && k + 1 < N) {
      const double akm1k = m.d21[k];
      const double akm1 = m.d11[k] / akm1k;
      const double ak = m.d22[k] / akm1k;
      const double denom = akm1 * ak - 1.0;
#pragma unroll 2
      for (int r = 0; r < TM_G; ++r) {
        const double bkm1 = slab[r * SP + k] / akm1k;
        const double bk = slab[r * SP + k + 1] / akm1k;
        slab[r * SP + k] = (ak * bkm1 - bk) / denom;
        slab[r * SP + k + 1] = (akm1 * bk - bkm1) / denom;
      }
    }
  }
  panel_stream<double, TM_SB, true>(g, slab, Ts, Ls, [] {});  // (its first barrier orders the D solve before T)
  for (int idx = threadIdx.x; idx < TM_G * w; idx += TM_NT) {
    const int r = idx / w, c = idx % w;
    if (r0 + r < nrhs && c < N) B[(int64_t)(r0 + r) * ldb + m.perm[c]] = slab[r * SP + c];
  }
}

// between the sweeps: B[r][j] /= D[j] (a division, LinearSolvers.cpp:62-64);
// system blockIdx.z (strides sB, sD)
template <typename T>
__global__ __launch_bounds__(TM_NT) void trsm_scale_kernel(T* B, int64_t ldb, int nrhs, int N,
                                                           const T* __restrict__ D, int64_t sB, int64_t sD) {
  const int j = blockIdx.x * TM_NT + threadIdx.x;
  if (j >= N) return;
  B += blockIdx.z * sB;
  D += blockIdx.z * sD;
  const T d = D[j];
  for (int r = blockIdx.y; r < nrhs; r += gridDim.y) {
    T* p = B + (int64_t)r * ldb + j;
    *p = *p / d;
  }
}

// The updates between panel solves, C[i][j] -= sum_k X[i][k] Op[k][j] for
// i < M (right-hand sides), j < Nc, k < Kd:
//   forward  (NT)  Op[k][j] = L[j * ldl + k]: B[:, p1:] -= Y[:, P] L[p1:, P]^T
//   backward (NN)  Op[k][j] = L[k * ldl + j]: B[:, :p0] -= X[:, P] L[P, :p0]
// 64 x 64 tile, 8 waves in 2 x 4 (32 x 16 each: two waves per SIMD, so one
// wave's LDS reads and barrier wait run under the other's MFMAs), k-chunks of
// one vector of X and one of L per thread (8 V: 16 deep in fp64, 32 in fp32)
// through two LDS buffers with one barrier per chunk as gemm.h's NT engine
// does, but UN_PD chunks in flight in a register ring: Kd is only one panel
// deep, so a tile is a short serial chain and nothing else hides its
// latencies.  The L tile is staged [j][k] (NT) or [k][j] (NN).  Workgroups
// that share an L tile (the right-hand-side groups of one column tile) have
// consecutive ids.  System blockIdx.y: X and C advance by sX, L by sL.
constexpr int UN_NT = 512, UN_BM = 64, UN_BN = 64, UN_PADB = UN_BN + 16, UN_PD = 3;
template <typename T>
struct UpdStage {
  typename Mfma<T>::vec16_t ra, rb;
};
template <typename T, bool NN>
__global__ __launch_bounds__(UN_NT) void trsm_update_kernel(const T* X, int64_t ldx, const T* __restrict__ L,
                                                            int64_t ldl, T* C, int64_t ldc, int M, int Nc, int Kd,
                                                            int ntm, const unsigned* gate, int64_t sX, int64_t sL,
                                                            int64_t sG) {
  if (gate && gate[blockIdx.y * sG] != 0u) return;
  typedef typename Mfma<T>::vec16_t vec_t;
  typedef typename Mfma<T>::acc_t acc_t;
  constexpr int V = Mfma<T>::V, BK = 8 * V, PADA = BK + V, BSTAGE = BK * UN_PADB;
  X += blockIdx.y * sX;
  C += blockIdx.y * sX;
  L += blockIdx.y * sL;
  static_assert(BSTAGE >= UN_BN * PADA, "B stage buffer holds either form");
  static_assert(UN_BM * BK / V == UN_NT && BK * UN_BN / V == UN_NT, "one vector of each operand per thread");
  __shared__ __attribute__((aligned(16))) T As[2][UN_BM * PADA];
  __shared__ __attribute__((aligned(16))) T Bs[2][BSTAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int i0 = (blockIdx.x % ntm) * UN_BM, j0 = (blockIdx.x / ntm) * UN_BN;
  auto load = [&](UpdStage<T>& st, int kk) {
    {
      const int i = i0 + tid / (BK / V), k = kk + (tid % (BK / V)) * V;
      st.ra = fetch16(X + (int64_t)i * ldx + k, X, i < M && k < Kd, Kd - k);
    }
    if (NN) {
      const int k = kk + tid / (UN_BN / V), j = j0 + (tid % (UN_BN / V)) * V;
      st.rb = fetch16(L + (int64_t)k * ldl + j, L, k < Kd && j < Nc, Nc - j);
    } else {
      const int j = j0 + tid / (BK / V), k = kk + (tid % (BK / V)) * V;
      st.rb = fetch16(L + (int64_t)j * ldl + k, L, j < Nc && k < Kd, Kd - k);
    }
  };
  auto store = [&](const UpdStage<T>& st, T* as, T* bs) {
    *reinterpret_cast<vec_t*>(&as[(tid / (BK / V)) * PADA + (tid % (BK / V)) * V]) = st.ra;
    const int off = NN ? (tid / (UN_BN / V)) * UN_PADB + (tid % (UN_BN / V)) * V
                       : (tid / (BK / V)) * PADA + (tid % (BK / V)) * V;
    *reinterpret_cast<vec_t*>(&bs[off]) = st.rb;
  };
  acc_t acc[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) acc[a] = (acc_t){T(0), T(0), T(0), T(0)};
  const int nch = (Kd + BK - 1) / BK;
  UpdStage<T> ring[UN_PD];
  // (loads past Kd are fully masked, never branched around: see trsm_panel_kernel)
#pragma unroll
  for (int d = 0; d < UN_PD; ++d) load(ring[d], d * BK);
  const int aoff = (wr * 32 + (lane & 15)) * PADA + (lane >> 4);
  const int boff = NN ? (lane >> 4) * UN_PADB + wc * 16 + (lane & 15) : (wc * 16 + (lane & 15)) * PADA + (lane >> 4);
  for (int t0 = 0;; t0 += UN_PD) {
#pragma unroll
    for (int d = 0; d < UN_PD; ++d) {
      const int t = t0 + d;
      if (t >= nch) goto done;
      const int cur = t & 1;
      store(ring[d], As[cur], Bs[cur]);
      __syncthreads();
      load(ring[d], (t + UN_PD) * BK);
      const T* as = As[cur];
      const T* bs = Bs[cur];
#pragma unroll
      for (int s = 0; s < BK / 4; ++s) {
        const T bf = bs[boff + (NN ? 4 * s * UN_PADB : 4 * s)];
#pragma unroll
        for (int a = 0; a < 2; ++a) acc[a] = Mfma<T>::mma(as[aoff + a * 16 * PADA + 4 * s], bf, acc[a]);
      }
    }
  }
done:
  const int j = j0 + wc * 16 + (lane & 15);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wr * 32 + a * 16 + Mfma<T>::row(lane, r);
      if (i < M && j < Nc) {
        T* cp = C + (int64_t)i * ldc + j;
        *cp = *cp - acc[a][r];
      }
    }
}

template <typename T, bool NN>
hipError_t launch_update(const T* X, int64_t ldx, const T* L, int64_t ldl, T* C, int64_t ldc, int M, int Nc, int Kd,
                         hipStream_t st, const unsigned* gate, const TrsmBatch& tb) {
  const int ntm = (M + UN_BM - 1) / UN_BM, ntn = (Nc + UN_BN - 1) / UN_BN;
  hipLaunchKernelGGL((trsm_update_kernel<T, NN>), dim3((unsigned)(ntm * ntn), (unsigned)tb.B), dim3(UN_NT), 0, st, X,
                     ldx, L, ldl, C, ldc, M, Nc, Kd, ntm, gate, tb.sB, tb.sK, tb.sG);
  return hipGetLastError();
}

template <typename T, bool BWD>
hipError_t launch_panel(const T* K, int64_t ld, int N, const T* Linv, int nbi, T* B, int64_t ldb, int nrhs, int p0,
                        int w, hipStream_t st, const unsigned* gate, const TrsmBatch& tb) {
  constexpr int NBI = PanelNbi<T>;
  // fp64: more than the 64 KB a kernel gets by default; raised once per process
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&trsm_panel_kernel<T, NBI, BWD>), hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)panel_lds_bytes<T>(IPMZ_TRSM_PANEL_MAX, NBI ? NBI : 128));
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL((trsm_panel_kernel<T, NBI, BWD>), dim3((nrhs + TM_G - 1) / TM_G, (unsigned)tb.B), dim3(TM_NT),
                     panel_lds_bytes<T>(w, nbi), st, K, ld, N, Linv, nbi, B, ldb, nrhs, p0, w, gate, tb.sK, tb.sL,
                     tb.sB, tb.sG);
  return hipGetLastError();
}

// LDS one workgroup may use on the current device (cached per process; one device type)
size_t device_lds_per_workgroup() {
  static size_t lds = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || n <= 0)
      n = 64 * 1024;
    return (size_t)n;
  }();
  return lds;
}

// more systems than a grid dimension holds, or strides that break the 16-byte loads
bool batch_ok(const TrsmBatch& tb) {
  return tb.B >= 1 && tb.B <= 65535 && (tb.B == 1 || !((tb.sK | tb.sL | tb.sB) & 1));
}

}  // namespace

template <typename T>
hipError_t trsm_sweep(const T* K, int64_t ld, int N, const T* Linv, int nbi, T* B, int64_t ldb, int nrhs, int w,
                      bool backward, hipStream_t st, const unsigned* gate, const TrsmBatch& tb) {
  if (N <= 0 || nrhs <= 0) return hipSuccess;
  // fp32: the mixed factor (nbi = 64, rows of whole 64-column blocks); leading dimensions in whole vectors
  const bool ok = std::is_same<T, float>::value
                      ? nbi == 64 && !(ld & 63) && !(ldb & 3) && !((uintptr_t)Linv & 15)
                      : (nbi == 64 || nbi == 128) && !(ld & 1) && !(ldb & 1);
  if (!ok || w < nbi || w % 128 != 0 || w > IPMZ_TRSM_PANEL_MAX || ld < N || ldb < N || ((uintptr_t)K & 15) ||
      ((uintptr_t)B & 15) || !batch_ok(tb) || (tb.B > 1 && std::is_same<T, float>::value))
    return hipErrorInvalidValue;
  hipError_t e;
  if (!backward) {
    for (int p0 = 0; p0 < N; p0 += w) {
      const int p1 = p0 + w < N ? p0 + w : N;
      if ((e = launch_panel<T, false>(K, ld, N, Linv, nbi, B, ldb, nrhs, p0, w, st, gate, tb)) != hipSuccess) return e;
      if (p1 < N &&  // B[:, p1:] -= Y[:, P] L[p1:, P]^T
          (e = launch_update<T, false>(B + p0, ldb, K + (int64_t)p1 * ld + p0, ld, B + p1, ldb, nrhs, N - p1, p1 - p0,
                                       st, gate, tb)) != hipSuccess)
        return e;
    }
    return hipSuccess;
  }
  for (int p0 = ((N - 1) / w) * w; p0 >= 0; p0 -= w) {
    const int p1 = p0 + w < N ? p0 + w : N;
    if ((e = launch_panel<T, true>(K, ld, N, Linv, nbi, B, ldb, nrhs, p0, w, st, gate, tb)) != hipSuccess) return e;
    if (p0 > 0 &&  // B[:, :p0] -= X[:, P] L[P, :p0]
        (e = launch_update<T, true>(B + p0, ldb, K + (int64_t)p0 * ld, ld, B, ldb, nrhs, p0, p1 - p0, st, gate, tb)) !=
            hipSuccess)
      return e;
  }
  return hipSuccess;
}
template hipError_t trsm_sweep<double>(const double*, int64_t, int, const double*, int, double*, int64_t, int, int,
                                       bool, hipStream_t, const unsigned*, const TrsmBatch&);
template hipError_t trsm_sweep<float>(const float*, int64_t, int, const float*, int, float*, int64_t, int, int, bool,
                                      hipStream_t, const unsigned*, const TrsmBatch&);

template <typename T>
hipError_t ldlt_solve_multi(const T* K, int64_t ld, int N, const T* D, const T* Linv, int nbi, T* B, int64_t ldb,
                            int nrhs, int w, hipStream_t st, const TrsmBatch& tb) {
  if (N <= 0 || nrhs <= 0) return hipSuccess;
  hipError_t e = trsm_sweep<T>(K, ld, N, Linv, nbi, B, ldb, nrhs, w, false, st, nullptr, tb);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(trsm_scale_kernel<T>, dim3((N + TM_NT - 1) / TM_NT, nrhs < 64 ? nrhs : 64, (unsigned)tb.B),
                     dim3(TM_NT), 0, st, B, ldb, nrhs, N, D, tb.sB, tb.sD);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return trsm_sweep<T>(K, ld, N, Linv, nbi, B, ldb, nrhs, w, true, st, nullptr, tb);
}
template hipError_t ldlt_solve_multi<double>(const double*, int64_t, int, const double*, const double*, int, double*,
                                             int64_t, int, int, hipStream_t, const TrsmBatch&);
template hipError_t ldlt_solve_multi<float>(const float*, int64_t, int, const float*, const float*, int, float*,
                                            int64_t, int, int, hipStream_t, const TrsmBatch&);

bool ldlt_solve_fused_eligible(int N, int nbi) {
  if (N <= 0 || (nbi != 64 && nbi != 128)) return false;
  return panel_lds_bytes<double>((N + nbi - 1) / nbi * nbi, nbi) <= device_lds_per_workgroup();
}

hipError_t ldlt_solve_fused(const double* K, int64_t ld, int N, const double* D, const double* Linv, int nbi,
                            double* B, int64_t ldb, int nrhs, hipStream_t st, const TrsmBatch& tb) {
  if (N <= 0 || nrhs <= 0) return hipSuccess;
  if (!ldlt_solve_fused_eligible(N, nbi) || (ld & 1) || (ldb & 1) || ld < N || ldb < N || ((uintptr_t)K & 15) ||
      ((uintptr_t)B & 15) || !batch_ok(tb))
    return hipErrorInvalidValue;
  // all the LDS a workgroup may have; raised once per process
  static const hipError_t attr = [] {
    const int lds = (int)device_lds_per_workgroup();
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&trsm_fused_kernel<TM_SB>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&trsm_fused_kernel<0>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e;
  }();
  if (attr != hipSuccess) return attr;
  const dim3 grid((nrhs + TM_G - 1) / TM_G, (unsigned)tb.B);
  const size_t lds = panel_lds_bytes<double>((N + nbi - 1) / nbi * nbi, nbi);
  if (nbi == TM_SB)
    hipLaunchKernelGGL(trsm_fused_kernel<TM_SB>, grid, dim3(TM_NT), lds, st, K, ld, N, D, Linv, nbi, B, ldb, nrhs, tb.sK,
                       tb.sD, tb.sL, tb.sB);
  else
    hipLaunchKernelGGL(trsm_fused_kernel<0>, grid, dim3(TM_NT), lds, st, K, ld, N, D, Linv, nbi, B, ldb, nrhs, tb.sK,
                       tb.sD, tb.sL, tb.sB);
  return hipGetLastError();
}

bool bk_solve_fused_eligible(int N) { return ldlt_solve_fused_eligible(N, TM_SB); }

hipError_t bk_solve_fused(const double* Lp, int64_t ldp, int N, const double* Linv, double* B, int64_t ldb, int nrhs,
                          const BkFusedMeta& m, hipStream_t st, const TrsmBatch& tb) {
  if (N <= 0 || nrhs <= 0) return hipSuccess;
  if (!bk_solve_fused_eligible(N) || (ldp & 1) || ldp < N || ldb < N || ((uintptr_t)Lp & 15) ||
      ((uintptr_t)Linv & 15) || !batch_ok(tb))
    return hipErrorInvalidValue;
  // all the LDS a workgroup may have; raised once per process
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&trsm_bk_fused_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)device_lds_per_workgroup());
  if (attr != hipSuccess) return attr;
  const int w = (N + TM_SB - 1) / TM_SB * TM_SB;
  hipLaunchKernelGGL(trsm_bk_fused_kernel, dim3((nrhs + TM_G - 1) / TM_G, (unsigned)tb.B), dim3(TM_NT),
                     panel_lds_bytes<double>(w, TM_SB), st, Lp, ldp, N, Linv, B, ldb, nrhs, m, tb.sK, tb.sL, tb.sB);
  return hipGetLastError();
}

}  // namespace ipmz
