// Multi-right-hand-side solve with the LDL^T factor: every row of B (one
// right-hand side per row, stride ldb) becomes x = L^{-T} D^{-1} L^{-1} b
// (LinearSolvers.cpp:44-74 applied to each row), i.e. B <- B K^{-1}.
//
// Blocked, right-looking over column panels of width w (a multiple of the
// factor's inner block nbi), everything on v_mfma_f64_16x16x4_f64:
//
//   forward, panels ascending:
//     panel solve  Y[:, P] = B[:, P] L_PP^{-T}        (trsm_panel_kernel<false>)
//     update       B[:, p1:] -= Y[:, P] L[p1:, P]^T   (trsm_update_kernel<false>, NT)
//   B[:, j] /= D[j]                                   (trsm_scale_kernel)
//   backward, panels descending:
//     panel solve  X[:, P] = Z[:, P] L_PP^{-1}        (trsm_panel_kernel<true>)
//     update       B[:, :p0] -= X[:, P] L[P, :p0]     (trsm_update_kernel<true>, NN)
//
// The panel solve walks the panel's diagonal blocks J with the inverted
// diagonal blocks the factor left (Linv, nbi x nbi each, identity-padded):
//   forward   T = B[:, J] - sum_{K < J in P} Y[:, K] L_JK^T,  Y[:, J] = T Linv_J^T
//   backward  T = Z[:, J] - sum_{K > J in P} X[:, K] L_KJ,    X[:, J] = T Linv_J
//
// No kernel here waits for another workgroup: right-hand sides are
// independent, a panel-solve workgroup owns 16 of them, an update workgroup
// one output tile, and the order between launches is stream order.  No spins,
// flags, tickets or atomics -- results are deterministic.
//
// L is only read strictly below the diagonal blocks (the diagonal blocks go
// through Linv), with row-contiguous 16-byte loads staged through LDS; an L
// tile is shared by all right-hand-side rows of its workgroup.  Needs even
// ld / ldb, 16-byte aligned K / B and K allocated as N rows of ld elements.
#include "common.h"
#include "kernels.h"

namespace ipmz {

namespace {

constexpr int TM_NT = 256;                 // threads: 4 waves
constexpr int TM_G = 16;                   // right-hand sides per panel-solve workgroup (the MFMA M)
constexpr int TM_SB = 64;                  // columns per sub-block: 4 waves x one 16-column tile
constexpr int TM_BK = 32;                  // k-depth of one staged L tile
constexpr int TM_PADK = TM_BK + 2;         // NT stage [n][k]: row stride (conflict-free fragment reads)
constexpr int TM_PADN = TM_SB + 16;        // NN stage [k][n]: row stride (k rows 32 banks apart)
constexpr int TM_STAGE = TM_BK * TM_PADN;  // doubles per stage buffer
static_assert(TM_STAGE >= TM_SB * TM_PADK, "stage buffer holds either form");

// Two consecutive doubles, zero where masked (ok1 implies ok0).  Branch-free,
// so that the loads of a register ring stay in flight behind counted waits
// (a branch around a load makes the compiler drain every load at the join):
// a fully masked lane loads the always-valid, 16-byte aligned `safe` instead
// and discards it.  p is 16-byte aligned whenever ok0 (even leading
// dimensions, even column offsets); with ok0 && !ok1 the discarded second
// element is the row's pad element (even ld / ldb) or Linv's identity padding.
__device__ __forceinline__ double2 fetch2(const double* p, const double* safe, bool ok0, bool ok1) {
  double2 t = *reinterpret_cast<const double2*>(ok0 ? p : safe);
  t.x = ok0 ? t.x : 0.0;
  t.y = ok1 ? t.y : 0.0;
  return t;
}

// One 64 (n) x TM_BK (k) tile of the operator Op[k][n], global -> registers
// -> LDS.  NT: Op[k][n] = M[n * ldm + k] (rows n contiguous along k), NN:
// Op[k][n] = M[k * ldm + n] (rows k contiguous along n); n < nlim, k < kd,
// zero outside.
template <bool NN>
struct OpStage {
  static constexpr int Q = TM_SB * TM_BK / 2 / TM_NT;  // double2 per thread
  double2 r[Q];
  __device__ __forceinline__ void load(const double* __restrict__ M, int64_t ldm, int nlim, int kd, int kk) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = threadIdx.x + TM_NT * q;
      if (NN) {
        const int k = kk + ch / (TM_SB / 2), n = (ch % (TM_SB / 2)) * 2;
        r[q] = fetch2(M + (int64_t)k * ldm + n, M, k < kd && n < nlim, k < kd && n + 1 < nlim);
      } else {
        const int n = ch / (TM_BK / 2), k = kk + (ch % (TM_BK / 2)) * 2;
        r[q] = fetch2(M + (int64_t)n * ldm + k, M, n < nlim && k < kd, n < nlim && k + 1 < kd);
      }
    }
  }
  __device__ __forceinline__ void store(double* Ls) const {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = threadIdx.x + TM_NT * q;
      const int off = NN ? (ch / (TM_SB / 2)) * TM_PADN + (ch % (TM_SB / 2)) * 2
                         : (ch / (TM_BK / 2)) * TM_PADK + (ch % (TM_BK / 2)) * 2;
      *reinterpret_cast<double2*>(&Ls[off]) = r[q];
    }
  }
};

// dynamic LDS of the panel solve: the 16 x w slab of B, T of one diagonal
// block, two stage buffers
inline size_t panel_lds_bytes(int w, int nbi) {
  return (size_t)(TM_G * (w + 2) + TM_G * (nbi + 2) + 2 * TM_STAGE) * sizeof(double);
}

// The panel solve as a stream of products acc (16 x 64) = A (16 x kd, LDS) *
// Op (kd x 64, global): per diagonal block J (size bj, 64-column sub-blocks
// u), phase 0 the columns already solved in this panel times L's block row
// (forward) / block column (backward) of J, phase 1 T times Linv_J.  Where the
// operands are depends only on (J, phase, u), never on data, so the L chunks
// of later products are loaded while earlier ones are still multiplied.
struct PanelGeom {
  const double* K;
  int64_t ld;
  int N;
  const double* Linv;
  int nbi, p0, p1, SP, TP;
};
struct Prod {
  const double* M;  // Op's first element
  int64_t ldm;
  int nlim, kd;  // valid columns (of 64) and depth
  int aofs, lda;  // A: offset and row stride in the slab (phase 0) or in T (phase 1)
};
template <bool BWD>
__device__ __forceinline__ Prod panel_prod(const PanelGeom& g, int j0, int phase, int u) {
  Prod p;
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
    const double* LinvJ = g.Linv + (int64_t)(j0 / g.nbi) * g.nbi * g.nbi;
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
struct Cursor {
  int j0, phase, u, t, nch;
  bool valid;
  Prod p;
};
template <bool BWD>
__device__ __forceinline__ void cursor_next(const PanelGeom& g, Cursor& c) {
  if (++c.t < c.nch) return;
  c.t = 0;
  for (;;) {
    const int bj = g.N - c.j0 < g.nbi ? g.N - c.j0 : g.nbi;
    if (++c.u >= (bj + TM_SB - 1) / TM_SB) {
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
    c.p = panel_prod<BWD>(g, c.j0, c.phase, c.u);
    c.nch = (c.p.kd + TM_BK - 1) / TM_BK;
    if (c.nch > 0) return;  // (only the first block's phase 0 is empty, and the stream starts after it)
  }
}

constexpr int TM_PD = 4;  // L chunks in flight (a register ring): hides the load latency of the product chain

// Panel solve of columns [p0, min(p0 + w, N)) for right-hand sides
// [16 * blockIdx.x, +16): the slab lives in LDS from the first load to the
// last store.  One barrier per chunk: chunk c is written to LDS buffer c & 1,
// the barrier passed, the ring slot refilled with chunk c + TM_PD, chunk c
// multiplied; a product's result is written (T, or the slab) right after its
// last chunk, one barrier before anything reads it.
template <bool BWD>
__global__ __launch_bounds__(TM_NT) void trsm_panel_kernel(const double* __restrict__ K, int64_t ld, int N,
                                                           const double* __restrict__ Linv, int nbi, double* B,
                                                           int64_t ldb, int nrhs, int p0, int w) {
  extern __shared__ __attribute__((aligned(16))) double trsm_sm[];
  const int SP = w + 2, TP = nbi + 2;
  double* slab = trsm_sm;         // [16][SP]: B[:, P], overwritten block by block with the solution
  double* Ts = slab + TM_G * SP;  // [16][TP]: T of the current diagonal block
  double* Ls = Ts + TM_G * TP;    // [2][TM_STAGE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * TM_G;
  const int p1 = p0 + w < N ? p0 + w : N;
  const int hw = w / 2;
  const PanelGeom g = {K, ld, N, Linv, nbi, p0, p1, SP, TP};

  // the stream starts at phase 1 of the first block (its phase 0 is empty: T = B[:, J])
  const int jfirst = BWD ? p0 + ((p1 - p0 - 1) / nbi) * nbi : p0;
  Cursor cc;
  cc.j0 = jfirst;
  cc.phase = 1;
  cc.u = 0;
  cc.t = 0;
  cc.valid = true;
  cc.p = panel_prod<BWD>(g, jfirst, 1, 0);
  cc.nch = (cc.p.kd + TM_BK - 1) / TM_BK;
  Cursor lc = cc;
  OpStage<BWD> ring[TM_PD];
  // (past the end of the stream the ring still loads -- all lanes masked, the
  // product's first element -- and never branches around a load: only then
  // does the compiler keep the later slots in flight behind counted waits)
#pragma unroll
  for (int d = 0; d < TM_PD; ++d) {
    ring[d].load(lc.p.M, lc.p.ldm, lc.valid ? lc.p.nlim : 0, lc.p.kd, lc.t * TM_BK);
    if (lc.valid) cursor_next<BWD>(g, lc);
  }

  for (int idx = tid; idx < TM_G * hw; idx += TM_NT) {
    const int r = idx / hw, c = (idx % hw) * 2;
    const bool rok = r0 + r < nrhs;
    const double2 v = fetch2(B + (int64_t)(r0 + r) * ldb + p0 + c, B + (int64_t)r0 * ldb + p0, rok && p0 + c < p1,
                             rok && p0 + c + 1 < p1);
    *reinterpret_cast<double2*>(&slab[r * SP + c]) = v;
  }
  __syncthreads();
  for (int idx = tid; idx < TM_G * TP; idx += TM_NT) {
    const int r = idx / TP, c = idx % TP;
    Ts[idx] = c < nbi ? slab[r * SP + (jfirst - p0) + c] : 0.0;
  }

  const int col = 16 * wave + (lane & 15);  // this lane's column inside a sub-block
  const int frag = BWD ? (lane >> 4) * TM_PADN + col : col * TM_PADK + (lane >> 4);
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  int buf = 0;
  for (;;) {
#pragma unroll
    for (int d = 0; d < TM_PD; ++d) {
      if (!cc.valid) goto done;
      double* bs = Ls + buf * TM_STAGE;
      ring[d].store(bs);
      __syncthreads();
      ring[d].load(lc.p.M, lc.p.ldm, lc.valid ? lc.p.nlim : 0, lc.p.kd, lc.t * TM_BK);
      if (lc.valid) cursor_next<BWD>(g, lc);
      const double* As = (cc.phase == 0 ? slab : Ts) + cc.p.aofs + (lane & 15) * cc.p.lda + (lane >> 4) + cc.t * TM_BK;
#pragma unroll
      for (int s = 0; s < TM_BK / 4; ++s)
        acc = mfma_f64_16x16x4(As[4 * s], bs[frag + (BWD ? 4 * s * TM_PADN : 4 * s)], acc);
      if (cc.t == cc.nch - 1) {
        const int so = cc.j0 - p0 + TM_SB * cc.u + col;  // slab column
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = (lane >> 4) + 4 * r;
          if (cc.phase == 0) Ts[row * TP + TM_SB * cc.u + col] = slab[row * SP + so] - acc[r];
          else slab[row * SP + so] = acc[r];
        }
        acc = (double4_t){0.0, 0.0, 0.0, 0.0};
      }
      cursor_next<BWD>(g, cc);
      buf ^= 1;
    }
  }
done:
  __syncthreads();

  for (int idx = tid; idx < TM_G * hw; idx += TM_NT) {
    const int r = idx / hw, c = (idx % hw) * 2;
    if (r0 + r >= nrhs || p0 + c >= p1) continue;
    double* dst = B + (int64_t)(r0 + r) * ldb + p0 + c;
    if (p0 + c + 1 < p1) *reinterpret_cast<double2*>(dst) = *reinterpret_cast<const double2*>(&slab[r * SP + c]);
    else dst[0] = slab[r * SP + c];
  }
}

// between the sweeps: B[r][j] /= D[j] (a division, LinearSolvers.cpp:62-64)
__global__ __launch_bounds__(TM_NT) void trsm_scale_kernel(double* B, int64_t ldb, int nrhs, int N,
                                                           const double* __restrict__ D) {
  const int j = blockIdx.x * TM_NT + threadIdx.x;
  if (j >= N) return;
  const double d = D[j];
  for (int r = blockIdx.y; r < nrhs; r += gridDim.y) {
    double* p = B + (int64_t)r * ldb + j;
    *p = *p / d;
  }
}

// The updates between panel solves, C[i][j] -= sum_k X[i][k] Op[k][j] for
// i < M (right-hand sides), j < Nc, k < Kd:
//   forward  (NT)  Op[k][j] = L[j * ldl + k]: B[:, p1:] -= Y[:, P] L[p1:, P]^T
//   backward (NN)  Op[k][j] = L[k * ldl + j]: B[:, :p0] -= X[:, P] L[P, :p0]
// 64 x 64 tile, 8 waves in 2 x 4 (32 x 16 each: two waves per SIMD, so one
// wave's LDS reads and barrier wait run under the other's MFMAs), 16-deep
// k-chunks through two LDS buffers with one barrier per chunk as gemm.h's NT
// engine does, but UN_PD chunks in flight in a register ring: Kd is only one
// panel deep, so a tile is a short serial chain and nothing else hides its
// latencies.  The L tile is staged [j][k] (NT) or [k][j] (NN).  Workgroups
// that share an L tile (the right-hand-side groups of one column tile) have
// consecutive ids.
constexpr int UN_NT = 512, UN_BM = 64, UN_BN = 64, UN_BK = 16, UN_PADA = UN_BK + 2, UN_PADB = UN_BN + 16, UN_PD = 3;
constexpr int UN_BSTAGE = UN_BK * UN_PADB;
static_assert(UN_BSTAGE >= UN_BN * UN_PADA, "B stage buffer holds either form");
struct UpdStage {
  static constexpr int QA = UN_BM * UN_BK / 2 / UN_NT, QB = UN_BK * UN_BN / 2 / UN_NT;
  static_assert(QA * UN_NT * 2 == UN_BM * UN_BK && QB * UN_NT * 2 == UN_BK * UN_BN, "whole double2 chunks per thread");
  double2 ra[QA], rb[QB];
};
template <bool NN>
__global__ __launch_bounds__(UN_NT) void trsm_update_kernel(const double* X, int64_t ldx, const double* __restrict__ L,
                                                            int64_t ldl, double* C, int64_t ldc, int M, int Nc, int Kd,
                                                            int ntm) {
  __shared__ __attribute__((aligned(16))) double As[2][UN_BM * UN_PADA];
  __shared__ __attribute__((aligned(16))) double Bs[2][UN_BSTAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int i0 = (blockIdx.x % ntm) * UN_BM, j0 = (blockIdx.x / ntm) * UN_BN;
  auto load = [&](UpdStage& st, int kk) {
#pragma unroll
    for (int q = 0; q < UpdStage::QA; ++q) {
      const int ch = tid + UN_NT * q, i = i0 + ch / (UN_BK / 2), k = kk + (ch % (UN_BK / 2)) * 2;
      st.ra[q] = fetch2(X + (int64_t)i * ldx + k, X, i < M && k < Kd, i < M && k + 1 < Kd);
    }
#pragma unroll
    for (int q = 0; q < UpdStage::QB; ++q) {
      const int ch = tid + UN_NT * q;
      if (NN) {
        const int k = kk + ch / (UN_BN / 2), j = j0 + (ch % (UN_BN / 2)) * 2;
        st.rb[q] = fetch2(L + (int64_t)k * ldl + j, L, k < Kd && j < Nc, k < Kd && j + 1 < Nc);
      } else {
        const int j = j0 + ch / (UN_BK / 2), k = kk + (ch % (UN_BK / 2)) * 2;
        st.rb[q] = fetch2(L + (int64_t)j * ldl + k, L, j < Nc && k < Kd, j < Nc && k + 1 < Kd);
      }
    }
  };
  auto store = [&](const UpdStage& st, double* as, double* bs) {
#pragma unroll
    for (int q = 0; q < UpdStage::QA; ++q) {
      const int ch = tid + UN_NT * q;
      *reinterpret_cast<double2*>(&as[(ch / (UN_BK / 2)) * UN_PADA + (ch % (UN_BK / 2)) * 2]) = st.ra[q];
    }
#pragma unroll
    for (int q = 0; q < UpdStage::QB; ++q) {
      const int ch = tid + UN_NT * q;
      const int off = NN ? (ch / (UN_BN / 2)) * UN_PADB + (ch % (UN_BN / 2)) * 2
                         : (ch / (UN_BK / 2)) * UN_PADA + (ch % (UN_BK / 2)) * 2;
      *reinterpret_cast<double2*>(&bs[off]) = st.rb[q];
    }
  };
  double4_t acc[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) acc[a] = (double4_t){0.0, 0.0, 0.0, 0.0};
  const int nch = (Kd + UN_BK - 1) / UN_BK;
  UpdStage ring[UN_PD];
  // (loads past Kd are fully masked, never branched around: see trsm_panel_kernel)
#pragma unroll
  for (int d = 0; d < UN_PD; ++d) load(ring[d], d * UN_BK);
  const int aoff = (wr * 32 + (lane & 15)) * UN_PADA + (lane >> 4);
  const int boff = NN ? (lane >> 4) * UN_PADB + wc * 16 + (lane & 15) : (wc * 16 + (lane & 15)) * UN_PADA + (lane >> 4);
  for (int t0 = 0;; t0 += UN_PD) {
#pragma unroll
    for (int d = 0; d < UN_PD; ++d) {
      const int t = t0 + d;
      if (t >= nch) goto done;
      const int cur = t & 1;
      store(ring[d], As[cur], Bs[cur]);
      __syncthreads();
      load(ring[d], (t + UN_PD) * UN_BK);
      const double* as = As[cur];
      const double* bs = Bs[cur];
#pragma unroll
      for (int s = 0; s < UN_BK / 4; ++s) {
        const double bf = bs[boff + (NN ? 4 * s * UN_PADB : 4 * s)];
#pragma unroll
        for (int a = 0; a < 2; ++a) acc[a] = mfma_f64_16x16x4(as[aoff + a * 16 * UN_PADA + 4 * s], bf, acc[a]);
      }
    }
  }
done:
  const int j = j0 + wc * 16 + (lane & 15);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wr * 32 + a * 16 + (lane >> 4) + 4 * r;
      if (i < M && j < Nc) {
        double* cp = C + (int64_t)i * ldc + j;
        *cp = *cp - acc[a][r];
      }
    }
}

template <bool NN>
hipError_t launch_update(const double* X, int64_t ldx, const double* L, int64_t ldl, double* C, int64_t ldc, int M,
                         int Nc, int Kd, hipStream_t st) {
  const int ntm = (M + UN_BM - 1) / UN_BM, ntn = (Nc + UN_BN - 1) / UN_BN;
  hipLaunchKernelGGL((trsm_update_kernel<NN>), dim3((unsigned)(ntm * ntn)), dim3(UN_NT), 0, st, X, ldx, L, ldl, C, ldc,
                     M, Nc, Kd, ntm);
  return hipGetLastError();
}

template <bool BWD>
hipError_t launch_panel(const double* K, int64_t ld, int N, const double* Linv, int nbi, double* B, int64_t ldb,
                        int nrhs, int p0, int w, hipStream_t st) {
  // more than the 64 KB a kernel gets by default: raised once per process
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&trsm_panel_kernel<BWD>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)panel_lds_bytes(IPMZ_TRSM_PANEL_MAX, 128));
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL((trsm_panel_kernel<BWD>), dim3((nrhs + TM_G - 1) / TM_G), dim3(TM_NT), panel_lds_bytes(w, nbi),
                     st, K, ld, N, Linv, nbi, B, ldb, nrhs, p0, w);
  return hipGetLastError();
}

}  // namespace

hipError_t ldlt_solve_multi(const double* K, int64_t ld, int N, const double* D, const double* Linv, int nbi,
                            double* B, int64_t ldb, int nrhs, int w, hipStream_t st) {
  if (N <= 0 || nrhs <= 0) return hipSuccess;
  if ((nbi != 64 && nbi != 128) || w < nbi || w % 128 != 0 || w > IPMZ_TRSM_PANEL_MAX || (ld & 1) || (ldb & 1) ||
      ld < N || ldb < N || ((uintptr_t)K & 15) || ((uintptr_t)B & 15))
    return hipErrorInvalidValue;
  hipError_t e;
  for (int p0 = 0; p0 < N; p0 += w) {
    const int p1 = p0 + w < N ? p0 + w : N;
    if ((e = launch_panel<false>(K, ld, N, Linv, nbi, B, ldb, nrhs, p0, w, st)) != hipSuccess) return e;
    if (p1 < N &&  // B[:, p1:] -= Y[:, P] L[p1:, P]^T
        (e = launch_update<false>(B + p0, ldb, K + (int64_t)p1 * ld + p0, ld, B + p1, ldb, nrhs, N - p1, p1 - p0,
                                  st)) != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(trsm_scale_kernel, dim3((N + TM_NT - 1) / TM_NT, nrhs < 64 ? nrhs : 64), dim3(TM_NT), 0, st, B,
                     ldb, nrhs, N, D);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int p0 = ((N - 1) / w) * w; p0 >= 0; p0 -= w) {
    const int p1 = p0 + w < N ? p0 + w : N;
    if ((e = launch_panel<true>(K, ld, N, Linv, nbi, B, ldb, nrhs, p0, w, st)) != hipSuccess) return e;
    if (p0 > 0 &&  // B[:, :p0] -= X[:, P] L[P, :p0]
        (e = launch_update<true>(B + p0, ldb, K + (int64_t)p0 * ld, ld, B, ldb, nrhs, p0, p1 - p0, st)) != hipSuccess)
      return e;
  }
  return hipSuccess;
}

}  // namespace ipmz
