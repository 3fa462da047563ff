// The multi-right-hand-side solve of trsm.hip for the fp32 factor of the
// mixed-precision path (mixed.hip): every row of B (fp32, stride ldb) becomes
// L^{-T} D^{-1} L^{-1} b with L, D, Linv of ldlt_factor<float> (nbi = 64).
//
// The same right-looking algorithm over column panels of width w, the same
// launch sequence and the same roles (a panel-solve workgroup owns 16
// right-hand sides, an update workgroup one 64 x 64 output tile; stream order
// only, no spins / flags / tickets / atomics, bitwise reproducible) -- see the
// head of trsm.hip.  A sibling file, not a template of trsm.hip, so that the
// fp64 kernels' generated code cannot move.  What differs for 4-byte elements:
//
//   * products on v_mfma_f32_16x16x4_f32, whose accumulator holds rows
//     4 (lane >> 4) + r (Mfma<float>::row), not (lane >> 4) + 4 r;
//   * a 16-byte load carries 4 floats: column offsets, k offsets and every
//     leading dimension are multiples of 4 (ld a multiple of 64, ldb of 4, p0
//     of 128, Linv rows of 64 floats);
//   * LDS row strides re-derived for 4-byte banks (64 banks): a fragment read
//     has lanes (c = lane & 15, q = lane >> 4) at c * stride + q ([n][k]
//     stages, the slab, T) or q * stride + c ([k][n] stages).  c * 36 mod 64
//     runs over the 16 multiples of 4 and q fills the gaps; q * 80 mod 64 =
//     16 q.  So [n][k] rows are BK + 4 = 36 floats (slab w + 4, T 64 + 4: 4 c
//     mod 64) and [k][n] rows 64 + 16 = 80 floats, all multiples of 4 floats
//     for the 16-byte stores.
#include "common.h"
#include "kernels.h"

namespace ipmz {

namespace {

constexpr int SM_NT = 256;                 // threads: 4 waves
constexpr int SM_G = 16;                   // right-hand sides per panel-solve workgroup (the MFMA M)
constexpr int SM_SB = 64;                  // columns per sub-block: 4 waves x one 16-column tile
constexpr int SM_NBI = 64;                 // the mixed factor's inner block
constexpr int SM_BK = 32;                  // k-depth of one staged L tile
constexpr int SM_PADK = SM_BK + 4;         // NT stage [n][k]: row stride
constexpr int SM_PADN = SM_SB + 16;        // NN stage [k][n]: row stride
constexpr int SM_STAGE = SM_BK * SM_PADN;  // floats per stage buffer
static_assert(SM_STAGE >= SM_SB * SM_PADK, "stage buffer holds either form");

// Four consecutive floats, zero where masked (ok0 = the first is valid, nv =
// how many are).  Branch-free as trsm.hip's fetch2: a fully masked lane loads
// the always-valid, 16-byte aligned `safe` and discards it.  p is 16-byte
// aligned whenever ok0; the discarded tail of a partly valid load lies in the
// row's padding (ld a multiple of 64, ldb of 4) or Linv's identity padding.
__device__ __forceinline__ float4 fetch4(const float* p, const float* safe, bool ok0, int nv) {
  float4 t = *reinterpret_cast<const float4*>(ok0 ? p : safe);
  t.x = ok0 ? t.x : 0.0f;
  t.y = ok0 && nv > 1 ? t.y : 0.0f;
  t.z = ok0 && nv > 2 ? t.z : 0.0f;
  t.w = ok0 && nv > 3 ? t.w : 0.0f;
  return t;
}

// One 64 (n) x SM_BK (k) tile of the operator Op[k][n], global -> registers
// -> LDS.  NT: Op[k][n] = M[n * ldm + k], NN: Op[k][n] = M[k * ldm + n];
// n < nlim, k < kd, zero outside.
template <bool NN>
struct OpStage32 {
  static constexpr int Q = SM_SB * SM_BK / 4 / SM_NT;  // float4 per thread
  float4 r[Q];
  __device__ __forceinline__ void load(const float* __restrict__ M, int64_t ldm, int nlim, int kd, int kk) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = threadIdx.x + SM_NT * q;
      if (NN) {
        const int k = kk + ch / (SM_SB / 4), n = (ch % (SM_SB / 4)) * 4;
        r[q] = fetch4(M + (int64_t)k * ldm + n, M, k < kd && n < nlim, nlim - n);
      } else {
        const int n = ch / (SM_BK / 4), k = kk + (ch % (SM_BK / 4)) * 4;
        r[q] = fetch4(M + (int64_t)n * ldm + k, M, n < nlim && k < kd, kd - k);
      }
    }
  }
  __device__ __forceinline__ void store(float* Ls) const {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = threadIdx.x + SM_NT * q;
      const int off = NN ? (ch / (SM_SB / 4)) * SM_PADN + (ch % (SM_SB / 4)) * 4
                         : (ch / (SM_BK / 4)) * SM_PADK + (ch % (SM_BK / 4)) * 4;
      *reinterpret_cast<float4*>(&Ls[off]) = r[q];
    }
  }
};

// dynamic LDS of the panel solve: the 16 x w slab of B, T of one diagonal
// block, two stage buffers (57.9 KB at w = 512: inside the default 64 KB)
inline size_t panel_lds_bytes32(int w) {
  return (size_t)(SM_G * (w + 4) + SM_G * (SM_NBI + 4) + 2 * SM_STAGE) * sizeof(float);
}

// the panel solve as a stream of products (trsm.hip: PanelGeom, Prod, Cursor)
struct PanelGeom32 {
  const float* K;
  int64_t ld;
  int N;
  const float* Linv;
  int p0, p1, SP, TP;
};
struct Prod32 {
  const float* M;  // Op's first element
  int64_t ldm;
  int nlim, kd;   // valid columns (of 64) and depth
  int aofs, lda;  // A: offset and row stride in the slab (phase 0) or in T (phase 1)
};
template <bool BWD>
__device__ __forceinline__ Prod32 panel_prod32(const PanelGeom32& g, int j0, int phase) {
  Prod32 p;
  const int bj = g.N - j0 < SM_NBI ? g.N - j0 : SM_NBI;
  if (phase == 0) {
    p.nlim = bj;
    p.ldm = g.ld;
    p.lda = g.SP;
    if (BWD) {  // rows below the block, inside the panel
      const int je = j0 + SM_NBI;
      p.M = g.K + (int64_t)je * g.ld + j0;
      p.kd = g.p1 > je ? g.p1 - je : 0;
      p.aofs = je - g.p0;
    } else {  // columns of the panel left of the block
      p.M = g.K + (int64_t)j0 * g.ld + g.p0;
      p.kd = j0 - g.p0;
      p.aofs = 0;
    }
  } else {  // T times Linv_J (BWD) / Linv_J^T: the whole bj x bj block
    p.M = g.Linv + (int64_t)(j0 / SM_NBI) * SM_NBI * SM_NBI;
    p.nlim = bj;
    p.ldm = SM_NBI;
    p.lda = g.TP;
    p.kd = bj;
    p.aofs = 0;
  }
  return p;
}
// position in the stream: chunk t of product (j0, phase); nbi == SM_SB, so a
// diagonal block is one sub-block
struct Cursor32 {
  int j0, phase, t, nch;
  bool valid;
  Prod32 p;
};
template <bool BWD>
__device__ __forceinline__ void cursor_next32(const PanelGeom32& g, Cursor32& c) {
  if (++c.t < c.nch) return;
  c.t = 0;
  for (;;) {
    if (++c.phase > 1) {
      c.phase = 0;
      c.j0 += BWD ? -SM_NBI : SM_NBI;
      if (BWD ? c.j0 < g.p0 : c.j0 >= g.p1) {
        c.valid = false;
        return;
      }
    }
    c.p = panel_prod32<BWD>(g, c.j0, c.phase);
    c.nch = (c.p.kd + SM_BK - 1) / SM_BK;
    if (c.nch > 0) return;  // (only the first block's phase 0 is empty, and the stream starts after it)
  }
}

constexpr int SM_PD = 4;  // L chunks in flight (a register ring)

// Panel solve of columns [p0, min(p0 + w, N)) for right-hand sides
// [16 * blockIdx.x, +16): trsm_panel_kernel in fp32.
template <bool BWD>
__global__ __launch_bounds__(SM_NT) void trsm32_panel_kernel(const float* __restrict__ K, int64_t ld, int N,
                                                             const float* __restrict__ Linv, float* B, int64_t ldb,
                                                             int nrhs, int p0, int w) {
  extern __shared__ __attribute__((aligned(16))) float trsm32_sm[];
  const int SP = w + 4, TP = SM_NBI + 4;
  float* slab = trsm32_sm;       // [16][SP]: B[:, P], overwritten block by block with the solution
  float* Ts = slab + SM_G * SP;  // [16][TP]: T of the current diagonal block
  float* Ls = Ts + SM_G * TP;    // [2][SM_STAGE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * SM_G;
  const int p1 = p0 + w < N ? p0 + w : N;
  const int qw = w / 4;
  const PanelGeom32 g = {K, ld, N, Linv, p0, p1, SP, TP};

  // the stream starts at phase 1 of the first block (its phase 0 is empty: T = B[:, J])
  const int jfirst = BWD ? p0 + ((p1 - p0 - 1) / SM_NBI) * SM_NBI : p0;
  Cursor32 cc;
  cc.j0 = jfirst;
  cc.phase = 1;
  cc.t = 0;
  cc.valid = true;
  cc.p = panel_prod32<BWD>(g, jfirst, 1);
  cc.nch = (cc.p.kd + SM_BK - 1) / SM_BK;
  Cursor32 lc = cc;
  OpStage32<BWD> ring[SM_PD];
  // (past the end of the stream the ring still loads, all lanes masked: trsm.hip)
#pragma unroll
  for (int d = 0; d < SM_PD; ++d) {
    ring[d].load(lc.p.M, lc.p.ldm, lc.valid ? lc.p.nlim : 0, lc.p.kd, lc.t * SM_BK);
    if (lc.valid) cursor_next32<BWD>(g, lc);
  }

  for (int idx = tid; idx < SM_G * qw; idx += SM_NT) {
    const int r = idx / qw, c = (idx % qw) * 4;
    const bool rok = r0 + r < nrhs;
    const float4 v = fetch4(B + (int64_t)(r0 + r) * ldb + p0 + c, B + (int64_t)r0 * ldb + p0, rok && p0 + c < p1,
                            p1 - p0 - c);
    *reinterpret_cast<float4*>(&slab[r * SP + c]) = v;
  }
  __syncthreads();
  for (int idx = tid; idx < SM_G * TP; idx += SM_NT) {
    const int r = idx / TP, c = idx % TP;
    Ts[idx] = c < SM_NBI ? slab[r * SP + (jfirst - p0) + c] : 0.0f;
  }

  const int col = 16 * wave + (lane & 15);  // this lane's column inside the block
  const int frag = BWD ? (lane >> 4) * SM_PADN + col : col * SM_PADK + (lane >> 4);
  float4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
  int buf = 0;
  for (;;) {
#pragma unroll
    for (int d = 0; d < SM_PD; ++d) {
      if (!cc.valid) goto done;
      float* bs = Ls + buf * SM_STAGE;
      ring[d].store(bs);
      __syncthreads();
      ring[d].load(lc.p.M, lc.p.ldm, lc.valid ? lc.p.nlim : 0, lc.p.kd, lc.t * SM_BK);
      if (lc.valid) cursor_next32<BWD>(g, lc);
      const float* As = (cc.phase == 0 ? slab : Ts) + cc.p.aofs + (lane & 15) * cc.p.lda + (lane >> 4) + cc.t * SM_BK;
#pragma unroll
      for (int s = 0; s < SM_BK / 4; ++s)
        acc = Mfma<float>::mma(As[4 * s], bs[frag + (BWD ? 4 * s * SM_PADN : 4 * s)], acc);
      if (cc.t == cc.nch - 1) {
        const int so = cc.j0 - p0 + col;  // slab column
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = Mfma<float>::row(lane, r);
          if (cc.phase == 0) Ts[row * TP + col] = slab[row * SP + so] - acc[r];
          else slab[row * SP + so] = acc[r];
        }
        acc = (float4_t){0.0f, 0.0f, 0.0f, 0.0f};
      }
      cursor_next32<BWD>(g, cc);
      buf ^= 1;
    }
  }
done:
  __syncthreads();

  for (int idx = tid; idx < SM_G * qw; idx += SM_NT) {
    const int r = idx / qw, c = (idx % qw) * 4;
    if (r0 + r >= nrhs || p0 + c >= p1) continue;
    float* dst = B + (int64_t)(r0 + r) * ldb + p0 + c;
    const float* src = &slab[r * SP + c];
    if (p0 + c + 3 < p1) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
    else
      for (int e = 0; p0 + c + e < p1; ++e) dst[e] = src[e];
  }
}

// between the sweeps: B[r][j] /= D[j]
__global__ __launch_bounds__(SM_NT) void trsm32_scale_kernel(float* B, int64_t ldb, int nrhs, int N,
                                                             const float* __restrict__ D) {
  const int j = blockIdx.x * SM_NT + threadIdx.x;
  if (j >= N) return;
  const float d = D[j];
  for (int r = blockIdx.y; r < nrhs; r += gridDim.y) {
    float* p = B + (int64_t)r * ldb + j;
    *p = *p / d;
  }
}

// The updates between panel solves (trsm_update_kernel in fp32):
// C[i][j] -= sum_k X[i][k] Op[k][j], i < M, j < Nc, k < Kd, NT or NN.  64 x 64
// tile, 8 waves in 2 x 4 (32 x 16 each), 32-deep k-chunks (one float4 of X
// and one of L per thread) through two LDS buffers with one barrier per chunk,
// S2_PD chunks in flight in a register ring.
constexpr int S2_NT = 512, S2_BM = 64, S2_BN = 64, S2_BK = 32, S2_PADA = S2_BK + 4, S2_PADB = S2_BN + 16, S2_PD = 3;
constexpr int S2_BSTAGE = S2_BK * S2_PADB;
static_assert(S2_BSTAGE >= S2_BN * S2_PADA, "B stage buffer holds either form");
static_assert(S2_BM * S2_BK / 4 == S2_NT && S2_BK * S2_BN / 4 == S2_NT, "one float4 of each operand per thread");
struct UpdStage32 {
  float4 ra, rb;
};
template <bool NN>
__global__ __launch_bounds__(S2_NT) void trsm32_update_kernel(const float* X, int64_t ldx, const float* __restrict__ L,
                                                              int64_t ldl, float* C, int64_t ldc, int M, int Nc,
                                                              int Kd, int ntm) {
  __shared__ __attribute__((aligned(16))) float As[2][S2_BM * S2_PADA];
  __shared__ __attribute__((aligned(16))) float Bs[2][S2_BSTAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int i0 = (blockIdx.x % ntm) * S2_BM, j0 = (blockIdx.x / ntm) * S2_BN;
  auto load = [&](UpdStage32& st, int kk) {
    {
      const int i = i0 + tid / (S2_BK / 4), k = kk + (tid % (S2_BK / 4)) * 4;
      st.ra = fetch4(X + (int64_t)i * ldx + k, X, i < M && k < Kd, Kd - k);
    }
    if (NN) {
      const int k = kk + tid / (S2_BN / 4), j = j0 + (tid % (S2_BN / 4)) * 4;
      st.rb = fetch4(L + (int64_t)k * ldl + j, L, k < Kd && j < Nc, Nc - j);
    } else {
      const int j = j0 + tid / (S2_BK / 4), k = kk + (tid % (S2_BK / 4)) * 4;
      st.rb = fetch4(L + (int64_t)j * ldl + k, L, j < Nc && k < Kd, Kd - k);
    }
  };
  auto store = [&](const UpdStage32& st, float* as, float* bs) {
    *reinterpret_cast<float4*>(&as[(tid / (S2_BK / 4)) * S2_PADA + (tid % (S2_BK / 4)) * 4]) = st.ra;
    const int off = NN ? (tid / (S2_BN / 4)) * S2_PADB + (tid % (S2_BN / 4)) * 4
                       : (tid / (S2_BK / 4)) * S2_PADA + (tid % (S2_BK / 4)) * 4;
    *reinterpret_cast<float4*>(&bs[off]) = st.rb;
  };
  float4_t acc[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) acc[a] = (float4_t){0.0f, 0.0f, 0.0f, 0.0f};
  const int nch = (Kd + S2_BK - 1) / S2_BK;
  UpdStage32 ring[S2_PD];
  // (loads past Kd are fully masked, never branched around)
#pragma unroll
  for (int d = 0; d < S2_PD; ++d) load(ring[d], d * S2_BK);
  const int aoff = (wr * 32 + (lane & 15)) * S2_PADA + (lane >> 4);
  const int boff = NN ? (lane >> 4) * S2_PADB + wc * 16 + (lane & 15) : (wc * 16 + (lane & 15)) * S2_PADA + (lane >> 4);
  for (int t0 = 0;; t0 += S2_PD) {
#pragma unroll
    for (int d = 0; d < S2_PD; ++d) {
      const int t = t0 + d;
      if (t >= nch) goto done;
      const int cur = t & 1;
      store(ring[d], As[cur], Bs[cur]);
      __syncthreads();
      load(ring[d], (t + S2_PD) * S2_BK);
      const float* as = As[cur];
      const float* bs = Bs[cur];
#pragma unroll
      for (int s = 0; s < S2_BK / 4; ++s) {
        const float bf = bs[boff + (NN ? 4 * s * S2_PADB : 4 * s)];
#pragma unroll
        for (int a = 0; a < 2; ++a) acc[a] = Mfma<float>::mma(as[aoff + a * 16 * S2_PADA + 4 * s], bf, acc[a]);
      }
    }
  }
done:
  const int j = j0 + wc * 16 + (lane & 15);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + wr * 32 + a * 16 + Mfma<float>::row(lane, r);
      if (i < M && j < Nc) {
        float* cp = C + (int64_t)i * ldc + j;
        *cp = *cp - acc[a][r];
      }
    }
}

template <bool NN>
hipError_t launch_update32(const float* X, int64_t ldx, const float* L, int64_t ldl, float* C, int64_t ldc, int M,
                           int Nc, int Kd, hipStream_t st) {
  const int ntm = (M + S2_BM - 1) / S2_BM, ntn = (Nc + S2_BN - 1) / S2_BN;
  hipLaunchKernelGGL((trsm32_update_kernel<NN>), dim3((unsigned)(ntm * ntn)), dim3(S2_NT), 0, st, X, ldx, L, ldl, C,
                     ldc, M, Nc, Kd, ntm);
  return hipGetLastError();
}

template <bool BWD>
hipError_t launch_panel32(const float* K, int64_t ld, int N, const float* Linv, float* B, int64_t ldb, int nrhs,
                          int p0, int w, hipStream_t st) {
  hipLaunchKernelGGL((trsm32_panel_kernel<BWD>), dim3((nrhs + SM_G - 1) / SM_G), dim3(SM_NT), panel_lds_bytes32(w), st,
                     K, ld, N, Linv, B, ldb, nrhs, p0, w);
  return hipGetLastError();
}

}  // namespace

hipError_t ldlt_solve_multi(const float* K, int64_t ld, int N, const float* D, const float* Linv, float* B,
                            int64_t ldb, int nrhs, int w, hipStream_t st) {
  if (N <= 0 || nrhs <= 0) return hipSuccess;
  if (w < 128 || w % 128 != 0 || w > IPMZ_TRSM_PANEL_MAX || (ld & 63) || (ldb & 3) || ld < N || ldb < N ||
      ((uintptr_t)K & 15) || ((uintptr_t)B & 15) || ((uintptr_t)Linv & 15))
    return hipErrorInvalidValue;
  hipError_t e;
  for (int p0 = 0; p0 < N; p0 += w) {
    const int p1 = p0 + w < N ? p0 + w : N;
    if ((e = launch_panel32<false>(K, ld, N, Linv, B, ldb, nrhs, p0, w, st)) != hipSuccess) return e;
    if (p1 < N &&  // B[:, p1:] -= Y[:, P] L[p1:, P]^T
        (e = launch_update32<false>(B + p0, ldb, K + (int64_t)p1 * ld + p0, ld, B + p1, ldb, nrhs, N - p1, p1 - p0,
                                    st)) != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(trsm32_scale_kernel, dim3((N + SM_NT - 1) / SM_NT, nrhs < 64 ? nrhs : 64), dim3(SM_NT), 0, st, B,
                     ldb, nrhs, N, D);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int p0 = ((N - 1) / w) * w; p0 >= 0; p0 -= w) {
    const int p1 = p0 + w < N ? p0 + w : N;
    if ((e = launch_panel32<true>(K, ld, N, Linv, B, ldb, nrhs, p0, w, st)) != hipSuccess) return e;
    if (p0 > 0 &&  // B[:, :p0] -= X[:, P] L[P, :p0]
        (e = launch_update32<true>(B + p0, ldb, K + (int64_t)p0 * ld, ld, B, ldb, nrhs, p0, p1 - p0, st)) != hipSuccess)
      return e;
  }
  return hipSuccess;
}

}  // namespace ipmz
