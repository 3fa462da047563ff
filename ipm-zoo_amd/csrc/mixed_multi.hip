// Mixed-precision solve for many right-hand sides: the refinement of
// mixed.hip with every right-hand side a row of B (stride ldb),
//
//   x = 0, r = b                                       (per row)
//   pass: d = (S K S)^{-1}_{fp32} fp32(S r)            blocked fp32 solve, trsm.hip
//         x += S d                                     rows still running
//         r = b - x K (fp64), ratio = max|r| / max|b|  sym_residual_kernel + k_mm_check
//         a row with ratio <= tol is FROZEN: its x, ratio and correction
//         count never change again and its next fp32 right-hand side is zero
//   until every row is frozen or max_refine corrections are applied.
//
// The residual R = B - X K reads only the lower triangle of the symmetric K
// and runs on v_mfma_f64_16x16x4_f64 with the rows as the MFMA M: a workgroup
// owns a 64-row x 64-column output tile J and walks all of k in 16-deep chunks,
// first the columns up to and including the tile's own (NT form, Op[k][j] =
// K[j * ld + k], k <= j), then the rows from the tile's own down (NN form,
// Op[k][j] = K[k * ld + j], k > j).  The triangle masks k <= j / k > j are
// applied to every chunk: they only bite in the diagonal tile, which so
// contributes both halves with the diagonal counted once.  trsm_update_kernel's
// staging is the model: a register ring of chunks in flight, two LDS buffers,
// one barrier per chunk.  The chunk order of a tile depends on (j0, N) alone,
// every output element is summed by one lane in that order, maxima are
// maxima: no atomics, no cross-workgroup partial sums, bitwise reproducible,
// and a row's result does not depend on which other rows are in the call.
//
// The stop test is per row; after each pass the host reads one all-stopped
// word (a pass that returns at once would still cost its launches: hundreds
// at N = 16384), so mixed_solve_multi blocks the host and cannot be captured.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace ipmz {

namespace {

constexpr int MM_NT = 256;

// max over the 16 lanes of a DPP row (the lanes that hold one accumulator row)
__device__ __forceinline__ double row16_max(double v) {
  v = fmax(v, dpp_double<0xb1>(v));   // quad_perm [1,0,3,2]
  v = fmax(v, dpp_double<0x4e>(v));   // quad_perm [2,3,0,1]
  v = fmax(v, dpp_double<0x124>(v));  // row_ror:4
  v = fmax(v, dpp_double<0x128>(v));  // row_ror:8
  return v;
}

constexpr int SR_NT = 512, SR_BM = 64, SR_BN = 64, SR_BK = 16, SR_PADA = SR_BK + 2, SR_PADB = SR_BN + 16, SR_PD = 3;
constexpr int SR_BSTAGE = SR_BK * SR_PADB;
static_assert(SR_BSTAGE >= SR_BN * SR_PADA, "B stage buffer holds either form");
static_assert(SR_BM * SR_BK / 2 == SR_NT && SR_BK * SR_BN / 2 == SR_NT, "one double2 of each operand per thread");
struct ResStage {
  double2 ra, rb;
};

// R[i][j] = B[i][j] - sum_k X[i][k] Ksym[k][j], i < M, j < N.  8 waves in
// 2 x 4 (32 x 16 each).  Optional outputs (null = not wanted):
//   R     the residual (may alias B: an element is read and written by one lane)
//   r32   fp32(s_j r_ij), the next fp32 right-hand side, rows with done[i] == 0
//   part  [i][tile][2] = max_j |r_ij|, max_j |b_ij| over the tile's columns
// done (with part / r32): a tile whose rows are all frozen returns at once.
__global__ __launch_bounds__(SR_NT) void sym_residual_kernel(const double* __restrict__ K, int64_t ld, int N,
                                                             const double* X, int64_t ldx, const double* B, int64_t ldb,
                                                             double* R, int64_t ldr, int M, int ntm,
                                                             const double* __restrict__ s, float* r32, int64_t ld32,
                                                             double* part, const unsigned* done) {
  __shared__ __attribute__((aligned(16))) double As[2][SR_BM * SR_PADA];
  __shared__ __attribute__((aligned(16))) double Bs[2][SR_BSTAGE];
  __shared__ double red[4][SR_BM][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int i0 = (blockIdx.x % ntm) * SR_BM, jt = blockIdx.x / ntm, j0 = jt * SR_BN;
  if (done) {
    const int i = i0 + (tid & 63);
    if (!__syncthreads_or(i < M && !done[i])) return;
  }
  const int jend = j0 + SR_BN < N ? j0 + SR_BN : N;
  const int ntNT = (jend + SR_BK - 1) / SR_BK;  // k in [0, jend): stored at row j
  const int nch = ntNT + (N - j0 + SR_BK - 1) / SR_BK;  // k in [j0, N): stored at row k
  // operand positions of this thread inside a chunk, either form
  const int ai = i0 + tid / (SR_BK / 2), ak = (tid % (SR_BK / 2)) * 2;
  const int ntr = j0 + tid / (SR_BK / 2), ntc = (tid % (SR_BK / 2)) * 2;   // NT: row j, column kk + ..
  const int nnr = tid / (SR_BN / 2), nnc = j0 + (tid % (SR_BN / 2)) * 2;  // NN: row kk + .., column j
  const int soffNT = (tid / (SR_BK / 2)) * SR_PADA + (tid % (SR_BK / 2)) * 2;
  const int soffNN = (tid / (SR_BN / 2)) * SR_PADB + (tid % (SR_BN / 2)) * 2;
  auto load = [&](ResStage& st, int t) {
    const bool live = t < nch, nn = t >= ntNT;
    const int kk = nn ? j0 + (t - ntNT) * SR_BK : t * SR_BK;
    const int k = kk + ak;
    st.ra = fetch16(X + (int64_t)ai * ldx + k, X, live && ai < M && k < N, N - k);
    const int row = nn ? kk + nnr : ntr, col = nn ? nnc : kk + ntc;
    // the lower triangle only: NT takes k <= j, NN k > j (col + 1 < ld: ld is even)
    const int cend = nn ? row : row + 1;
    st.rb = fetch16(K + (int64_t)row * ld + col, K, live && row < N && col < cend, cend - col);
  };
  auto store = [&](const ResStage& st, int t, double* as, double* bs) {
    *reinterpret_cast<double2*>(&as[soffNT]) = st.ra;
    *reinterpret_cast<double2*>(&bs[t >= ntNT ? soffNN : soffNT]) = st.rb;
  };
  double4_t acc[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) acc[a] = (double4_t){0.0, 0.0, 0.0, 0.0};
  ResStage ring[SR_PD];
  // (loads past the last chunk are fully masked, never branched around: trsm.hip)
#pragma unroll
  for (int d = 0; d < SR_PD; ++d) load(ring[d], d);
  const int aoff = (wr * 32 + (lane & 15)) * SR_PADA + (lane >> 4);
  const int boffNN = (lane >> 4) * SR_PADB + wc * 16 + (lane & 15);
  const int boffNT = (wc * 16 + (lane & 15)) * SR_PADA + (lane >> 4);
  for (int t0 = 0;; t0 += SR_PD) {
#pragma unroll
    for (int d = 0; d < SR_PD; ++d) {
      const int t = t0 + d;
      if (t >= nch) goto done_k;
      const int cur = t & 1;
      store(ring[d], t, As[cur], Bs[cur]);
      __syncthreads();
      load(ring[d], t + SR_PD);
      const double* as = As[cur];
      const double* bs = Bs[cur] + (t >= ntNT ? boffNN : boffNT);
      const int bstep = t >= ntNT ? 4 * SR_PADB : 4;
#pragma unroll
      for (int q = 0; q < SR_BK / 4; ++q) {
        const double bf = bs[q * bstep];
#pragma unroll
        for (int a = 0; a < 2; ++a) acc[a] = mfma_f64_16x16x4(as[aoff + a * 16 * SR_PADA + 4 * q], bf, acc[a]);
      }
    }
  }
done_k:
  const int j = j0 + wc * 16 + (lane & 15);
  const double sj = (r32 && j < N) ? s[j] : 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int il = wr * 32 + a * 16 + (lane >> 4) + 4 * r, i = i0 + il;
      double rr = 0.0, bb = 0.0;
      if (i < M && j < N) {
        const double b = B[(int64_t)i * ldb + j];
        const double v = b - acc[a][r];
        if (R) R[(int64_t)i * ldr + j] = v;
        if (r32 && !done[i]) r32[(int64_t)i * ld32 + j] = (float)(sj * v);
        rr = fabs(v);
        bb = fabs(b);
      }
      if (part) {
        rr = row16_max(rr);
        bb = row16_max(bb);
        if ((lane & 15) == 0) {
          red[wc][il][0] = rr;
          red[wc][il][1] = bb;
        }
      }
    }
  if (!part) return;
  __syncthreads();
  if (tid < 2 * SR_BM) {
    const int il = tid >> 1, c = tid & 1, i = i0 + il;
    const int ntn = gridDim.x / ntm;
    if (i < M)
      part[((int64_t)i * ntn + jt) * 2 + c] =
          fmax(fmax(red[0][il][c], red[1][il][c]), fmax(red[2][il][c], red[3][il][c]));
  }
}

// x = 0, r32 = fp32(S b), per-row state reset
__global__ __launch_bounds__(MM_NT) void k_mm_begin(int N, int nrhs, const double* __restrict__ B, int64_t ldb,
                                                    const double* __restrict__ s, double* __restrict__ x, int64_t ldx,
                                                    float* __restrict__ r32, int64_t ld32, unsigned* __restrict__ done,
                                                    double* __restrict__ stat) {
  const int j = blockIdx.x * MM_NT + threadIdx.x;
  for (int r = blockIdx.y; r < nrhs; r += gridDim.y) {
    if (j < N) {
      x[(int64_t)r * ldx + j] = 0.0;
      r32[(int64_t)r * ld32 + j] = (float)(s[j] * B[(int64_t)r * ldb + j]);
    }
    if (j == 0) {
      done[r] = 0u;
      stat[2 * r] = 0.0;
      stat[2 * r + 1] = 0.0;
    }
  }
}

// x += S d for the rows still running (d: the fp32 solve's output, in r32)
__global__ __launch_bounds__(MM_NT) void k_mm_accum(int N, int nrhs, const double* __restrict__ s,
                                                    const float* __restrict__ d, int64_t ld32, double* __restrict__ x,
                                                    int64_t ldx, const unsigned* __restrict__ done) {
  const int j = blockIdx.x * MM_NT + threadIdx.x;
  if (j >= N) return;
  const double sj = s[j];
  for (int r = blockIdx.y; r < nrhs; r += gridDim.y)
    if (!done[r]) x[(int64_t)r * ldx + j] += sj * (double)d[(int64_t)r * ld32 + j];
}

// The stop test of k_mx_check per row (one wave each): ratio = bb > 0 ? rr /
// bb : rr, stat = {ratio, corrections applied}; a row with ratio <= tol is
// frozen from here on and its next fp32 right-hand side zeroed.
__global__ __launch_bounds__(MM_NT) void k_mm_check(int N, int nrhs, int ntiles, const double* __restrict__ part,
                                                    double tol, int pass, unsigned* __restrict__ done,
                                                    double* __restrict__ stat, float* __restrict__ r32, int64_t ld32) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * (MM_NT / 64) + (threadIdx.x >> 6);
  if (r >= nrhs || done[r]) return;
  double rr = 0.0, bb = 0.0;
  for (int t = lane; t < ntiles; t += 64) {
    rr = fmax(rr, part[((int64_t)r * ntiles + t) * 2]);
    bb = fmax(bb, part[((int64_t)r * ntiles + t) * 2 + 1]);
  }
  rr = wave_max(rr);
  bb = wave_max(bb);
  const double ratio = bb > 0.0 ? rr / bb : rr;
  if (lane == 0) {
    stat[2 * r] = ratio;
    stat[2 * r + 1] = (double)pass;
  }
  if (ratio <= tol) {
    for (int j = lane; j < N; j += 64) r32[(int64_t)r * ld32 + j] = 0.0f;
    if (lane == 0) done[r] = 1u;
  }
}

// word[0] = every row is frozen
__global__ __launch_bounds__(MM_NT) void k_mm_all(int nrhs, const unsigned* __restrict__ done,
                                                  unsigned* __restrict__ word) {
  int running = 0;
  for (int r = threadIdx.x; r < nrhs; r += MM_NT) running |= done[r] ? 0 : 1;
  running = __syncthreads_or(running);
  if (threadIdx.x == 0) word[0] = running ? 0u : 1u;
}

__global__ __launch_bounds__(MM_NT) void k_mm_finish(int N, int nrhs, const double* __restrict__ x, int64_t ldx,
                                                     double* __restrict__ B, int64_t ldb) {
  const int j = blockIdx.x * MM_NT + threadIdx.x;
  if (j >= N) return;
  for (int r = blockIdx.y; r < nrhs; r += gridDim.y) B[(int64_t)r * ldb + j] = x[(int64_t)r * ldx + j];
}

hipError_t launch_residual(const double* K, int64_t ld, int N, const double* X, int64_t ldx, const double* B,
                           int64_t ldb, double* R, int64_t ldr, int nrhs, const double* s, float* r32, int64_t ld32,
                           double* part, const unsigned* done, hipStream_t st) {
  const int ntm = (nrhs + SR_BM - 1) / SR_BM, ntn = (N + SR_BN - 1) / SR_BN;
  hipLaunchKernelGGL(sym_residual_kernel, dim3((unsigned)(ntm * ntn)), dim3(SR_NT), 0, st, K, ld, N, X, ldx, B, ldb, R,
                     ldr, nrhs, ntm, s, r32, ld32, part, done);
  return hipGetLastError();
}

}  // namespace

int64_t mixed_multi_ws_carve(char* base, int N, int nrhs, MixedMultiWs& m) {
  Carver c{base};
  m.ldx = (N + 1) / 2 * 2;
  m.ld32 = (N + 63) / 64 * 64;
  m.ntiles = (N + SR_BN - 1) / SR_BN;
  m.x = c.take<double>((int64_t)nrhs * m.ldx);
  m.r32 = c.take<float>((int64_t)nrhs * m.ld32);
  m.part = c.take<double>((int64_t)nrhs * m.ntiles * 2);
  m.stat = c.take<double>((int64_t)nrhs * 2);
  m.done = c.take<unsigned>(nrhs);
  m.word = c.take<unsigned>(16);
  return c.off;
}

hipError_t sym_residual_multi(const double* K, int64_t ld, int N, const double* X, int64_t ldx, const double* B,
                              int64_t ldb, double* R, int64_t ldr, int nrhs, hipStream_t st) {
  if (N <= 0 || nrhs <= 0) return hipSuccess;
  if ((ld & 1) || (ldx & 1) || ld < N || ldx < N || ldb < N || ldr < N || ((uintptr_t)K & 15) || ((uintptr_t)X & 15))
    return hipErrorInvalidValue;
  return launch_residual(K, ld, N, X, ldx, B, ldb, R, ldr, nrhs, nullptr, nullptr, 0, nullptr, nullptr, st);
}

hipError_t mixed_solve_multi(const double* K, int64_t ld, const MixedWs& w, const MixedMultiWs& m, double* B,
                             int64_t ldb, int nrhs, double tol, int max_refine, int pw, hipStream_t st) {
  const int N = w.N;
  if (N <= 0 || nrhs <= 0) return hipSuccess;
  if ((ld & 1) || ld < N || ldb < N || ((uintptr_t)K & 15)) return hipErrorInvalidValue;
  const dim3 gv((N + MM_NT - 1) / MM_NT, nrhs < 1024 ? nrhs : 1024), bt(MM_NT);
  hipError_t e;
  hipLaunchKernelGGL(k_mm_begin, gv, bt, 0, st, N, nrhs, B, ldb, w.s, m.x, m.ldx, m.r32, m.ld32, m.done, m.stat);
  for (int pass = 0; pass <= max_refine; ++pass) {
    if ((e = ldlt_solve_multi(w.K32, w.ld32, N, w.D32, w.Linv32, 64, m.r32, m.ld32, nrhs, pw, st)) != hipSuccess)
      return e;
    hipLaunchKernelGGL(k_mm_accum, gv, bt, 0, st, N, nrhs, w.s, m.r32, m.ld32, m.x, m.ldx, m.done);
    if ((e = launch_residual(K, ld, N, m.x, m.ldx, B, ldb, nullptr, 0, nrhs, w.s, m.r32, m.ld32, m.part, m.done,
                             st)) != hipSuccess)
      return e;
    hipLaunchKernelGGL(k_mm_check, dim3((nrhs + MM_NT / 64 - 1) / (MM_NT / 64)), bt, 0, st, N, nrhs, m.ntiles, m.part,
                       tol, pass, m.done, m.stat, m.r32, m.ld32);
    hipLaunchKernelGGL(k_mm_all, dim3(1), bt, 0, st, nrhs, m.done, m.word);
    unsigned all = 0;
    if ((e = hipMemcpyAsync(&all, m.word, sizeof(unsigned), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (all) break;
  }
  hipLaunchKernelGGL(k_mm_finish, gv, bt, 0, st, N, nrhs, m.x, m.ldx, B, ldb);
  return hipGetLastError();
}

}  // namespace ipmz
