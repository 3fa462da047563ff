// Newton-step kernels around the factorization: synthetic QP generation,
// build_environment's initial iterate, residual (shorthand) vectors,
// KKT assembly, augmented rhs, eliminated-variable back-substitution, ratio
// tests, mu / sigma, corrector residuals and the iterate update; and the rhs,
// back-substitution and ratio test of a caller's block of residual vectors
// (ipmz_*_newton_solve_multi), the same formulas over another accessor.
//
// Formulations (tests/golden/formulations.txt is the reference's own
// symbolic output these formulas restate): InequalityHandling::SlackedSlacks
// (default) or ::Slacks, one-sided / absent inequality and variable bounds,
// EqualityHandling Regularization / None / PenaltyFunction.  The flags are
// per QP and uniform inside a launch.  The
// element-wise formulas keep the reference evaluator's operand order
// (Evaluation.cpp:102-176) and the library is built with -ffp-contract=off,
// so they round exactly like oracle/ipmz_oracle.cpp; only the reductions
// (matvecs, norms, means) and the factor/solve change summation order.
//
// Everything here is HBM-bound O(n^2) (matvecs, assembly) or O(N) work.
#include <type_traits>

#include "common.h"
#include "data_terms.h"  // a_dual: the vector A^T multiplies in r_x
#include "kernels.h"
#include "sync.h"
#include "trsv_small.h"

namespace ipmz {

namespace {
constexpr int NT = 256;
constexpr int RED_BLOCKS = 512;  // partial-reduction grid
enum : uint64_t { TAG_Q = 1, TAG_C = 2, TAG_A = 3, TAG_C_EQ = 4, TAG_D = 5 };

__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < NT / 64; ++w) t += sh[w];
  return t;  // valid in thread 0
}
__device__ __forceinline__ double block_min(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_min(v);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 1.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < NT / 64; ++w) t = fmin(t, sh[w]);
  return t;
}
// every thread gets the result (fused per-QP kernels); deterministic order
template <int NTH>
__device__ __forceinline__ double block_allsum(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < NTH / 64; ++w) t += sh[w];
  __syncthreads();  // sh reusable
  return t;
}
template <int NTH>
__device__ __forceinline__ double block_allmin(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_min(v);
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 1.0;
  for (int w = 0; w < NTH / 64; ++w) t = fmin(t, sh[w]);
  __syncthreads();
  return t;
}
}  // namespace

// ---------------------------------------------------------------------------
// Generator, bit-identical to the oracle's generator.  Matrices are
// written row-major with leading dimension n.
__global__ void k_gen_Q(const QPDev* __restrict__ qs, uint64_t seed0) {
  const QPDev& q = qs[blockIdx.y];
  const int n = q.n;
  const int64_t ld = q.ldn;
  const uint64_t seed = seed0 + blockIdx.y;
  double* Q = const_cast<double*>(q.Q);
  const int64_t total = (int64_t)n * n;
  for (int64_t t = blockIdx.x * (int64_t)NT + threadIdx.x; t < total; t += (int64_t)gridDim.x * NT) {
    const int64_t i = t / n, j = t % n;
    double v;
    if (i == j) v = 1.0 + ipmz_u01(seed, TAG_Q, i, i);
    else if (j < i) v = (2.0 * ipmz_u01(seed, TAG_Q, i, j) - 1.0) / (double)n;
    else v = (2.0 * ipmz_u01(seed, TAG_Q, j, i) - 1.0) / (double)n;
    Q[i * ld + j] = v;
  }
}
__global__ void k_gen_rect(const QPDev* __restrict__ qs, uint64_t seed0, int which) {
  const QPDev& q = qs[blockIdx.y];
  const int n = q.n, rows = which ? q.p_usr : q.m_usr;
  const int64_t ld = q.ldn;
  const uint64_t seed = seed0 + blockIdx.y, tag = which ? TAG_C_EQ : TAG_A;
  double* M = const_cast<double*>(which ? q.C : q.A);
  const int64_t total = (int64_t)rows * n;
  const double sn = sqrt((double)n);
  for (int64_t t = blockIdx.x * (int64_t)NT + threadIdx.x; t < total; t += (int64_t)gridDim.x * NT) {
    const int64_t i = t / n, j = t % n;
    M[i * ld + j] = (2.0 * ipmz_u01(seed, tag, i, j) - 1.0) / sn;
  }
}
__global__ void k_gen_vec(const QPDev* __restrict__ qs, uint64_t seed0) {
  const QPDev& q = qs[blockIdx.y];
  const int n = q.n, m = q.m_usr, p = q.p_usr;
  const uint64_t seed = seed0 + blockIdx.y;
  double *c = const_cast<double*>(q.c), *lA = const_cast<double*>(q.lA), *uA = const_cast<double*>(q.uA);
  double *d = const_cast<double*>(q.d), *lx = const_cast<double*>(q.lx), *ux = const_cast<double*>(q.ux);
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t < n) {
    c[t] = 2.0 * ipmz_u01(seed, TAG_C, t, 0) - 1.0;
    lx[t] = -1.0;
    ux[t] = 1.0;
  }
  if (t < m) {
    lA[t] = -1.0;
    uA[t] = 1.0;
  }
  if (t < p) {
    d[t] = (2.0 * ipmz_u01(seed, TAG_D, t, 0) - 1.0) * 0.1;
    if (q.eqss) lA[m + t] = uA[m + t] = d[t];  // the equality rows as l = u = d
  }
}

static inline int max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

static dim3 grid2(int64_t x, int B) { return dim3((unsigned)(x < 1 ? 1 : x), (unsigned)B); }

hipError_t qp_generate(const QPBatch& qb, uint64_t seed0, hipStream_t st) {
  const QPDev& h = qb.h;
  const int64_t gq = ((int64_t)h.n * h.n + NT - 1) / NT;
  hipLaunchKernelGGL(k_gen_Q, grid2(gq < 2048 ? gq : 2048, qb.B), dim3(NT), 0, st, qb.d, seed0);
  if (h.m_usr) {
    const int64_t g = ((int64_t)h.m_usr * h.n + NT - 1) / NT;
    hipLaunchKernelGGL(k_gen_rect, grid2(g < 1024 ? g : 1024, qb.B), dim3(NT), 0, st, qb.d, seed0, 0);
  }
  if (h.p_usr) {
    const int64_t g = ((int64_t)h.p_usr * h.n + NT - 1) / NT;
    hipLaunchKernelGGL(k_gen_rect, grid2(g < 1024 ? g : 1024, qb.B), dim3(NT), 0, st, qb.d, seed0, 1);
  }
  const int mx = max3(h.n, h.m_usr, h.p_usr);
  hipLaunchKernelGGL(k_gen_vec, grid2((mx + NT - 1) / NT, qb.B), dim3(NT), 0, st, qb.d, seed0);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// build_environment (EnvironmentBuilder.cpp:34-73): x = (l+u)/2, s = (l_A+u_A)/2,
// every other slack and dual 1.
__global__ void k_init_iterate(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.y];
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t < q.n) {
    q.v[X][t] = 0.5 * (q.lx[t] + q.ux[t]);
    if (q.vlo) q.v[LY][t] = 1.0;
    if (q.vup) q.v[LZ][t] = 1.0;
    if (q.vlo && !q.slacks) q.v[Y][t] = 1.0;
    if (q.vup && !q.slacks) q.v[Z][t] = 1.0;
  }
  if (t < q.m) {
    if (!q.naive) {
      q.v[S][t] = (q.eqss && t >= q.m_usr) ? 1.0 : 0.5 * (q.lA[t] + q.uA[t]);  // t = 1 (EnvironmentBuilder.cpp)
      q.v[LA][t] = 1.0;
    }
    if (q.alo) q.v[LG][t] = 1.0;
    if (q.aup) q.v[LH][t] = 1.0;
    if (q.alo && !q.slacks) q.v[G][t] = 1.0;
    if (q.aup && !q.slacks) q.v[H][t] = 1.0;
  }
  if (t < q.p) {
    q.v[LC][t] = 1.0;
    if (!q.eqnone && !q.eqpen) q.v[P][t] = 1.0;
  }
  if (t == 0) q.scal[SC_MU_NEW] = 1.0;  // the environment's mu (EnvironmentBuilder.cpp:49)
}

hipError_t qp_init_iterate(const QPBatch& qb, hipStream_t st) {
  hipLaunchKernelGGL(k_init_iterate, grid2((update_rows(qb.h) + NT - 1) / NT, qb.B), dim3(NT), 0, st, qb.d);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Dense matvecs (Evaluation.cpp:35-41 and the materialised transpose at
// :126-140).  MV selects Q x -> Qx, A x -> Ax, C x -> Cx; one wave per row,
// 16-byte loads; blockIdx.y = QP of the batch.
enum { MV_Q = 0, MV_A = 1, MV_C = 2 };
// one wave: sum_j r[j] x[j] (16-byte loads, two lane partials, DPP sum)
__device__ __forceinline__ double row_dot(const double* __restrict__ r, const double* __restrict__ x, int cols,
                                          int lane) {
  double s0 = 0.0, s1 = 0.0;
  int j = lane * 2;
  for (; j + 1 < cols; j += 128) {
    const double2 a = *reinterpret_cast<const double2*>(r + j);
    const double2 b = *reinterpret_cast<const double2*>(x + j);
    s0 += a.x * b.x;
    s1 += a.y * b.y;
  }
  if (j < cols) s0 += r[j] * x[j];
  return wave_sum(s0 + s1);
}
template <int MV>
__global__ __launch_bounds__(NT) void k_matvec_rows(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.y];
  const int rows = MV == MV_Q ? q.n : MV == MV_A ? q.m : q.p;
  const double* M = MV == MV_Q ? q.Q : MV == MV_A ? q.A : q.C;
  double* out = MV == MV_Q ? q.Qx : MV == MV_A ? q.Ax : q.Cx;
  const double* x = q.v[X];
  const int cols = q.n;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const double s = row_dot(M + (int64_t)row * q.ldn, x, cols, lane);
  if (lane == 0) out[row] = s;
}

// A^T lambda_A -> ATl, C^T lambda_C -> CTl: column blocks of NT x row chunks
// of 128, deterministic two-pass (chunk partials, then an ordered sum).
constexpr int TCHUNK = IPMZ_TCHUNK;  // 32: C2's A^T (512 x 2048) in 128 workgroups, not 32
template <int MV>
__global__ __launch_bounds__(NT) void k_matvec_t_part(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.z];
  const int rows = MV == MV_A ? q.m : q.p, cols = q.n;
  const double* M = MV == MV_A ? q.A : q.C;
  const int j = blockIdx.x * NT + threadIdx.x;
  const int i0 = blockIdx.y * TCHUNK;
  if (j >= cols) return;
  const int i1 = i0 + TCHUNK < rows ? i0 + TCHUNK : rows;
  double s = 0.0;
#pragma unroll 8
  for (int i = i0; i < i1; ++i) s += M[(int64_t)i * q.ldn + j] * (MV == MV_A ? a_dual(q, i) : q.v[LC][i]);
  q.tpart[(int64_t)blockIdx.y * cols + j] = s;
}
template <int MV>
__global__ void k_sum_chunks(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.y];
  const int rows = MV == MV_A ? q.m : q.p, cols = q.n;
  const int nchunk = (rows + TCHUNK - 1) / TCHUNK;
  double* out = MV == MV_A ? q.ATl : q.CTl;
  const int j = blockIdx.x * NT + threadIdx.x;
  if (j >= cols) return;
  double s = 0.0;
  for (int c = 0; c < nchunk; ++c) s += q.tpart[(int64_t)c * cols + j];
  out[j] = s;
}

template <int MV>
static void matvec_t(const QPBatch& qb, hipStream_t st) {
  const QPDev& h = qb.h;
  const int rows = MV == MV_A ? h.m : h.p;
  const int nchunk = (rows + TCHUNK - 1) / TCHUNK;
  hipLaunchKernelGGL((k_matvec_t_part<MV>), dim3((h.n + NT - 1) / NT, nchunk, qb.B), dim3(NT), 0, st, qb.d);
  hipLaunchKernelGGL((k_sum_chunks<MV>), grid2((h.n + NT - 1) / NT, qb.B), dim3(NT), 0, st, qb.d);
}

// number of complementarity rows (get_mu_'s divisor, Optimizer.cpp:250-268)
__device__ __forceinline__ int comp_count(const QPDev& q) { return (q.vlo + q.vup) * q.n + (q.alo + q.aup) * q.m; }

// ---------------------------------------------------------------------------
// Shorthand residuals r_v := -rhs_v at mu (SymbolicOptimization.cpp:480-492),
// plus per-block partials of ||rhs||^2, sum |complementarity|, and the two
// objective sums (Optimizer.cpp:128-130).
// one element t of the residual pass (t < n + m + p).  SC: the matvec
// results (Qx, A^T lambda_A, ...) were stored write-through by other
// workgroups of the same launch -- read them with agent-scope loads.
template <bool SC = false>
__device__ __forceinline__ void residual_elem(const QPDev& q, int t, double mu, double& res2, double& comp,
                                              double& fa, double& fb) {
  const int n = q.n, m = q.m, p = q.p;
  auto mv = [](const double* a) { return SC ? ld_sc1(a) : *a; };
  if (t < n) {
    const int i = t;
    // r_x := (c [+ lambda_z] + (Q*x) [+ (A^T*lambda_A)] [+ (C^T*lambda_C)] [- lambda_y])
    double s = q.c[i];
    if (q.vup) s = s + q.v[LZ][i];
    s = s + mv(&q.Qx[i]);
    if (m) s = s + mv(&q.ATl[i]);
    if (p) s = s + mv(&q.CTl[i]);
    const double rx = q.vlo ? s + (-q.v[LY][i]) : s;
    q.r[X][i] = rx;
    res2 += rx * rx;
    if (q.slacks) {  // (((X - L_x)*lambda_y) - (mu*e_x)), (((U_x - X)*lambda_z) - (mu*e_x))
      if (q.vlo) {
        const double r = ((q.v[X][i] + (-q.lx[i])) * q.v[LY][i]) + (-(mu * 1.0));
        q.r[LY][i] = r;
        res2 += r * r;
        comp += fabs(r);
      }
      if (q.vup) {
        const double r = ((q.ux[i] + (-q.v[X][i])) * q.v[LZ][i]) + (-(mu * 1.0));
        q.r[LZ][i] = r;
        res2 += r * r;
        comp += fabs(r);
      }
    } else {
      if (q.vlo) {
        const double rly = (q.lx[i] + q.v[Y][i]) + (-q.v[X][i]);     // (l_x + y - x)
        const double ry = q.v[Y][i] * q.v[LY][i] + (-(mu * 1.0));  // ((Y*lambda_y) - (mu*e_x))
        q.r[LY][i] = rly;
        q.r[Y][i] = ry;
        res2 += rly * rly + ry * ry;
        comp += fabs(ry);
      }
      if (q.vup) {
        const double rlz = (q.v[X][i] + q.v[Z][i]) + (-q.ux[i]);   // (x + z - u_x)
        const double rz = q.v[Z][i] * q.v[LZ][i] + (-(mu * 1.0));
        q.r[LZ][i] = rlz;
        q.r[Z][i] = rz;
        res2 += rlz * rlz + rz * rz;
        comp += fabs(rz);
      }
    }
    fa += (0.5 * q.v[X][i]) * mv(&q.Qx[i]);
    fb += q.c[i] * q.v[X][i];
  } else if (t < n + m && q.naive) {
    const int i = t - n;
    const double ax = mv(&q.Ax[i]);
    const double rlg = (q.lA[i] + q.v[G][i]) + (-ax);             // (l_A + g - (A*x))
    const double rlh = (q.v[H][i] + ax) + (-q.uA[i]);             // (h + (A*x) - u_A)
    const double rg = q.v[G][i] * q.v[LG][i] + (-(mu * 1.0));     // ((G*lambda_g) - (mu*e_A))
    const double rh = q.v[H][i] * q.v[LH][i] + (-(mu * 1.0));
    q.r[LG][i] = rlg;
    q.r[LH][i] = rlh;
    q.r[G][i] = rg;
    q.r[H][i] = rh;
    res2 += rlg * rlg + rlh * rlh + rg * rg + rh * rh;
    comp += fabs(rg) + fabs(rh);
  } else if (t < n + m) {
    const int i = t - n;
    const double rla = mv(&q.Ax[i]) + (-q.v[S][i]);  // ((A*x) - s)
    double rs;
    if (q.alo && q.aup) rs = -((q.v[LA][i] + q.v[LG][i]) + (-q.v[LH][i]));  // -(lambda_A + lambda_g - lambda_h)
    else if (q.alo) rs = -(q.v[LA][i] + q.v[LG][i]);                        // -(lambda_A + lambda_g)
    else rs = q.v[LH][i] + (-q.v[LA][i]);                                   // (lambda_h - lambda_A)
    q.r[LA][i] = rla;
    q.r[S][i] = rs;
    res2 += rla * rla + rs * rs;
    if (q.slacks) {  // (((S - L_A)*lambda_g) - (mu*e_A)), (((U_A - S)*lambda_h) - (mu*e_A))
      const double rlg = ((q.v[S][i] + (-q.lA[i])) * q.v[LG][i]) + (-(mu * 1.0));
      const double rlh = ((q.uA[i] + (-q.v[S][i])) * q.v[LH][i]) + (-(mu * 1.0));
      q.r[LG][i] = rlg;
      q.r[LH][i] = rlh;
      res2 += rlg * rlg + rlh * rlh;
      comp += fabs(rlg) + fabs(rlh);
    } else {
      if (q.alo) {
        const double rlg = (q.lA[i] + q.v[G][i]) + (-q.v[S][i]);  // (l_A + g - s)
        const double rg = q.v[G][i] * q.v[LG][i] + (-(mu * 1.0));
        q.r[LG][i] = rlg;
        q.r[G][i] = rg;
        res2 += rlg * rlg + rg * rg;
        comp += fabs(rg);
      }
      if (q.aup) {
        const double rlh = (q.v[H][i] + q.v[S][i]) + (-q.uA[i]);  // (h + s - u_A)
        const double rh = q.v[H][i] * q.v[LH][i] + (-(mu * 1.0));
        q.r[LH][i] = rlh;
        q.r[H][i] = rh;
        res2 += rlh * rlh + rh * rh;
        comp += fabs(rh);
      }
    }
  } else {
    const int i = t - n - m;
    if (q.eqnone) {  // ((C*x) - d)
      const double rlc = mv(&q.Cx[i]) + (-q.d[i]);
      q.r[LC][i] = rlc;
      res2 += rlc * rlc;
    } else if (q.eqpen) {  // -(d + (mu*lambda_C) - (C*x))
      const double rlc = -((q.d[i] + mu * q.v[LC][i]) + (-mv(&q.Cx[i])));
      q.r[LC][i] = rlc;
      res2 += rlc * rlc;
    } else {  // ((C*x) + (delta*p) - d), (p + (delta*lambda_C))
      const double rlc = (mv(&q.Cx[i]) + q.delta * q.v[P][i]) + (-q.d[i]);
      const double rp = q.v[P][i] + q.delta * q.v[LC][i];
      q.r[LC][i] = rlc;
      q.r[P][i] = rp;
      res2 += rlc * rlc + rp * rp;
    }
  }
}

__global__ __launch_bounds__(NT) void k_residuals(const QPDev* __restrict__ qs, double mu, int with_stats) {
  const QPDev& q = qs[blockIdx.y];
  __shared__ double sh[NT / 64];
  double res2 = 0.0, comp = 0.0, fa = 0.0, fb = 0.0;
  const int total = residual_rows(q);
  for (int t = blockIdx.x * NT + threadIdx.x; t < total; t += gridDim.x * NT)
    residual_elem(q, t, mu, res2, comp, fa, fb);
  if (!with_stats) return;
  double a = block_sum(res2, sh);
  if (threadIdx.x == 0) q.part[4 * blockIdx.x + 0] = a;
  a = block_sum(comp, sh);
  if (threadIdx.x == 0) q.part[4 * blockIdx.x + 1] = a;
  a = block_sum(fa, sh);
  if (threadIdx.x == 0) q.part[4 * blockIdx.x + 2] = a;
  a = block_sum(fb, sh);
  if (threadIdx.x == 0) q.part[4 * blockIdx.x + 3] = a;
}

// the evaluation's scalars from the three sums of the residual pass (one thread)
__device__ __forceinline__ void stats_store(const QPDev& q, double res2, double comp, double f) {
  const double res = sqrt(res2);
  const int cnt = comp_count(q);
  const double mu = cnt == 0 ? 0.0 : comp / (double)cnt;
  q.scal[SC_F] = f;
  q.scal[SC_RES] = res;
  q.scal[SC_MU] = mu;
  q.scal[SC_CONVERGED] = (res < 1e-8 && mu < 1e-8) ? 1.0 : 0.0;  // Optimizer.cpp:124,133
}

__global__ void k_stats_final(const QPDev* __restrict__ qs, int nblocks) {
  const QPDev& q = qs[blockIdx.y];
  __shared__ double sh[4][NT];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblocks; b += NT)
    for (int k = 0; k < 4; ++k) s[k] += q.part[4 * b + k];
  for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < NT; ++i)
      for (int k = 0; k < 4; ++k) t[k] += sh[k][i];
    stats_store(q, t[0], t[1], t[2] + t[3]);
  }
}

static int red_blocks(int total) {
  int b = (total + NT - 1) / NT;
  return b < 1 ? 1 : (b > RED_BLOCKS ? RED_BLOCKS : b);
}

// the products of the current iterate that the residual pass reads: Q x, A x, A^T (its dual), C x, C^T lambda_C
static void evaluate_products(const QPBatch& qb, hipStream_t st) {
  const QPDev& h = qb.h;
  hipLaunchKernelGGL((k_matvec_rows<MV_Q>), grid2((h.n + 3) / 4, qb.B), dim3(NT), 0, st, qb.d);
  if (h.m) {
    hipLaunchKernelGGL((k_matvec_rows<MV_A>), grid2((h.m + 3) / 4, qb.B), dim3(NT), 0, st, qb.d);
    matvec_t<MV_A>(qb, st);
  }
  if (h.p) {
    hipLaunchKernelGGL((k_matvec_rows<MV_C>), grid2((h.p + 3) / 4, qb.B), dim3(NT), 0, st, qb.d);
    matvec_t<MV_C>(qb, st);
  }
}

hipError_t qp_evaluate(const QPBatch& qb, hipStream_t st) {
  const QPDev& h = qb.h;
  evaluate_products(qb, st);
  const int nb = red_blocks(residual_rows(h));
  hipLaunchKernelGGL(k_residuals, grid2(nb, qb.B), dim3(NT), 0, st, qb.d, 0.0, 1);
  hipLaunchKernelGGL(k_stats_final, grid2(1, qb.B), dim3(NT), 0, st, qb.d, nb);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Augmented KKT (get_as_matrix_, Optimizer.cpp:387-391, 441-501): lower
// triangle only, row-major ld.  One workgroup per row, coalesced stores.
__device__ __forceinline__ double ds_inv(const QPDev& q, int i) {
  return ipmz_inv(ipmz_inv(q.v[G][i]) * q.v[LG][i] + ipmz_inv(q.v[H][i]) * q.v[LH][i]);
}
// Slacks: (((U_A - S)^{-1}*Lambda_h) + ((S - L_A)^{-1}*Lambda_g))^{-1}
__device__ __forceinline__ double ds_inv_sl(const QPDev& q, int i) {
  return ipmz_inv(ipmz_inv(q.uA[i] + (-q.v[S][i])) * q.v[LH][i] + ipmz_inv(q.v[S][i] + (-q.lA[i])) * q.v[LG][i]);
}
// (x, x) diagonal: Q_ii + the bound terms; (lambda_A, lambda_A) diagonal
__device__ __forceinline__ double kkt_xx(const QPDev& q, int i, double qii) {
  double h = qii;
  if (q.slacks) {  // (Q + ((U_x - X)^{-1}*Lambda_z) + ((X - L_x)^{-1}*Lambda_y))
    if (q.vup) h = h + ipmz_inv(q.ux[i] + (-q.v[X][i])) * q.v[LZ][i];
    if (q.vlo) h = h + ipmz_inv(q.v[X][i] + (-q.lx[i])) * q.v[LY][i];
  } else {  // (Q [+ (Y^{-1}*Lambda_y)] [+ (Z^{-1}*Lambda_z)])
    if (q.vlo) h = h + ipmz_inv(q.v[Y][i]) * q.v[LY][i];
    if (q.vup) h = h + ipmz_inv(q.v[Z][i]) * q.v[LZ][i];
  }
  return h;
}
__device__ __forceinline__ double kkt_aa(const QPDev& q, int i) {
  if (q.slacks) return -ds_inv_sl(q, i);
  if (q.alo && q.aup) return -ds_inv(q, i);            // -((G^{-1}*Lambda_g) + (H^{-1}*Lambda_h))^{-1}
  if (q.alo) return -(ipmz_inv(q.v[LG][i]) * q.v[G][i]);  // -(Lambda_g^{-1}*G)
  return -(ipmz_inv(q.v[LH][i]) * q.v[H][i]);             // -(Lambda_h^{-1}*H)
}

// diagonal element of KKT row i (< N):  x | lambda_A (NaiveSlacks: lambda_g, then lambda_h) | lambda_C
__device__ __forceinline__ double kkt_diag(const QPDev& q, int i) {
  const int n = q.n, m = q.m;
  if (i < n) return kkt_xx(q, i, q.Q[(int64_t)i * q.ldn + i]);
  if (q.naive && i < n + m) return -(ipmz_inv(q.v[LG][i - n]) * q.v[G][i - n]);          // -(L_g^{-1}*G)
  if (q.naive && i < n + q.mk) return -(ipmz_inv(q.v[LH][i - n - m]) * q.v[H][i - n - m]);  // -(L_h^{-1}*H)
  if (i < n + q.mk) return kkt_aa(q, i - n);
  return q.eqnone ? 0.0 : q.eqpen ? -q.scal[SC_MU_NEW] : -(q.delta * q.delta);
}

// row i of the lower triangle, columns split over nth threads (tid); the diagonal store stays where it was, at the
// end of each branch.  (Which of Q / A / C the row copies, its sign and its zeros are decided here and once more in
// k_fused_pre's copy units: a description shared by both changed k_fused_pre's register allocation, DESIGN.md
// "One definition per Newton-step formula and loop bound".)
__device__ __forceinline__ void assemble_row(const QPDev& q, int i, int tid, int nth, int c0, int c1) {
  // columns [c0, c1) of the row: the whole row with c0 = 0, c1 = N (qp_assemble_cols: the step's two parts)
  double* __restrict__ K = q.K;
  const int64_t ld = q.ldk;
  const int n = q.n, m = q.m, mk = q.mk;
  double* Kr = K + (int64_t)i * ld;
  const int je = i < c1 ? i : c1;              // end of the off-diagonal columns written
  const int jn = n < je ? n : je;              // ... of those copied from A / C
  const int jz = n > c0 ? n : c0;              // start of the zeros
  const bool dg = c0 <= i && i < c1;           // the diagonal is among them
  if (i < n) {
    const double* Qr = q.Q + (int64_t)i * q.ldn;
    for (int j = c0 + tid; j < je; j += nth) Kr[j] = Qr[j];
    if (!dg) return;
    if (tid == 0) Kr[i] = kkt_diag(q, i);
  } else if (i < n + mk && q.naive) {  // | -A | -(L_g^{-1}*G) | 0 |  and  | A | 0 | -(L_h^{-1}*H) |
    const bool hrow = i >= n + m;
    const int r = hrow ? i - n - m : i - n;
    const double* Ar = q.A + (int64_t)r * q.ldn;
    for (int j = c0 + tid; j < jn; j += nth) Kr[j] = hrow ? Ar[j] : -Ar[j];
    for (int j = jz + tid; j < je; j += nth) Kr[j] = 0.0;
    if (!dg) return;
    if (tid == 0) Kr[i] = kkt_diag(q, i);
  } else if (i < n + m) {
    const int r = i - n;
    const double* Ar = q.A + (int64_t)r * q.ldn;
    for (int j = c0 + tid; j < jn; j += nth) Kr[j] = Ar[j];
    for (int j = jz + tid; j < je; j += nth) Kr[j] = 0.0;
    if (!dg) return;
    if (tid == 0) Kr[i] = kkt_diag(q, i);
  } else {
    const int r = i - n - mk;
    const double* Cr = q.C + (int64_t)r * q.ldn;
    for (int j = c0 + tid; j < jn; j += nth) Kr[j] = Cr[j];
    for (int j = jz + tid; j < je; j += nth) Kr[j] = 0.0;
    if (!dg) return;
    if (tid == 0) Kr[i] = kkt_diag(q, i);
  }
}

// rows row0 .. of the lower triangle, columns [c0, c1)
__global__ __launch_bounds__(NT) void k_assemble(const QPDev* __restrict__ qs, int row0, int c0, int c1) {
  assemble_row(qs[blockIdx.y], row0 + blockIdx.x, threadIdx.x, NT, c0, c1);
}

hipError_t qp_assemble(const QPBatch& qb, hipStream_t st) {
  hipLaunchKernelGGL(k_assemble, grid2(qb.h.N, qb.B), dim3(NT), 0, st, qb.d, 0, 0, qb.h.N);
  return hipGetLastError();
}
// the same matrix in two launches: head = columns < c of every row (with the
// diagonal of rows < c), else columns >= c (rows >= c, with their diagonal)
hipError_t qp_assemble_cols(const QPBatch& qb, int c, bool head, hipStream_t st) {
  const int N = qb.h.N;
  if (c > N) c = N;
  if (head) {
    if (c > 0) hipLaunchKernelGGL(k_assemble, grid2(N, qb.B), dim3(NT), 0, st, qb.d, 0, 0, c);
  } else if (c < N) {
    hipLaunchKernelGGL(k_assemble, grid2(N - c, qb.B), dim3(NT), 0, st, qb.d, c, c, N);
  }
  return hipGetLastError();
}

// Where the residual vectors r_v, the augmented vector b and the directions of
// rhs_elem / backsub_elem / ratio_elem live -- the formulas themselves are
// written once, over an accessor IO: r(slot, i) reads r_v, b(t) is where the
// augmented rhs goes, x(t) reads the solved vector, d(slot, i) is a direction
// element, val_t the value type and zero() its zero.
//   DSel    the step's own slots of the QPDev: q.r, q.b and q.daff (which = 0)
//           or q.dir (1); val_t = double.
//   RowsIO  RP rows of a caller's block at once (newton_solve_multi below):
//           val_t = RowVec<RP>, one double per row, with the element-wise
//           operators the formulas use.  r_v lives in R and the directions in
//           D, both in Newton order -- the device slot layout itself, so
//           element i of slot s is at q.r[s] - q.r[0] + i -- and b in rows of
//           the workspace W.  What depends on the iterate alone (the ipmz_inv
//           reciprocals, ds_inv, the bounds) stays a double: it is evaluated
//           once per element for all RP rows.  D may be R (in place): an
//           element of a row is read and written by one thread only, so
//           neither pointer is __restrict__.  cnt <= RP rows are valid; the
//           others read the last valid row again and store nothing.
//   RowD    one row of D, for ratio_elem.
// The library is built with -ffp-contract=off: the same expression rounds the
// same way in every instantiation.
struct DSel {
  typedef double val_t;
  const QPDev& q;
  double* const* dd;
  __device__ __forceinline__ double r(int slot, int i) const { return q.r[slot][i]; }
  __device__ __forceinline__ double& b(int t) const { return q.b[t]; }
  __device__ __forceinline__ double x(int t) const { return q.b[t]; }
  __device__ __forceinline__ double& d(int slot, int i) const { return dd[slot][i]; }
  __device__ __forceinline__ double zero() const { return 0.0; }
};
__device__ __forceinline__ DSel dsel(const QPDev& q, int which) { return DSel{q, which ? q.dir : q.daff}; }

template <int RP>
struct RowVec {
  double v[RP];
};
#define IPMZ_ROWVEC_OP(OP)                                                                                \
  template <int RP>                                                                                       \
  __device__ __forceinline__ RowVec<RP> operator OP(const RowVec<RP>& a, const RowVec<RP>& b) {            \
    RowVec<RP> c;                                                                                         \
    _Pragma("unroll") for (int k = 0; k < RP; ++k) c.v[k] = a.v[k] OP b.v[k];                              \
    return c;                                                                                             \
  }                                                                                                       \
  template <int RP>                                                                                       \
  __device__ __forceinline__ RowVec<RP> operator OP(const RowVec<RP>& a, double b) {                       \
    RowVec<RP> c;                                                                                         \
    _Pragma("unroll") for (int k = 0; k < RP; ++k) c.v[k] = a.v[k] OP b;                                   \
    return c;                                                                                             \
  }                                                                                                       \
  template <int RP>                                                                                       \
  __device__ __forceinline__ RowVec<RP> operator OP(double a, const RowVec<RP>& b) {                       \
    RowVec<RP> c;                                                                                         \
    _Pragma("unroll") for (int k = 0; k < RP; ++k) c.v[k] = a OP b.v[k];                                   \
    return c;                                                                                             \
  }
IPMZ_ROWVEC_OP(+)
IPMZ_ROWVEC_OP(*)
#undef IPMZ_ROWVEC_OP
template <int RP>
__device__ __forceinline__ RowVec<RP> operator-(const RowVec<RP>& a) {
  RowVec<RP> c;
#pragma unroll
  for (int k = 0; k < RP; ++k) c.v[k] = -a.v[k];
  return c;
}
// element e of cnt rows, ld apart: assignment stores the valid rows
template <int RP>
struct RowRef {
  double* p;
  int64_t ld;
  int cnt;
  __device__ __forceinline__ void operator=(const RowVec<RP>& a) const {
#pragma unroll
    for (int k = 0; k < RP; ++k)
      if (k < cnt) p[k * ld] = a.v[k];
  }
};
template <int RP>
struct RowsIO {
  typedef RowVec<RP> val_t;
  const QPDev& q;
  const double* R;
  int64_t ldr;
  double* W;
  int64_t ldw;
  double* D;
  int64_t ldd;
  int cnt;
  __device__ __forceinline__ val_t load(const double* p, int64_t ld) const {
    val_t a;
#pragma unroll
    for (int k = 0; k < RP; ++k) a.v[k] = p[(k < cnt ? k : cnt - 1) * ld];
    return a;
  }
  __device__ __forceinline__ val_t r(int slot, int i) const { return load(R + (q.r[slot] - q.r[0]) + i, ldr); }
  __device__ __forceinline__ RowRef<RP> b(int t) const { return RowRef<RP>{W + t, ldw, cnt}; }
  __device__ __forceinline__ val_t x(int t) const { return load(W + t, ldw); }
  __device__ __forceinline__ RowRef<RP> d(int slot, int i) const {
    return RowRef<RP>{D + (q.r[slot] - q.r[0]) + i, ldd, cnt};
  }
  __device__ __forceinline__ val_t zero() const {
    val_t a;
#pragma unroll
    for (int k = 0; k < RP; ++k) a.v[k] = 0.0;
    return a;
  }
};
struct RowD {
  const QPDev& q;
  const double* D;
  __device__ __forceinline__ double d(int slot, int i) const { return D[(q.r[slot] - q.r[0]) + i]; }
};

// ---------------------------------------------------------------------------
// Augmented rhs (formulations.txt, augmented system rhs rows 0..2).
// element t (< N) of the augmented rhs
template <class IO>
__device__ __forceinline__ void rhs_elem(const QPDev& q, const IO& io, int t) {
  const int n = q.n, m = q.m;
  if (t < n) {
    const int i = t;
    const auto rx = io.r(X, i);
    if (q.slacks) {  // (((U_x - X)^{-1}*r_lz) - r_x - ((X - L_x)^{-1}*r_ly)), absent terms dropped
      auto b = q.vup ? ipmz_inv(q.ux[i] + (-q.v[X][i])) * io.r(LZ, i) + (-rx) : -rx;
      if (q.vlo) b = b + (-(ipmz_inv(q.v[X][i] + (-q.lx[i])) * io.r(LY, i)));
      io.b(i) = b;
      return;
    }
    const auto tz = q.vup ? ipmz_inv(q.v[Z][i]) * (io.r(Z, i) + (-(q.v[LZ][i] * io.r(LZ, i)))) : io.zero();
    const auto ty = q.vlo ? ipmz_inv(q.v[Y][i]) * (io.r(Y, i) + (-(q.v[LY][i] * io.r(LY, i)))) : io.zero();
    if (q.vlo && q.vup) io.b(i) = (tz + (-rx)) + (-ty);
    else if (q.vup) io.b(i) = tz + (-rx);  // ((Z^{-1}*(r_z - (L_z*r_lz))) - r_x)
    else if (q.vlo) io.b(i) = -(rx + ty);  // -(r_x + (Y^{-1}*(r_y - (L_y*r_ly))))
    else io.b(i) = -rx;
  } else if (t < n + q.mk && q.naive) {
    if (t < n + m) {  // ((L_g^{-1}*r_g) - r_lg)
      const int i = t - n;
      io.b(t) = ipmz_inv(q.v[LG][i]) * io.r(G, i) + (-io.r(LG, i));
    } else {  // ((L_h^{-1}*r_h) - r_lh)
      const int i = t - n - m;
      io.b(t) = ipmz_inv(q.v[LH][i]) * io.r(H, i) + (-io.r(LH, i));
    }
  } else if (t < n + m) {
    const int i = t - n;
    const auto rla = io.r(LA, i), rs = io.r(S, i);
    if (q.slacks) {
      const auto a = ipmz_inv(q.uA[i] + (-q.v[S][i])) * io.r(LH, i);
      const auto c = ipmz_inv(q.v[S][i] + (-q.lA[i])) * io.r(LG, i);
      io.b(t) = ds_inv_sl(q, i) * ((a + (-rs)) + (-c)) + (-rla);
    } else if (q.alo && q.aup) {
      const auto th = ipmz_inv(q.v[H][i]) * (io.r(H, i) + (-(q.v[LH][i] * io.r(LH, i))));
      const auto tg = ipmz_inv(q.v[G][i]) * (io.r(G, i) + (-(q.v[LG][i] * io.r(LG, i))));
      io.b(t) = ds_inv(q, i) * ((th + (-rs)) + (-tg)) + (-rla);
    } else if (q.alo) {  // -(r_lA + (L_g^{-1}*(r_g + (G*r_s))) - r_lg)
      io.b(t) = -((rla + ipmz_inv(q.v[LG][i]) * (io.r(G, i) + q.v[G][i] * rs)) + (-io.r(LG, i)));
    } else {  // ((L_h^{-1}*(r_h - (H*r_s))) - r_lA - r_lh)
      io.b(t) = ((ipmz_inv(q.v[LH][i]) * (io.r(H, i) + (-(q.v[H][i] * rs)))) + (-rla)) + (-io.r(LH, i));
    }
  } else if (t < q.N) {
    const int i = t - n - q.mk;
    io.b(t) = (q.eqnone || q.eqpen) ? -io.r(LC, i) : q.delta * io.r(P, i) + (-io.r(LC, i));
  }
}

__device__ __forceinline__ void rhs_elem(const QPDev& q, int t) { rhs_elem(q, dsel(q, 0), t); }

__global__ void k_rhs(const QPDev* __restrict__ qs) { rhs_elem(qs[blockIdx.y], blockIdx.x * NT + threadIdx.x); }

hipError_t qp_rhs(const QPBatch& qb, hipStream_t st) {
  hipLaunchKernelGGL(k_rhs, grid2((qb.h.N + NT - 1) / NT, qb.B), dim3(NT), 0, st, qb.d);
  return hipGetLastError();
}

// Back-substitution of the eliminated variables (delta_definitions,
// Optimizer.cpp:373-378) into the directions io.d.
//
// The reference's order for a slack / dual pair is dual first,
//   dl_g = -(G^-1 L_g)((ds + L_g^-1 r_g) - r_lg),  dg = -(L_g^-1 (r_g + G dl_g)),
// which the step keeps operation for operation (DSel).  It is accurate for the
// iterate's own residual (r_g = g l_g, so L_g^-1 r_g = g), not for a caller's:
// at a late iterate L_g^-1 r_g is 1e9 |r_g| where the dual is 1e-9, ds and r_lg
// are absorbed in the sum, and dg comes out of the cancellation r_g + G dl_g
// with an absolute error of 1e9 u -- row lambda_g of the Newton system, dg -
// ds + r_lg = 0, is then missed by 1e8 .. 1e9 u of its own terms
// (tests/test_gpu_graded_pivots.py measured 1.3e9 u).  For a caller's rows
// (every accessor but DSel) the pair is therefore taken row by row, slack first:
//   dg = ds - r_lg (row lambda_g, one rounding),  dl_g = -(G^-1 (r_g + L_g dg)) (row g),
// the same two equations in exact arithmetic, each met to a few u componentwise.
template <class IO>
struct backsub_rowwise {
  static constexpr bool value = !std::is_same<IO, DSel>::value;
};

// element t (< N): the solution b -> the Newton directions D
template <class IO>
__device__ __forceinline__ void backsub_elem(const QPDev& q, const IO& io, int t) {
  const int n = q.n, m = q.m;
  constexpr bool ROWWISE = backsub_rowwise<IO>::value;
  if (t < n) {
    const int i = t;
    const auto dx = io.x(i);
    io.d(X, i) = dx;
    if (q.slacks) {
      if (q.vlo)  // -((X - L_x)^{-1}*(r_ly + (L_y*dx)))
        io.d(LY, i) = -(ipmz_inv(q.v[X][i] + (-q.lx[i])) * (io.r(LY, i) + q.v[LY][i] * dx));
      if (q.vup)  // ((U_x - X)^{-1}*((L_z*dx) - r_lz))
        io.d(LZ, i) = ipmz_inv(q.ux[i] + (-q.v[X][i])) * (q.v[LZ][i] * dx + (-io.r(LZ, i)));
      return;
    }
    if constexpr (ROWWISE) {  // (both values before either store: D may be R)
      if (q.vlo) {
        const auto dy = dx + (-io.r(LY, i));
        const auto dly = -(ipmz_inv(q.v[Y][i]) * (io.r(Y, i) + q.v[LY][i] * dy));
        io.d(LY, i) = dly;
        io.d(Y, i) = dy;
      }
      if (q.vup) {
        const auto dz = -(dx + io.r(LZ, i));
        const auto dlz = -(ipmz_inv(q.v[Z][i]) * (io.r(Z, i) + q.v[LZ][i] * dz));
        io.d(LZ, i) = dlz;
        io.d(Z, i) = dz;
      }
      return;
    }
    if (q.vlo) {
      const auto dly = -((ipmz_inv(q.v[Y][i]) * q.v[LY][i]) *
                         ((dx + ipmz_inv(q.v[LY][i]) * io.r(Y, i)) + (-io.r(LY, i))));
      io.d(LY, i) = dly;
      io.d(Y, i) = -(ipmz_inv(q.v[LY][i]) * (io.r(Y, i) + q.v[Y][i] * dly));
    }
    if (q.vup) {
      const auto dlz = -((ipmz_inv(q.v[Z][i]) * q.v[LZ][i]) *
                         ((ipmz_inv(q.v[LZ][i]) * io.r(Z, i) + (-io.r(LZ, i))) + (-dx)));
      io.d(LZ, i) = dlz;
      io.d(Z, i) = -(ipmz_inv(q.v[LZ][i]) * (io.r(Z, i) + q.v[Z][i] * dlz));
    }
  } else if (t < n + q.mk && q.naive) {
    if (t < n + m) {  // -(L_g^{-1}*(r_g + (G*dl_g)))
      const int i = t - n;
      const auto dlg = io.x(t);
      io.d(LG, i) = dlg;
      io.d(G, i) = -(ipmz_inv(q.v[LG][i]) * (io.r(G, i) + q.v[G][i] * dlg));
    } else {
      const int i = t - n - m;
      const auto dlh = io.x(t);
      io.d(LH, i) = dlh;
      io.d(H, i) = -(ipmz_inv(q.v[LH][i]) * (io.r(H, i) + q.v[H][i] * dlh));
    }
  } else if (t < n + m) {
    const int i = t - n;
    const auto dla = io.x(t), rs = io.r(S, i);
    io.d(LA, i) = dla;
    if (q.slacks) {
      const auto a = ipmz_inv(q.uA[i] + (-q.v[S][i])) * io.r(LH, i);
      const auto c = ipmz_inv(q.v[S][i] + (-q.lA[i])) * io.r(LG, i);
      const auto ds = ds_inv_sl(q, i) * (((dla + a) + (-rs)) + (-c));
      io.d(S, i) = ds;
      io.d(LG, i) = -(ipmz_inv(q.v[S][i] + (-q.lA[i])) * (io.r(LG, i) + q.v[LG][i] * ds));
      io.d(LH, i) = ipmz_inv(q.uA[i] + (-q.v[S][i])) * (q.v[LH][i] * ds + (-io.r(LH, i)));
      return;
    }
    typename IO::val_t ds;
    if (q.alo && q.aup) {
      const auto th = ipmz_inv(q.v[H][i]) * (io.r(H, i) + (-(q.v[LH][i] * io.r(LH, i))));
      const auto tg = ipmz_inv(q.v[G][i]) * (io.r(G, i) + (-(q.v[LG][i] * io.r(LG, i))));
      ds = ds_inv(q, i) * (((dla + th) + (-rs)) + (-tg));
    } else if (q.alo) {  // (L_g^{-1}*G*(dla - r_s - (G^{-1}*(r_g - (L_g*r_lg)))))
      ds = (ipmz_inv(q.v[LG][i]) * q.v[G][i]) *
           ((dla + (-rs)) + (-(ipmz_inv(q.v[G][i]) * (io.r(G, i) + (-(q.v[LG][i] * io.r(LG, i)))))));
    } else {  // (L_h^{-1}*H*(dla + (H^{-1}*(r_h - (L_h*r_lh))) - r_s))
      ds = (ipmz_inv(q.v[LH][i]) * q.v[H][i]) *
           ((dla + ipmz_inv(q.v[H][i]) * (io.r(H, i) + (-(q.v[LH][i] * io.r(LH, i))))) + (-rs));
    }
    io.d(S, i) = ds;
    if constexpr (ROWWISE) {
      if (q.alo) {
        const auto dg = ds + (-io.r(LG, i));
        const auto dlg = -(ipmz_inv(q.v[G][i]) * (io.r(G, i) + q.v[LG][i] * dg));
        io.d(LG, i) = dlg;
        io.d(G, i) = dg;
      }
      if (q.aup) {
        const auto dh = -(ds + io.r(LH, i));
        const auto dlh = -(ipmz_inv(q.v[H][i]) * (io.r(H, i) + q.v[LH][i] * dh));
        io.d(LH, i) = dlh;
        io.d(H, i) = dh;
      }
      return;
    }
    if (q.alo) {
      const auto dlg =
          -((ipmz_inv(q.v[G][i]) * q.v[LG][i]) * ((ds + ipmz_inv(q.v[LG][i]) * io.r(G, i)) + (-io.r(LG, i))));
      io.d(LG, i) = dlg;
      io.d(G, i) = -(ipmz_inv(q.v[LG][i]) * (io.r(G, i) + q.v[G][i] * dlg));
    }
    if (q.aup) {
      const auto dlh =
          -((ipmz_inv(q.v[H][i]) * q.v[LH][i]) * ((ipmz_inv(q.v[LH][i]) * io.r(H, i) + (-io.r(LH, i))) + (-ds)));
      io.d(LH, i) = dlh;
      io.d(H, i) = -(ipmz_inv(q.v[LH][i]) * (io.r(H, i) + q.v[H][i] * dlh));
    }
  } else if (t < q.N) {
    const int i = t - n - q.mk;
    const auto dlc = io.x(t);
    io.d(LC, i) = dlc;
    if (!q.eqnone && !q.eqpen) io.d(P, i) = -(io.r(P, i) + q.delta * dlc);
  }
}

__global__ void k_backsub(const QPDev* __restrict__ qs, int which) {
  const QPDev& q = qs[blockIdx.y];
  backsub_elem(q, dsel(q, which), blockIdx.x * NT + threadIdx.x);
}

hipError_t qp_backsub(const QPBatch& qb, int which, hipStream_t st) {
  hipLaunchKernelGGL(k_backsub, grid2((qb.h.N + NT - 1) / NT, qb.B), dim3(NT), 0, st, qb.d, which);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// get_max_step_ (Optimizer.cpp:270-342): fraction-to-boundary over the
// non-negative Newton variables, plus -- when neither g nor h is a Newton
// variable (box-only SlackedSlacks, or Slacks) -- explicit bounds on x
// (l_x, u_x) and s (l_A, u_A), both always (the environment holds both).
// Element t (< n + m), folded into a.
template <class IO>
__device__ __forceinline__ void ratio_elem(const QPDev& q, const IO& io, int t, double& a) {
  const int n = q.n, m = q.m;
  const bool explicit_bounds = q.slacks || m == 0;
  auto nonneg = [&](int slot, int i) {
    const double d = io.d(slot, i);
    if (d < 0.0) a = fmin(a, -q.v[slot][i] / d);
  };
  auto bounded = [&](double v, double d, double lo, double up) {
    if (d < 0.0) a = fmin(a, (lo - v) / d);
    if (d > 0.0) a = fmin(a, (up - v) / d);
  };
  if (t < n) {
    const int i = t;
    if (q.vlo) nonneg(LY, i);
    if (q.vup) nonneg(LZ, i);
    if (!q.slacks) {
      if (q.vlo) nonneg(Y, i);
      if (q.vup) nonneg(Z, i);
    }
    if (explicit_bounds) bounded(q.v[X][i], io.d(X, i), q.lx[i], q.ux[i]);
  } else {
    const int i = t - n;
    if (q.alo) nonneg(LG, i);
    if (q.aup) nonneg(LH, i);
    if (!q.slacks) {
      if (q.alo) nonneg(G, i);
      if (q.aup) nonneg(H, i);
    }
    if (explicit_bounds) bounded(q.v[S][i], io.d(S, i), q.lA[i], q.uA[i]);
  }
}

__global__ __launch_bounds__(NT) void k_ratio_part(const QPDev* __restrict__ qs, int which) {
  const QPDev& q = qs[blockIdx.y];
  const DSel D = dsel(q, which);
  __shared__ double sh[NT / 64];
  double a = 1.0;
  for (int t = blockIdx.x * NT + threadIdx.x; t < comp_rows(q); t += gridDim.x * NT) ratio_elem(q, D, t, a);
  a = block_min(a, sh);
  if (threadIdx.x == 0) q.part[blockIdx.x] = a;
}
__global__ void k_min_final(const QPDev* __restrict__ qs, int nblocks, int out_index) {
  const QPDev& q = qs[blockIdx.y];
  __shared__ double sh[NT / 64];
  double a = 1.0;
  for (int b = threadIdx.x; b < nblocks; b += NT) a = fmin(a, q.part[b]);
  a = block_min(a, sh);
  if (threadIdx.x == 0) q.scal[out_index] = a;
}

hipError_t qp_ratio(const QPBatch& qb, int which, int out_index, hipStream_t st) {
  const int nb = red_blocks(comp_rows(qb.h));
  hipLaunchKernelGGL(k_ratio_part, grid2(nb, qb.B), dim3(NT), 0, st, qb.d, which);
  hipLaunchKernelGGL(k_min_final, grid2(1, qb.B), dim3(NT), 0, st, qb.d, nb, out_index);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// compute_search_direction_ (Optimizer.cpp:344-380) for a block of residual
// vectors (ipmz_*_newton_solve_multi): row r of QP z of R holds r_v in Newton
// order; k_rhs_multi writes its augmented rhs to row r of the workspace W, the
// blocked solves overwrite W with K^{-1} W, k_backsub_multi writes the full
// direction to row r of D and k_ratio_multi get_max_step_ of (iterate, row).
// Grid (N / NT, row groups, QP): a thread owns KKT element t of one QP and
// the RP rows of its group at once (RowsIO) -- a row's loads are coalesced
// across t, and what depends on the iterate alone is evaluated once for the
// group.  Stream order only, no atomics; a row's result depends on no other
// row (the rows of a group share only those iterate factors).
template <int RP>
__global__ __launch_bounds__(NT) void k_rhs_multi(const QPDev* __restrict__ qs, const double* __restrict__ R,
                                                  int64_t ldr, int64_t sR, double* __restrict__ W, int64_t ldw,
                                                  int64_t sW, int row0, int nrhs) {
  const QPDev& q = qs[blockIdx.z];
  const int t = blockIdx.x * NT + threadIdx.x;
  const int r0 = row0 + blockIdx.y * RP;
  if (t >= q.N || r0 >= nrhs) return;
  R += blockIdx.z * sR + (int64_t)r0 * ldr;
  W += blockIdx.z * sW + (int64_t)r0 * ldw;
  rhs_elem(q, RowsIO<RP>{q, R, ldr, W, ldw, nullptr, 0, nrhs - r0 < RP ? nrhs - r0 : RP}, t);
}
// (R and D without __restrict__: D may be R)
template <int RP>
__global__ __launch_bounds__(NT) void k_backsub_multi(const QPDev* __restrict__ qs, const double* R, int64_t ldr,
                                                      int64_t sR, const double* __restrict__ W, int64_t ldw,
                                                      int64_t sW, double* D, int64_t ldd, int64_t sD, int row0,
                                                      int nrhs) {
  const QPDev& q = qs[blockIdx.z];
  const int t = blockIdx.x * NT + threadIdx.x;
  const int r0 = row0 + blockIdx.y * RP;
  if (t >= q.N || r0 >= nrhs) return;
  R += blockIdx.z * sR + (int64_t)r0 * ldr;
  W += blockIdx.z * sW + (int64_t)r0 * ldw;
  D += blockIdx.z * sD + (int64_t)r0 * ldd;
  backsub_elem(q, RowsIO<RP>{q, R, ldr, const_cast<double*>(W), ldw, D, ldd, nrhs - r0 < RP ? nrhs - r0 : RP}, t);
}
// one workgroup of NTH threads per (row, QP): ratio_elem over t < n + m in a
// fixed order (and fmin over finite values does not depend on it)
template <int NTH>
__global__ __launch_bounds__(NTH) void k_ratio_multi(const QPDev* __restrict__ qs, const double* __restrict__ D,
                                                     int64_t ldd, int64_t sD, double* __restrict__ alpha, int row0,
                                                     int nrhs) {
  const QPDev& q = qs[blockIdx.y];
  const int r = row0 + blockIdx.x;
  const RowD io{q, D + blockIdx.y * sD + (int64_t)r * ldd};
  __shared__ double sh[NTH / 64];
  double a = 1.0;
  for (int t = threadIdx.x; t < comp_rows(q); t += NTH) ratio_elem(q, io, t, a);
  a = block_allmin<NTH>(a, sh);
  if (threadIdx.x == 0) alpha[(int64_t)blockIdx.y * nrhs + r] = a;
}

// rows per group of the two element-wise kernels (tools/newton_multi_bench.py,
// DESIGN.md "Newton directions for a block of residuals"); the debug bits
// select 1, 2 or 8 for the A/B
static int newton_multi_rpg() {
  const int dbg = debug_inject_mask();
  const bool r1 = dbg & IPMZ_DEBUG_NEWTON_RPG1, r8 = dbg & IPMZ_DEBUG_NEWTON_RPG8;
  return r1 && r8 ? 2 : r1 ? 1 : r8 ? 8 : IPMZ_NEWTON_MULTI_RPG;
}
// f(rows per group as a constant, first row, grid): grid y <= 65535, further launches for more groups
template <typename F>
static void newton_multi_launches(const QPBatch& qb, int nrhs, F&& f) {
  const int rpg = newton_multi_rpg();
  const int64_t groups = ((int64_t)nrhs + rpg - 1) / rpg;
  for (int64_t g0 = 0; g0 < groups; g0 += 65535) {
    const dim3 grid((qb.h.N + NT - 1) / NT, (unsigned)(groups - g0 < 65535 ? groups - g0 : 65535), qb.B);
    const int row0 = (int)(g0 * rpg);
    if (rpg == 1) f(std::integral_constant<int, 1>{}, row0, grid);
    else if (rpg == 2) f(std::integral_constant<int, 2>{}, row0, grid);
    else if (rpg == 8) f(std::integral_constant<int, 8>{}, row0, grid);
    else f(std::integral_constant<int, IPMZ_NEWTON_MULTI_RPG>{}, row0, grid);
  }
}

hipError_t qp_rhs_multi(const QPBatch& qb, const double* R, int64_t ldr, int64_t sR, double* W, int64_t ldw, int64_t sW,
                        int nrhs, hipStream_t st) {
  newton_multi_launches(qb, nrhs, [&](auto rp, int row0, dim3 grid) {
    hipLaunchKernelGGL((k_rhs_multi<decltype(rp)::value>), grid, dim3(NT), 0, st, qb.d, R, ldr, sR, W, ldw, sW, row0,
                       nrhs);
  });
  return hipGetLastError();
}
hipError_t qp_backsub_multi(const QPBatch& qb, const double* R, int64_t ldr, int64_t sR, const double* W, int64_t ldw,
                            int64_t sW, double* D, int64_t ldd, int64_t sD, int nrhs, hipStream_t st) {
  newton_multi_launches(qb, nrhs, [&](auto rp, int row0, dim3 grid) {
    hipLaunchKernelGGL((k_backsub_multi<decltype(rp)::value>), grid, dim3(NT), 0, st, qb.d, R, ldr, sR, W, ldw, sW, D,
                       ldd, sD, row0, nrhs);
  });
  return hipGetLastError();
}
// ---------------------------------------------------------------------------
// The transposed map (ipmz_*_newton_adjoint_multi).  Per row the forward call
// is b = G_r r (rhs_elem), x = K^{-1} b, d = E x + F r (backsub_elem), so
// Dir = M r with M = F + E K^{-1} G_r; K is symmetric and G_r, E, F couple only
// the slots element t owns at its own index, so
//   M^T g = F^T g + G_r^T K^{-1} (E^T g)
// is two element-wise kernels on the same grid around the same solves:
//   k_adj_reduce_multi  row of G -> c = E^T g in the row of W
//   k_adj_expand_multi  the solved row y of W and the row of G ->
//                       out(slot, i) = sum_dslot F[dslot][slot] g(dslot, i) + G_r[slot] y(t)
// The coefficients are not restated: rhs_elem / backsub_elem are linear and
// homogeneous in (r, x), so two more accessors read them off the formulas.
//   AdjReduceIO  val_t = double, r = 0, x(t) = 1: what backsub_elem assigns to
//                d(slot, i) is E[slot]; the assignment adds E[slot] g(slot, i)
//                to c for the RP rows.
//   AdjExpandIO  val_t = RowVec<ADJ_LANES>, one lane per residual slot of the
//                element (adj_lane: at most 6 meet in one), r(slot, i) the unit
//                vector of the slot's lane, x = 0: what rhs_elem assigns to b(t)
//                is G_r by lane, what backsub_elem assigns to d(slot, i) is row
//                `slot` of F by lane; that assignment adds F[slot][lane]
//                g(slot, i) to the lane's accumulator for the RP rows.
// Both evaluate the coefficients once per element for the RP rows of the group.
// The slots an element has are the ones the formulas touched (present); only
// those are written.  A thread loads every g element it owns (in the d
// assignments) before it stores any out element, so Out may be the block of
// cotangents itself (Cot below: the caller's G, which is a slot's name here).
#define ADJ_LANES 6
__device__ __forceinline__ constexpr int adj_lane(int slot) {
  // t < n: x y z lambda_y lambda_z | inequality rows: s g h lambda_A lambda_g lambda_h | equality rows: p lambda_C
  return slot == X || slot == S || slot == P ? 0
         : slot == Y || slot == G || slot == LC ? 1
         : slot == Z || slot == H ? 2
         : slot == LY || slot == LA ? 3
         : slot == LZ || slot == LG ? 4
                                    : 5;
}
// element e of cnt rows of the cotangent block, ld apart (rows past cnt: the last valid one again)
template <int RP>
__device__ __forceinline__ RowVec<RP> adj_load(const double* p, int64_t ld, int cnt) {
  RowVec<RP> a;
#pragma unroll
  for (int k = 0; k < RP; ++k) a.v[k] = p[(k < cnt ? k : cnt - 1) * ld];
  return a;
}

template <int RP>
struct AdjReduceRef {
  const double* g;
  int64_t ldg;
  int cnt;
  RowVec<RP>& c;
  __device__ __forceinline__ void operator=(double coef) const { c = c + coef * adj_load<RP>(g, ldg, cnt); }
};
template <int RP>
struct AdjReduceIO {
  typedef double val_t;
  const QPDev& q;
  const double* Cot;
  int64_t ldg;
  int cnt;
  RowVec<RP>& c;
  __device__ __forceinline__ double r(int, int) const { return 0.0; }
  __device__ __forceinline__ double x(int) const { return 1.0; }
  __device__ __forceinline__ AdjReduceRef<RP> d(int slot, int i) const {
    return AdjReduceRef<RP>{Cot + (q.r[slot] - q.r[0]) + i, ldg, cnt, c};
  }
  __device__ __forceinline__ double zero() const { return 0.0; }
};

template <int RP>
struct AdjExpandState {
  RowVec<RP> acc[ADJ_LANES];  // by lane: sum over d slots of F[dslot][lane] g(dslot, i)
  RowVec<ADJ_LANES> gr;       // G_r by lane
  unsigned present;           // bit per slot the element has
  int i;                      // ... all at this index
};
struct AdjCaptureRef {
  RowVec<ADJ_LANES>& gr;
  __device__ __forceinline__ void operator=(const RowVec<ADJ_LANES>& a) const { gr = a; }
};
template <int RP>
struct AdjExpandRef {
  const double* g;
  int64_t ldg;
  int cnt;
  AdjExpandState<RP>& s;
  __device__ __forceinline__ void operator=(const RowVec<ADJ_LANES>& coef) const {
    const RowVec<RP> gv = adj_load<RP>(g, ldg, cnt);
#pragma unroll
    for (int l = 0; l < ADJ_LANES; ++l) s.acc[l] = s.acc[l] + coef.v[l] * gv;
  }
};
template <int RP>
struct AdjExpandIO {
  typedef RowVec<ADJ_LANES> val_t;
  const QPDev& q;
  const double* Cot;
  int64_t ldg;
  int cnt;
  AdjExpandState<RP>& s;
  __device__ __forceinline__ void own(int slot, int i) const {
    s.present |= 1u << slot;
    s.i = i;
  }
  __device__ __forceinline__ val_t r(int slot, int i) const {
    own(slot, i);
    val_t a;
#pragma unroll
    for (int l = 0; l < ADJ_LANES; ++l) a.v[l] = l == adj_lane(slot) ? 1.0 : 0.0;
    return a;
  }
  __device__ __forceinline__ AdjCaptureRef b(int) const { return AdjCaptureRef{s.gr}; }
  __device__ __forceinline__ val_t x(int) const { return zero(); }
  __device__ __forceinline__ AdjExpandRef<RP> d(int slot, int i) const {
    own(slot, i);
    return AdjExpandRef<RP>{Cot + (q.r[slot] - q.r[0]) + i, ldg, cnt, s};
  }
  __device__ __forceinline__ val_t zero() const {
    val_t a;
#pragma unroll
    for (int l = 0; l < ADJ_LANES; ++l) a.v[l] = 0.0;
    return a;
  }
};

template <int RP>
__global__ __launch_bounds__(NT) void k_adj_reduce_multi(const QPDev* __restrict__ qs, const double* __restrict__ Cot,
                                                         int64_t ldg, int64_t sG, double* __restrict__ W, int64_t ldw,
                                                         int64_t sW, int row0, int nrhs) {
  const QPDev& q = qs[blockIdx.z];
  const int t = blockIdx.x * NT + threadIdx.x;
  const int r0 = row0 + blockIdx.y * RP;
  if (t >= q.N || r0 >= nrhs) return;
  const int cnt = nrhs - r0 < RP ? nrhs - r0 : RP;
  Cot += blockIdx.z * sG + (int64_t)r0 * ldg;
  W += blockIdx.z * sW + (int64_t)r0 * ldw;
  RowVec<RP> c;
#pragma unroll
  for (int k = 0; k < RP; ++k) c.v[k] = 0.0;
  backsub_elem(q, AdjReduceIO<RP>{q, Cot, ldg, cnt, c}, t);
  RowRef<RP>{W + t, ldw, cnt} = c;
}
// (Cot, the caller's G, and Out without __restrict__: Out may be Cot)
template <int RP>
__global__ __launch_bounds__(NT) void k_adj_expand_multi(const QPDev* __restrict__ qs, const double* Cot, int64_t ldg,
                                                         int64_t sG, const double* __restrict__ W, int64_t ldw,
                                                         int64_t sW, double* Out, int64_t ldo, int64_t sO, int row0,
                                                         int nrhs) {
  const QPDev& q = qs[blockIdx.z];
  const int t = blockIdx.x * NT + threadIdx.x;
  const int r0 = row0 + blockIdx.y * RP;
  if (t >= q.N || r0 >= nrhs) return;
  const int cnt = nrhs - r0 < RP ? nrhs - r0 : RP;
  Cot += blockIdx.z * sG + (int64_t)r0 * ldg;
  W += blockIdx.z * sW + (int64_t)r0 * ldw;
  Out += blockIdx.z * sO + (int64_t)r0 * ldo;
  AdjExpandState<RP> s;
  s.present = 0u;
  s.i = 0;
#pragma unroll
  for (int l = 0; l < ADJ_LANES; ++l) {
    s.gr.v[l] = 0.0;
#pragma unroll
    for (int k = 0; k < RP; ++k) s.acc[l].v[k] = 0.0;
  }
  const AdjExpandIO<RP> io{q, Cot, ldg, cnt, s};
  rhs_elem(q, io, t);
  backsub_elem(q, io, t);  // the last load of Cot
  const RowVec<RP> y = adj_load<RP>(W + t, ldw, cnt);
#pragma unroll
  for (int slot = 0; slot < NSLOT; ++slot)
    if (s.present >> slot & 1u)
      RowRef<RP>{Out + (q.r[slot] - q.r[0]) + s.i, ldo, cnt} = s.acc[adj_lane(slot)] + s.gr.v[adj_lane(slot)] * y;
}

hipError_t qp_adj_reduce_multi(const QPBatch& qb, const double* Cot, int64_t ldg, int64_t sG, double* W, int64_t ldw,
                               int64_t sW, int nrhs, hipStream_t st) {
  newton_multi_launches(qb, nrhs, [&](auto rp, int row0, dim3 grid) {
    hipLaunchKernelGGL((k_adj_reduce_multi<decltype(rp)::value>), grid, dim3(NT), 0, st, qb.d, Cot, ldg, sG, W, ldw, sW,
                       row0, nrhs);
  });
  return hipGetLastError();
}
hipError_t qp_adj_expand_multi(const QPBatch& qb, const double* Cot, int64_t ldg, int64_t sG, const double* W,
                               int64_t ldw, int64_t sW, double* Out, int64_t ldo, int64_t sO, int nrhs, hipStream_t st) {
  newton_multi_launches(qb, nrhs, [&](auto rp, int row0, dim3 grid) {
    hipLaunchKernelGGL((k_adj_expand_multi<decltype(rp)::value>), grid, dim3(NT), 0, st, qb.d, Cot, ldg, sG, W, ldw, sW,
                       Out, ldo, sO, row0, nrhs);
  });
  return hipGetLastError();
}

hipError_t qp_ratio_multi(const QPBatch& qb, const double* D, int64_t ldd, int64_t sD, double* alpha, int nrhs,
                          hipStream_t st) {
  if (nrhs <= 0) return hipSuccess;
  // 1024 threads where a row keeps them busy (a single large QP: one workgroup walks n + m elements)
  if (comp_rows(qb.h) > 2048)
    hipLaunchKernelGGL(k_ratio_multi<1024>, dim3(nrhs, qb.B), dim3(1024), 0, st, qb.d, D, ldd, sD, alpha, 0, nrhs);
  else
    hipLaunchKernelGGL(k_ratio_multi<NT>, dim3(nrhs, qb.B), dim3(NT), 0, st, qb.d, D, ldd, sD, alpha, 0, nrhs);
  return hipGetLastError();
}

// mu at the affine trial point v + alpha_aff * daff (Optimizer.cpp:167-180):
// |complementarity| of every row that carries e and mu, at the trial point.
__device__ __forceinline__ void mu_aff_elem(const QPDev& q, int t, double al, double& s) {
  const int n = q.n;
  auto tv = [&](int slot, int i) { return q.v[slot][i] + al * q.daff[slot][i]; };
  auto term = [&](double a, double b) { return fabs(-(a * b + (-(0.0 * 1.0)))); };
  if (t < n) {
    const int i = t;
    if (q.slacks) {
      if (q.vlo) s += term(tv(X, i) + (-q.lx[i]), tv(LY, i));  // ((X - L_x)*lambda_y)
      if (q.vup) s += term(q.ux[i] + (-tv(X, i)), tv(LZ, i));  // ((U_x - X)*lambda_z)
    } else {
      if (q.vlo) s += term(tv(Y, i), tv(LY, i));
      if (q.vup) s += term(tv(Z, i), tv(LZ, i));
    }
  } else {
    const int i = t - n;
    if (q.slacks) {
      s += term(tv(S, i) + (-q.lA[i]), tv(LG, i));  // ((S - L_A)*lambda_g)
      s += term(q.uA[i] + (-tv(S, i)), tv(LH, i));  // ((U_A - S)*lambda_h)
    } else {
      if (q.alo) s += term(tv(G, i), tv(LG, i));
      if (q.aup) s += term(tv(H, i), tv(LH, i));
    }
  }
}
__global__ __launch_bounds__(NT) void k_mu_aff_part(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.y];
  __shared__ double sh[NT / 64];
  const double al = q.scal[SC_ALPHA_AFF];
  double s = 0.0;
  for (int t = blockIdx.x * NT + threadIdx.x; t < comp_rows(q); t += gridDim.x * NT) mu_aff_elem(q, t, al, s);
  s = block_sum(s, sh);
  if (threadIdx.x == 0) q.part[blockIdx.x] = s;
}
// mu_aff, sigma = (mu_aff / mu)^3, mu_new = mu sigma (Optimizer.cpp:167-182)
// from s = the sum of mu_aff_elem; pure, so every thread of a workgroup may
// evaluate it before one of them stores
struct Centering {
  double mu_aff, sigma, mu_new;
};
__device__ __forceinline__ Centering centering(const QPDev& q, double s) {
  const int cnt = comp_count(q);
  const double mu_aff = cnt == 0 ? 0.0 : s / (double)cnt;
  const double mu = q.scal[SC_MU];
  const double sigma = mu > 0.0 ? pow(mu_aff / mu, 3.0) : 0.0;
  return Centering{mu_aff, sigma, mu * sigma};
}
__device__ __forceinline__ void centering_store(const QPDev& q, const Centering& c) {
  q.scal[SC_MU_AFF] = c.mu_aff;
  q.scal[SC_SIGMA] = c.sigma;
  q.scal[SC_MU_NEW] = c.mu_new;
}
__global__ void k_mu_aff_final(const QPDev* __restrict__ qs, int nblocks) {
  const QPDev& q = qs[blockIdx.y];
  __shared__ double sh[NT / 64];
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += NT) s += q.part[b];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) centering_store(q, centering(q, s));
}

hipError_t qp_mu_aff(const QPBatch& qb, hipStream_t st) {
  const int nb = red_blocks(comp_rows(qb.h));
  hipLaunchKernelGGL(k_mu_aff_part, grid2(nb, qb.B), dim3(NT), 0, st, qb.d);
  hipLaunchKernelGGL(k_mu_aff_final, grid2(1, qb.B), dim3(NT), 0, st, qb.d, nb);
  return hipGetLastError();
}

// Corrector (Optimizer.cpp:183-209): every complementarity row at mu_new plus
// the same row with mu -> 0 and every VARIABLE replaced by its affine
// direction: SlackedSlacks r_y = (Y lambda_y - mu_new e) + (dY_aff
// dlambda_y_aff - 0 e); Slacks r_lambda_y = ((X - L_x) lambda_y - mu_new e) +
// ((dX_aff - L_x) dlambda_y_aff - 0 e) -- the bound constant leaks into the
// correction (the reference's Slacks defect, SURVEY.md App. C.1, reproduced).
__device__ __forceinline__ void corrector_elem(const QPDev& q, int t, double mu) {
  const int n = q.n, m = q.m;
  const double* const* v = q.v;
  const double* const* da = q.daff;
  auto ss = [&](int c, int d, int i) {  // SlackedSlacks pair (c = slack, d = its dual)
    q.r[c][i] = (v[c][i] * v[d][i] + (-(mu * 1.0))) + (da[c][i] * da[d][i] + (-(0.0 * 1.0)));
  };
  if (t < n) {
    const int i = t;
    if (q.slacks) {
      if (q.vlo)
        q.r[LY][i] = (((v[X][i] + (-q.lx[i])) * v[LY][i]) + (-(mu * 1.0))) +
                     ((da[X][i] + (-q.lx[i])) * da[LY][i] + (-(0.0 * 1.0)));
      if (q.vup)
        q.r[LZ][i] = (((q.ux[i] + (-v[X][i])) * v[LZ][i]) + (-(mu * 1.0))) +
                     ((q.ux[i] + (-da[X][i])) * da[LZ][i] + (-(0.0 * 1.0)));
    } else {
      if (q.vlo) ss(Y, LY, i);
      if (q.vup) ss(Z, LZ, i);
    }
  } else if (t < n + m) {
    const int i = t - n;
    if (q.slacks) {
      q.r[LG][i] = (((v[S][i] + (-q.lA[i])) * v[LG][i]) + (-(mu * 1.0))) +
                   ((da[S][i] + (-q.lA[i])) * da[LG][i] + (-(0.0 * 1.0)));
      q.r[LH][i] = (((q.uA[i] + (-v[S][i])) * v[LH][i]) + (-(mu * 1.0))) +
                   ((q.uA[i] + (-da[S][i])) * da[LH][i] + (-(0.0 * 1.0)));
    } else {
      if (q.alo) ss(G, LG, i);
      if (q.aup) ss(H, LH, i);
    }
  } else {
    // PenaltyFunction: r_lambda_C carries mu (no e, so no affine correction)
    const int i = t - n - m;
    if (q.eqpen && i < q.p) q.r[LC][i] = -((q.d[i] + mu * v[LC][i]) + (-q.Cx[i]));
  }
}
__global__ void k_corrector(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.y];
  corrector_elem(q, blockIdx.x * NT + threadIdx.x, q.scal[SC_MU_NEW]);
}

hipError_t qp_corrector_residuals(const QPBatch& qb, hipStream_t st) {
  hipLaunchKernelGGL(k_corrector, grid2((corrector_rows(qb.h) + NT - 1) / NT, qb.B), dim3(NT), 0, st, qb.d);
  return hipGetLastError();
}

// update_variables_(0.995 * alpha, ...) (Optimizer.cpp:216-231)
// freeze != 0: a converged QP of a batch keeps its iterate (the reference
// stops iterating it, Optimizer.cpp:133-135).
__device__ __forceinline__ void update_elem(const QPDev& q, int t, double s) {
  const int n = q.n, m = q.m, p = q.p;
  auto up = [&](int slot, int i) { q.v[slot][i] = q.v[slot][i] + s * q.dir[slot][i]; };
  if (t < n) {
    up(X, t);
    if (q.vlo) up(LY, t);
    if (q.vup) up(LZ, t);
    if (q.vlo && !q.slacks) up(Y, t);
    if (q.vup && !q.slacks) up(Z, t);
  }
  if (t < m) {
    if (!q.naive) {
      up(LA, t);
      up(S, t);
    }
    if (q.alo) up(LG, t);
    if (q.aup) up(LH, t);
    if (q.alo && !q.slacks) up(G, t);
    if (q.aup && !q.slacks) up(H, t);
  }
  if (t < p) {
    up(LC, t);
    if (!q.eqnone && !q.eqpen) up(P, t);
  }
}
// The same rule for the centering loop (qp_center_update below), when frozen is given: QP z sits out where
// frozen[z] != 0 -- its workgroups return here, at the top of the launch -- its step length is alpha[z] (before the
// 0.995), and count[z] counts the updates it received.
struct UpdateGate {
  const int* frozen = nullptr;
  const double* alpha = nullptr;
  int* count = nullptr;
};
__global__ void k_update(const QPDev* __restrict__ qs, int freeze, UpdateGate g) {
  const QPDev& q = qs[blockIdx.y];
  if (g.frozen ? g.frozen[blockIdx.y] != 0 : (freeze && q.scal[SC_CONVERGED] != 0.0)) return;
  update_elem(q, blockIdx.x * NT + threadIdx.x, 0.995 * (g.frozen ? g.alpha[blockIdx.y] : q.scal[SC_ALPHA]));
  if (g.frozen && blockIdx.x == 0 && threadIdx.x == 0) g.count[blockIdx.y] += 1;
}
static hipError_t launch_update(const QPBatch& qb, int freeze, const UpdateGate& g, hipStream_t st) {
  hipLaunchKernelGGL(k_update, grid2((update_rows(qb.h) + NT - 1) / NT, qb.B), dim3(NT), 0, st, qb.d, freeze, g);
  return hipGetLastError();
}

hipError_t qp_update(const QPBatch& qb, int freeze, hipStream_t st) { return launch_update(qb, freeze, UpdateGate{}, st); }

// Benchmark restart: a converged iterate is reset (on device, no host sync)
// to the saved initial state, so every timed step is a real Newton step.
// Element t of the restart copy (the callers stride over state_len elements;
// p <= state_len).  PenaltyFunction: C x goes back too -- its corrector row is
// rebuilt from q.Cx (corrector_elem), which otherwise still holds the
// converged iterate's; no other formulation reads a product of the evaluation
// between a restart and the next evaluation.
__device__ __forceinline__ void restart_elem(const QPDev& q, int64_t t) {
  if (t < q.state_len) {
    q.v[0][t] = q.v0[t];
    q.r[0][t] = q.r0[t];
  }
  if (q.eqpen && t < q.p) q.Cx[t] = q.Cx0[t];
}
__global__ void k_restart_copy(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.y];
  if (q.scal[SC_CONVERGED] == 0.0) return;
  for (int64_t t = blockIdx.x * (int64_t)NT + threadIdx.x; t < q.state_len; t += (int64_t)gridDim.x * NT)
    restart_elem(q, t);
}
// the restart of the scalar block (one thread): the saved scalars, the restart count kept and raised
__device__ __forceinline__ void restart_scalars(const QPDev& q) {
  const double restarts = q.scal[SC_RESTARTS];
  for (int k = 0; k < SC_RESTARTS; ++k) q.scal[k] = q.scal0[k];
  q.scal[SC_RESTARTS] = restarts + 1.0;
}
__global__ void k_restart_scal(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.y];
  if (threadIdx.x != 0 || q.scal[SC_CONVERGED] == 0.0) return;
  restart_scalars(q);
}

hipError_t qp_restart_if_converged(const QPBatch& qb, hipStream_t st) {
  const int64_t g = (qb.h.state_len + NT - 1) / NT;
  hipLaunchKernelGGL(k_restart_copy, grid2(g < 256 ? g : 256, qb.B), dim3(NT), 0, st, qb.d);
  hipLaunchKernelGGL(k_restart_scal, grid2(1, qb.B), dim3(64), 0, st, qb.d);
  return hipGetLastError();
}

// Convergence summary of a batch (the input of the cross-GPU all-reduce,
// SURVEY.md §8e; the stopping rule res < 1e-8 and mu < 1e-8 of
// Optimizer.cpp:124-135): out = {max res, max mu, unconverged count} -- all
// three MAX-reducible, so ONE all-reduce (MAX) over the ranks decides the
// stop: every QP of the job converged <=> the reduced out[2] == 0.
__global__ __launch_bounds__(NT) void k_batch_summary(const QPDev* __restrict__ qs, int B, double* __restrict__ out) {
  __shared__ double sh[3][NT];
  double r = 0.0, m = 0.0, u = 0.0;
  for (int b = threadIdx.x; b < B; b += NT) {
    const double* sc = qs[b].scal;
    r = fmax(r, sc[SC_RES]);
    m = fmax(m, sc[SC_MU]);
    u += sc[SC_CONVERGED] != 0.0 ? 0.0 : 1.0;
  }
  sh[0][threadIdx.x] = r;
  sh[1][threadIdx.x] = m;
  sh[2][threadIdx.x] = u;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sh[0][threadIdx.x] = fmax(sh[0][threadIdx.x], sh[0][threadIdx.x + s]);
      sh[1][threadIdx.x] = fmax(sh[1][threadIdx.x], sh[1][threadIdx.x + s]);
      sh[2][threadIdx.x] += sh[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) out[threadIdx.x] = sh[threadIdx.x][0];
}
hipError_t qp_batch_summary(const QPBatch& qb, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_batch_summary, dim3(1), dim3(NT), 0, st, qb.d, qb.B, out);
  return hipGetLastError();
}

// snapshot of the initial iterate (restart source)
__global__ void k_save_initial(const QPDev* __restrict__ qs) {
  const QPDev& q = qs[blockIdx.y];
  for (int64_t t = blockIdx.x * (int64_t)NT + threadIdx.x; t < q.state_len; t += (int64_t)gridDim.x * NT) {
    q.v0[t] = q.v[0][t];
    q.r0[t] = q.r[0][t];
    if (q.eqpen && t < q.p) q.Cx0[t] = q.Cx[t];
  }
  if (blockIdx.x == 0 && threadIdx.x < SC_COUNT) q.scal0[threadIdx.x] = q.scal[threadIdx.x];
}
hipError_t qp_save_initial(const QPBatch& qb, hipStream_t st) {
  const int64_t g = (qb.h.state_len + NT - 1) / NT;
  hipLaunchKernelGGL(k_save_initial, grid2(g < 256 ? g : 256, qb.B), dim3(NT), 0, st, qb.d);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Fused per-QP step phases for batches of small systems (config C4): ONE
// workgroup per QP runs every O(N) / O(n^2) phase between the factor and the
// solves, so a Newton step is six launches (pre, factor, solve, mid, solve,
// post) instead of ~25 -- at 128 QPs per GPU the short grid kernels above
// were ~5 us each, a quarter of the step.  Shared with the grid kernels, each
// stated once: the element formulas (*_elem), the KKT diagonal (kkt_diag),
// the scalars after a reduction (stats_store, centering, restart_scalars) and
// the loop bounds (kernels.h *_rows) -- bitwise the same values; only the
// reductions (res, comp, f, mu_aff) sum in a different order.  Not shared:
// the off-diagonal copy (see assemble_row) and the mat-vecs.
constexpr int FT = 512;  // 8 waves

// restart-if-converged, KKT assembly, affine rhs.  gridDim.x workgroups per
// QP (blockIdx.y): the off-diagonal copy (independent of the iterate) is
// split over all of them; workgroup 0 also restarts, writes the diagonal and
// the rhs (which read the iterate) in that order.
// kmode (kernels.h KMODE_*): where the matrix goes -- K whole, or the kept
// K0 (its off-diagonal part once per data load, its diagonal every step)
// skip (IPMZ_STEP_SKIP_CONVERGED): a converged QP's workgroups return here,
// after QP 0's lead has done its work for the whole batch; the lead of every
// other QP counts the step in SC_STEPS
__global__ __launch_bounds__(FT) void k_fused_pre(const QPDev* __restrict__ qs, int restart, int* info, int kmode,
                                                  int skip) {
  const QPDev& q = qs[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool lead = blockIdx.x == 0 && kmode != KMODE_K0_OFFDIAG;
  double* const KT = kmode == KMODE_K ? q.K : q.K0;
  if (info && lead && blockIdx.y == 0 && tid == 0) *info = 0x7f7f7f7f;  // the factor's first-failure word
  if (skip) {
    if (q.scal[SC_CONVERGED] != 0.0) return;
    if (lead && tid == 0) q.scal[SC_STEPS] += 1.0;
  }
  if (lead && restart && q.scal[SC_CONVERGED] != 0.0) {
    for (int64_t t = tid; t < q.state_len; t += FT) restart_elem(q, t);
    __syncthreads();  // every thread has read SC_CONVERGED
    if (tid == 0) restart_scalars(q);
    __syncthreads();  // v, r and mu_new restored before assembly reads them
  }
  // strict lower triangle in 128-column units (a wave per unit, a column
  // pair per lane), eight units per wave in flight: one workgroup moves the
  // QP's ~0.8 MB only with many loads outstanding
  const int N = q.N, n = q.n, m = q.m, nm = q.n + q.mk;
  const int nch = (N + 127) / 128, units = kmode == KMODE_K0_DIAG ? 0 : N * nch;
  for (int u0 = (blockIdx.x * (FT / 64) + wave) * 8; u0 < units; u0 += gridDim.x * (FT / 64) * 8) {
    double v0[8], v1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int u = u0 + k, i = u / nch, j = (u % nch) * 128 + 2 * lane;
      v0[k] = v1[k] = 0.0;
      if (u < units) {
        // NaiveSlacks: the lambda_g rows hold -A, the lambda_h rows A
        const bool ah = q.naive && i >= n + m && i < nm;
        const double* src = i < n ? q.Q + (int64_t)i * q.ldn
                           : i < nm ? q.A + (int64_t)(ah ? i - n - m : i - n) * q.ldn : q.C + (int64_t)(i - nm) * q.ldn;
        const bool neg = q.naive && i >= n && i < n + m;
        const int lim = i < n ? i : n;  // source columns [0, lim); zeros in [n, i)
        if (j + 1 < lim) {  // one 16-byte load (ldn and j even)
          const double2 t = *reinterpret_cast<const double2*>(src + j);
          v0[k] = neg ? -t.x : t.x;
          v1[k] = neg ? -t.y : t.y;
        } else if (j < lim) {
          v0[k] = neg ? -src[j] : src[j];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int u = u0 + k, i = u / nch, j = (u % nch) * 128 + 2 * lane;
      if (u < units) {
        double* Kr = KT + (int64_t)i * q.ldk;
        if (j + 1 < i) *reinterpret_cast<double2*>(Kr + j) = make_double2(v0[k], v1[k]);  // ldk even
        else if (j < i) Kr[j] = v0[k];
      }
    }
  }
  if (!lead) return;
  for (int i = tid; i < N; i += FT) KT[(int64_t)i * q.ldk + i] = kkt_diag(q, i);
  for (int t = tid; t < N; t += FT) rhs_elem(q, t);
}

// predictor back-substitution, alpha_aff, mu_aff / sigma, corrector rows,
// corrector rhs
// (T threads per QP; sh: T / 64 doubles of LDS)
template <int T>
__device__ __forceinline__ void fused_mid_body(const QPDev& q, double* sh) {
  const int tid = threadIdx.x;
  const int N = q.N, nm = comp_rows(q);
  const DSel D = dsel(q, 0);
  for (int t = tid; t < N; t += T) backsub_elem(q, D, t);
  __syncthreads();
  double a = 1.0;
  for (int t = tid; t < nm; t += T) ratio_elem(q, D, t, a);
  a = block_allmin<T>(a, sh);
  if (tid == 0) q.scal[SC_ALPHA_AFF] = a;
  double s = 0.0;
  for (int t = tid; t < nm; t += T) mu_aff_elem(q, t, a, s);
  s = block_allsum<T>(s, sh);
  // every thread evaluates the same scalars; thread 0 stores them
  const Centering c = centering(q, s);
  const int rows = corrector_rows(q);
  for (int t = tid; t < rows; t += T) corrector_elem(q, t, c.mu_new);
  __syncthreads();  // SC_MU read by every thread; corrector rows written
  if (tid == 0) centering_store(q, c);
  for (int t = tid; t < N; t += T) rhs_elem(q, t);
}
__global__ __launch_bounds__(FT) void k_fused_mid(const QPDev* __restrict__ qs, int skip) {
  __shared__ double sh[FT / 64];
  if (skip && qs[blockIdx.x].scal[SC_CONVERGED] != 0.0) return;
  fused_mid_body<FT>(qs[blockIdx.x], sh);
}

// corrector back-substitution, alpha, the update (one workgroup per QP)
template <int T>
__device__ __forceinline__ void fused_post_body(const QPDev& q, int freeze, double* sh) {
  const int tid = threadIdx.x;
  const int N = q.N, nm = comp_rows(q);
  const DSel D = dsel(q, 1);
  const bool frozen = freeze && q.scal[SC_CONVERGED] != 0.0;
  for (int t = tid; t < N; t += T) backsub_elem(q, D, t);
  __syncthreads();
  double a = 1.0;
  for (int t = tid; t < nm; t += T) ratio_elem(q, D, t, a);
  a = block_allmin<T>(a, sh);
  if (tid == 0) q.scal[SC_ALPHA] = a;
  if (!frozen) {
    const int mx = update_rows(q);
    for (int t = tid; t < mx; t += T) update_elem(q, t, 0.995 * a);
  }
}
__global__ __launch_bounds__(FT) void k_fused_post(const QPDev* __restrict__ qs, int freeze, int skip) {
  __shared__ double sh[FT / 64];
  if (skip && qs[blockIdx.x].scal[SC_CONVERGED] != 0.0) return;
  fused_post_body<FT>(qs[blockIdx.x], freeze, sh);
}

// The four per-QP phases between the factor and the evaluation in ONE
// workgroup per QP: predictor solve, the middle phase (k_fused_mid), corrector
// solve, the corrector back-substitution and update (k_fused_post) -- no
// dependency crosses QPs, so a QP moves on when its own phase is done instead
// of waiting for the whole batch at three kernel boundaries.  Each phase is
// the kernel's code (trsv_small.h, the bodies above) with a workgroup
// barrier in between (its global stores visible to the next phase's loads:
// every wave of the workgroup shares the CU's L1).  NW = 8: the same values
// as the separate launches, bitwise; NW = 16: the middle / post reductions
// over 16 wave partials.  (NW = 8: at most 128 VGPRs, two workgroups per CU
// like trsv_small_kernel<8>.)
template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW == 8 ? 4 : 1))) void k_fused_solves(const QPDev* __restrict__ qs, const double* __restrict__ K,
                                                          int64_t ld, int N, const double* D,
                                                          const double* __restrict__ Linv, double* b,
                                                          int64_t sK, int64_t sD, int64_t sL, int64_t sb,
                                                          int freeze, int skip) {
  // (b and D without __restrict__: the middle and post phases reach the
  // same vectors through qs[i].b / the QP's D as well)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double sh[NW];
  const int64_t i = blockIdx.x;
  const QPDev& q = qs[i];
  if (skip && q.scal[SC_CONVERGED] != 0.0) return;
  K += i * sK;
  D += i * sD;
  Linv += i * sL;
  b += i * sb;
  trsv_small_body<NW>(K, ld, N, D, Linv, b, sm);
  __syncthreads();
  fused_mid_body<64 * NW>(q, sh);
  __syncthreads();
  trsv_small_body<NW>(K, ld, N, D, Linv, b, sm);
  __syncthreads();
  fused_post_body<64 * NW>(q, freeze, sh);
}

// Evaluation of the new iterate (Qx, Ax, Cx, A^T lambda_A, C^T lambda_C,
// then residuals, f, res, mu): gridDim.x workgroups per QP (blockIdx.y)
// share the matvec rows and transpose columns; the last to arrive (counter
// q.done, reset by it) runs the residual pass and the stats.
// skip: a converged QP's workgroups return before they arrive at q.done (the
// flag is this kernel's own output: written by the last workgroup to arrive,
// after every workgroup of the QP has read it here)
__global__ __launch_bounds__(FT) __attribute__((amdgpu_waves_per_eu(8))) void k_fused_eval(const QPDev* __restrict__ qs,
                                                                                             int skip) {
  const QPDev& q = qs[blockIdx.y];
  if (skip && q.scal[SC_CONVERGED] != 0.0) return;
  __shared__ double sh[FT / 64];
  __shared__ unsigned last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = q.n, m = q.m, p = q.p;
  const int gw = blockIdx.x * (FT / 64) + wave, nw = gridDim.x * (FT / 64);
  const double* x = q.v[X];
  const int nr = residual_rows(q);  // (a product row of Q, A, C per residual element)
  auto row_ptr = [&](int r) {
    return r < n ? q.Q + (int64_t)r * q.ldn
                 : r < n + m ? q.A + (int64_t)(r - n) * q.ldn : q.C + (int64_t)(r - n - m) * q.ldn;
  };
  // four rows per wave at a time (their loads interleaved); each row's sum
  // in row_dot's order
  for (int r0 = gw * 4; r0 < nr; r0 += nw * 4) {
    double s0[4], s1[4];
    const double* rp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s0[k] = s1[k] = 0.0;
      rp[k] = row_ptr(r0 + k < nr ? r0 + k : r0);
    }
    int j = lane * 2;
    for (; j + 1 < n; j += 128) {
      const double2 b = *reinterpret_cast<const double2*>(x + j);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double2 a = *reinterpret_cast<const double2*>(rp[k] + j);
        s0[k] += a.x * b.x;
        s1[k] += a.y * b.y;
      }
    }
    if (j < n) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s0[k] += rp[k][j] * x[j];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = wave_sum(s0[k] + s1[k]);
      const int r = r0 + k;
      if (lane == 0 && r < nr) st_sc1(r < n ? &q.Qx[r] : r < n + m ? &q.Ax[r - n] : &q.Cx[r - n - m], d);
    }
  }
  // transposes: one thread per (column j, chunk of FCH rows), the chunk
  // summed in row order (its loads all in flight), the chunk partials then
  // added in chunk order through LDS; passes of FT / nch columns spread over
  // the QP's workgroups (a thread per column walking all the rows was
  // ~16 us of dependent load batches at C4)
  constexpr int FCH = 8;
  __shared__ double tp[FT];
  auto transpose = [&](const double* M, auto yf, int rows, double* out) {
    const int nch = (rows + FCH - 1) / FCH;
    if (nch > FT) {  // (not at the fused path's sizes) thread per column
      for (int j = blockIdx.x * FT + tid; j < n; j += gridDim.x * FT) {
        double tot = 0.0;
        for (int i0 = 0; i0 < rows; i0 += FCH) {
          const int i1 = i0 + FCH < rows ? i0 + FCH : rows;
          double c = 0.0;
          for (int i = i0; i < i1; ++i) c += M[(int64_t)i * q.ldn + j] * yf(i);
          tot += c;
        }
        st_sc1(&out[j], tot);
      }
      return;
    }
    const int cpp = FT / nch;  // columns per pass
    const int jj = tid % cpp, h = tid / cpp;
    const int npass = (n + cpp - 1) / cpp;
    for (int pi = blockIdx.x; pi < npass; pi += gridDim.x) {  // (uniform per workgroup)
      const int j = pi * cpp + jj;
      double c = 0.0;
      if (h < nch && j < n) {
        const int i0 = h * FCH, i1 = i0 + FCH < rows ? i0 + FCH : rows;
#pragma unroll
        for (int i = i0; i < i0 + FCH; ++i)
          if (i < i1) c += M[(int64_t)i * q.ldn + j] * yf(i);
      }
      __syncthreads();  // the previous pass's reads of tp
      tp[tid] = c;
      __syncthreads();
      if (tid < cpp && j < n) {
        double tot = 0.0;
        for (int k = 0; k < nch; ++k) tot += tp[k * cpp + tid];
        st_sc1(&out[j], tot);
      }
    }
  };
  if (m) transpose(q.A, [&](int i) { return a_dual(q, i); }, m, q.ATl);
  if (p) transpose(q.C, [&](int i) { return q.v[LC][i]; }, p, q.CTl);
  // arrival (sync.h protocol: write-through data, vmcnt drained, barrier, one
  // agent-scope atomic); no cache-wide fences
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    last = __hip_atomic_fetch_add(q.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!last) return;
  if (tid == 0) st_sc1(q.done, 0u);
  double res2 = 0.0, comp = 0.0, fa = 0.0, fb = 0.0;
  // (residual_rows elements, not N: NaiveSlacks has 2 m KKT rows for the m elements of the inequality block, and an
  // element past the last one would read and write the equality slots out of range)
  for (int t = tid; t < nr; t += FT) residual_elem<true>(q, t, 0.0, res2, comp, fa, fb);
  res2 = block_allsum<FT>(res2, sh);
  comp = block_allsum<FT>(comp, sh);
  fa = block_allsum<FT>(fa, sh);
  fb = block_allsum<FT>(fb, sh);
  if (tid == 0) stats_store(q, res2, comp, fa + fb);
}

// about two workgroups per CU: a lone workgroup per QP cannot keep enough
// loads in flight
static int fused_split(int B) {
  const int s = (2 * device_cus() + B - 1) / B;
  return s < 1 ? 1 : (s > 8 ? 8 : s);
}

hipError_t qp_fused_pre(const QPBatch& qb, int restart, int* info, hipStream_t st, int kmode) {
  if (kmode != KMODE_K && !qb.h.K0) return hipErrorInvalidValue;
  // the diagonal-only mode has no copy to spread: one workgroup per QP
  const int split = kmode == KMODE_K0_DIAG ? 1 : fused_split(qb.B);
  hipLaunchKernelGGL(k_fused_pre, dim3(split, qb.B), dim3(FT), 0, st, qb.d, kmode == KMODE_K0_OFFDIAG ? 0 : restart,
                     kmode == KMODE_K0_OFFDIAG ? nullptr : info, kmode, kmode == KMODE_K0_OFFDIAG ? 0 : qb.skip);
  return hipGetLastError();
}
hipError_t qp_fused_mid(const QPBatch& qb, hipStream_t st) {
  hipLaunchKernelGGL(k_fused_mid, dim3(qb.B), dim3(FT), 0, st, qb.d, qb.skip);
  return hipGetLastError();
}
hipError_t qp_fused_solves(const QPBatch& qb, const double* K, int64_t ld, int N, const double* D, const double* Linv,
                           double* b, int64_t sK, int64_t sD, int64_t sL, int64_t sb, int freeze, hipStream_t st) {
  if (!fused_solves_ok(N, ld)) return hipErrorInvalidValue;
  // 16 waves when the batch leaves a CU per QP, 8 when QPs share CUs (trsv.hip)
  if (qb.B <= device_cus())
    hipLaunchKernelGGL(k_fused_solves<16>, dim3(qb.B), dim3(64 * 16), trsv_small_lds(N, 16), st, qb.d, K, ld, N, D,
                       Linv, b, sK, sD, sL, sb, freeze, qb.skip);
  else
    hipLaunchKernelGGL(k_fused_solves<8>, dim3(qb.B), dim3(64 * 8), trsv_small_lds(N, 8), st, qb.d, K, ld, N, D, Linv,
                       b, sK, sD, sL, sb, freeze, qb.skip);
  return hipGetLastError();
}
// the evaluation's workgroups per QP: enough for two row passes (4 rows per
// wave, 8 waves) as long as the whole grid stays resident (8 waves per SIMD
// at 64 VGPRs: 4 workgroups per CU).  C4: B = 1024 -> 1, B = 128 -> 5
// (0.038 -> 0.035 ms against the 4 of fused_split; 2 or 8 slower,
// profiles/r05_s/c4_eval_split_ab.txt)
static int eval_split(const QPBatch& qb) {
  const int cap = 4 * device_cus() / qb.B;
  const int rows = (residual_rows(qb.h) + 63) / 64;
  const int s = rows < cap ? rows : cap;
  return s < 1 ? 1 : (s > 8 ? 8 : s);
}
hipError_t qp_fused_eval(const QPBatch& qb, hipStream_t st) {
  hipLaunchKernelGGL(k_fused_eval, dim3(eval_split(qb), qb.B), dim3(FT), 0, st, qb.d, qb.skip);
  return hipGetLastError();
}
hipError_t qp_fused_post(const QPBatch& qb, int freeze, hipStream_t st) {
  hipLaunchKernelGGL(k_fused_post, dim3(qb.B), dim3(FT), 0, st, qb.d, freeze, qb.skip);
  hipLaunchKernelGGL(k_fused_eval, dim3(eval_split(qb), qb.B), dim3(FT), 0, st, qb.d, qb.skip);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Centering on the central path (ipmz_batch_center; DESIGN.md "Centering on the
// central path"): damped Newton toward r(z; mu = kappa) = 0 with kappa a constant
// of the call.  Nothing of the Newton step is restated: the test is the step's
// own residual pass at mu = kappa (k_residuals, the evaluation's launch without
// its statistics) followed by the infinity norm over the residual slots, the
// direction is ipmz_*_newton_solve_multi's map for one row per QP on the
// solver's own slots (qp.cpp), the update is k_update behind its gate.
//
// The norm crosses workgroups without atomics: every workgroup of a QP writes
// the maximum of its strided share of the state_len residuals (two per lane and
// load: the slots are contiguous and 16-byte aligned) to its own partial, and
// one thread per QP of the summary launch takes the maximum over the partials
// in index order.  A NaN counts as +infinity, so it never passes e <= tol.  A
// QP that passed is frozen: the flag is only ever raised, and the norm, the
// summary and the update skip it.
__global__ __launch_bounds__(NT) void k_center_norm(const QPDev* __restrict__ qs, CenterWs w) {
  if (w.frozen[blockIdx.y]) return;
  const QPDev& q = qs[blockIdx.y];
  __shared__ double sh[NT / 64];
  const double* __restrict__ r = q.r[0];
  auto mag = [](double v) {
    v = fabs(v);
    return v == v ? v : INFINITY;
  };
  const int64_t pairs = q.state_len / 2;
  double a = 0.0;
  for (int64_t t = blockIdx.x * (int64_t)NT + threadIdx.x; t < pairs; t += (int64_t)gridDim.x * NT) {
    const double2 v = reinterpret_cast<const double2*>(r)[t];
    a = fmax(a, fmax(mag(v.x), mag(v.y)));
  }
  if ((q.state_len & 1) && blockIdx.x == 0 && threadIdx.x == 0) a = fmax(a, mag(r[q.state_len - 1]));
  a = wave_max(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < NT / 64; ++k) a = fmax(a, sh[k]);
    w.part[blockIdx.y * (int64_t)w.nb + blockIdx.x] = a;
  }
}
// the test of every QP not yet frozen, and the host's look: sum = {QPs not centered, the largest e among them}
__global__ __launch_bounds__(NT) void k_center_summary(int B, double tol, CenterWs w) {
  __shared__ double sh[2][NT];
  double open = 0.0, worst = 0.0;
  for (int b = threadIdx.x; b < B; b += NT) {
    if (w.frozen[b]) continue;
    double e = 0.0;
    for (int k = 0; k < w.nb; ++k) e = fmax(e, w.part[b * (int64_t)w.nb + k]);
    w.e[b] = e;
    if (e <= tol) {
      w.frozen[b] = 1;
    } else {
      open += 1.0;
      worst = fmax(worst, e);
    }
  }
  sh[0][threadIdx.x] = open;
  sh[1][threadIdx.x] = worst;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
      sh[1][threadIdx.x] = fmax(sh[1][threadIdx.x], sh[1][threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) w.sum[threadIdx.x] = sh[threadIdx.x][0];
}

int qp_center_blocks(const QPBatch& qb) { return red_blocks((int)((qb.h.state_len + 1) / 2)); }

hipError_t qp_center_test(const QPBatch& qb, double kappa, double tol, const CenterWs& w, hipStream_t st) {
  evaluate_products(qb, st);
  hipLaunchKernelGGL(k_residuals, grid2(red_blocks(residual_rows(qb.h)), qb.B), dim3(NT), 0, st, qb.d, kappa, 0);
  hipLaunchKernelGGL(k_center_norm, grid2(w.nb, qb.B), dim3(NT), 0, st, qb.d, w);
  hipLaunchKernelGGL(k_center_summary, dim3(1), dim3(NT), 0, st, qb.B, tol, w);
  return hipGetLastError();
}

hipError_t qp_center_update(const QPBatch& qb, const CenterWs& w, hipStream_t st) {
  return launch_update(qb, 0, UpdateGate{w.frozen, w.alpha, w.iters}, st);
}

}  // namespace ipmz
