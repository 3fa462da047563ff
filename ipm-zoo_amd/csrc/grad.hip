// Gradients of the residual vectors with respect to the problem data
// (ipmz_batch_data_vjp): with w one cotangent row per QP in the layout of
// IPMZ_STATE_RES (the adjoint solve's Out), g_theta = (d r / d theta)^T w at the
// QP's iterate, written into a caller's strided blocks -- per QP, or, for a
// block every QP shares (QP stride 0), summed over the batch.
//
// Every r_v of residual_elem (newton.hip) is affine in the data, and the only
// bilinear terms are the three matvecs.  Their gradients have one shape,
//
//     g[i][j] = ra[i] x[j] + rb[i] w_x[j]        (grad_row_factors below)
//
// Q: ra = w_x, no rb (rank 1; the n^2 entries of Q are independent, so gQ is
//    w_x x^T, not symmetrised);
// A: ra = the cotangent of the row A x sits in, rb = the dual A^T multiplies;
// C: ra = w_lambda_C, rb = lambda_C.
//
// Per-QP matrix blocks are pure stores (batch * rows * n * 8 bytes written,
// O(n) read): a wave per row, the row's two factors in registers, consecutive
// lanes on consecutive columns, 16-byte stores where the block allows them.
// Shared matrix blocks are a GEMM with the batch as the K dimension on
// v_mfma_f64_16x16x4: K split into chunks of IPMZ_VJP_KCHUNK QPs, one partial
// tile per chunk in the solver's workspace, summed in chunk order by a second
// launch -- no atomics, an order fixed by the shape alone.
#include "common.h"
#include "kernels.h"

namespace ipmz {

namespace {
constexpr int NT = 256;
constexpr int KCHUNK = IPMZ_VJP_KCHUNK;
constexpr int NJ = 4;  // 16-column tiles of one wave's strip (they share the row operands)
constexpr int KG = 4;  // MFMA steps (4 QPs each) whose operands are loaded together

dim3 grad_grid(int64_t per, int B) {  // io.hip's io_grid: x over one QP's work (grid-stride), y over the QPs (looped)
  int64_t gx = (per + NT - 1) / NT;
  gx = gx < 1 ? 1 : gx > 2048 ? 2048 : gx;
  int64_t gy = 4096 / gx;
  gy = gy < 1 ? 1 : gy > B ? B : gy;
  return dim3((unsigned)gx, (unsigned)gy);
}

// element i of slot `slot` of a cotangent row in the layout of IPMZ_STATE_RES.  The slots' offsets are those of any
// QP of the batch (one formulation, one shape): q0 = qs[0], so that they are uniform loads, hoisted out of every loop
__device__ __forceinline__ double cot(const QPDev& q0, const double* __restrict__ w, int slot, int i) {
  return w[(q0.r[slot] - q0.r[0]) + i];
}

// Row i's two factors of g[i][j] = ra x[j] + rb w_x[j], by the block and the formulation (MODE, uniform over the
// launch; G_Q is rank 1, rb unused).  The coefficients are those of residual_elem (newton.hip), restated here
// because a bilinear term has no element-local form to call:
//   G_Q        r_x has + (Q*x)                                    ("s = s + mv(&q.Qx[i])")
//   G_A        r_x has + (A^T*lambda_A) (a_dual); r_lambda_A = ((A*x) - s)   ("rla = mv(&q.Ax[i]) + (-q.v[S][i])")
//   G_A_NAIVE  r_x has + (A^T*(lambda_h - lambda_g)) (a_dual's NaiveSlacks branch); r_lambda_g = (l_A + g - (A*x)),
//              r_lambda_h = (h + (A*x) - u_A)                     ("rlg", "rlh" of the naive branch)
//   G_C        r_x has + (C^T*lambda_C); r_lambda_C = (C*x) ... in all three equality handlings ("rlc": eqnone,
//              eqpen's -(d + mu lambda_C - (C*x)), Regularization)
// q0: the offsets (above); q: the QP whose iterate is read.
enum { G_Q = 0, G_A = 1, G_A_NAIVE = 2, G_C = 3 };
template <int MODE>
__device__ __forceinline__ void grad_row_factors(const QPDev& q0, const QPDev& q, const double* __restrict__ w, int i,
                                                 double& ra, double& rb) {
  if (MODE == G_Q) {
    ra = w[i];  // (x leads the Newton order)
    rb = 0.0;
  } else if (MODE == G_A) {
    ra = cot(q0, w, LA, i);
    rb = q.v[LA][i];
  } else if (MODE == G_A_NAIVE) {
    ra = cot(q0, w, LH, i) + (-cot(q0, w, LG, i));
    rb = q.v[LH][i] + (-q.v[LG][i]);
  } else {
    ra = cot(q0, w, LC, i);
    rb = q.v[LC][i];
  }
}
template <int MODE>
__device__ __forceinline__ double grad_elem(double ra, double rb, double x, double wx) {
  return MODE == G_Q ? ra * x : ra * x + rb * wx;
}

// The six vector gradients of element t (t < n: c, l_x, u_x; t < m: l_A, u_A; t < p: d), again residual_elem's
// coefficients: r_x = (c + ...); SlackedSlacks / NaiveSlacks rows (l + y - x), (x + z - u), (l_A + g - s | (A*x)),
// (h + s | (A*x) - u_A); Slacks rows ((X - L_x)*lambda_y), ((U_x - X)*lambda_z), ((S - L_A)*lambda_g),
// ((U_A - S)*lambda_h); every r_lambda_C has - d.  A bound the formulation does not have: 0.  q0: the formulation
// and the offsets; q: the QP whose iterate is read (Slacks only).
struct VecGrad {
  double c, lx, ux, lA, uA, d;
};
__device__ __forceinline__ VecGrad vec_grad_elem(const QPDev& q0, const QPDev& q, const double* __restrict__ w, int t) {
  VecGrad g{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool sl = q0.slacks && !q0.naive;
  if (t < q0.n) {
    g.c = w[t];
    if (q0.vlo) g.lx = q0.slacks ? -(q.v[LY][t] * cot(q0, w, LY, t)) : cot(q0, w, LY, t);
    if (q0.vup) g.ux = q0.slacks ? q.v[LZ][t] * cot(q0, w, LZ, t) : -cot(q0, w, LZ, t);
  }
  if (t < q0.m) {
    if (q0.alo) g.lA = sl ? -(q.v[LG][t] * cot(q0, w, LG, t)) : cot(q0, w, LG, t);
    if (q0.aup) g.uA = sl ? q.v[LH][t] * cot(q0, w, LH, t) : -cot(q0, w, LH, t);
  }
  if (t < q0.p) g.d = -cot(q0, w, LC, t);
  return g;
}
}  // namespace

// ---------------------------------------------------------------------------
// The per-QP vector blocks (QP stride != 0, or a solver of one QP) in one
// launch: QP z's gradient at out + z * stride.
__global__ void __launch_bounds__(NT) k_grad_vectors(const QPDev* __restrict__ qs, const double* __restrict__ W,
                                                     int64_t sW, QpGradOut o, int B) {
  const QPDev& q0 = qs[0];
  const int n = q0.n, m = q0.m, p = q0.p;
  const int mx = n > m ? (n > p ? n : p) : (m > p ? m : p);
  for (int z = blockIdx.y; z < B; z += gridDim.y) {
    const double* w = W + (int64_t)z * sW;
    for (int t = blockIdx.x * NT + threadIdx.x; t < mx; t += gridDim.x * NT) {
      const VecGrad g = vec_grad_elem(q0, qs[z], w, t);
      if (t < n) {
        if (o.c) o.c[(int64_t)z * o.sc + t] = g.c;
        if (o.lx) o.lx[(int64_t)z * o.slx + t] = g.lx;
        if (o.ux) o.ux[(int64_t)z * o.sux + t] = g.ux;
      }
      if (t < m) {
        if (o.lA) o.lA[(int64_t)z * o.slA + t] = g.lA;
        if (o.uA) o.uA[(int64_t)z * o.suA + t] = g.uA;
      }
      if (t < p && o.d) o.d[(int64_t)z * o.sd + t] = g.d;
    }
  }
}

// The shared vector blocks in one launch: element t of a block = the sum over the batch, in an order fixed by the
// batch size alone -- the batch is cut into VS contiguous ranges of ceil(B / VS) QPs, a thread sums one range in QP
// order (VE elements x VS ranges per workgroup: one thread per element would wait out B dependent load latencies),
// and the ranges' sums are added in range order.
constexpr int VS = 64, VE = 16, VNT = VS * VE;
__global__ void __launch_bounds__(VNT) k_grad_vectors_shared(const QPDev* __restrict__ qs, const double* __restrict__ W,
                                                             int64_t sW, QpGradOut o, int B) {
  __shared__ double sh[6][VS][VE];
  const QPDev& q0 = qs[0];
  const int n = q0.n, m = q0.m, p = q0.p;
  const int mx = n > m ? (n > p ? n : p) : (m > p ? m : p);
  const int e = threadIdx.x % VE, range = threadIdx.x / VE;
  const int t = blockIdx.x * VE + e;
  const int zlen = (B + VS - 1) / VS, za = range * zlen, zb = za + zlen < B ? za + zlen : B;
  VecGrad s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < mx && q0.slacks) {  // (the iterate enters: vec_grad_elem itself)
    for (int z = za; z < zb; ++z) {
      const VecGrad g = vec_grad_elem(q0, qs[z], W + (int64_t)z * sW, t);
      s.c += g.c, s.lx += g.lx, s.ux += g.ux, s.lA += g.lA, s.uA += g.uA, s.d += g.d;
    }
  } else if (t < mx) {
    // every other formulation: vec_grad_elem is +w or -w of one slot per block, whatever the QP -- the slot's
    // offset and the sign once, then plain loads, four QPs' worth in flight together before they are added in QP
    // order (an absent element loads the row's head and adds 0; a QP past the range's end reloads its last one)
    const bool ok[6] = {t < n, t < n && q0.vlo, t < n && q0.vup, t < m && q0.alo, t < m && q0.aup, t < p};
    const int slot[6] = {X, LY, LZ, LG, LH, LC};
    const double sg[6] = {1.0, 1.0, -1.0, 1.0, -1.0, -1.0};
    int64_t off[6];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) off[k] = ok[k] ? (q0.r[slot[k]] - q0.r[0]) + t : 0;
    for (int z = za; z < zb; z += 4) {
      double v[4][6];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double* __restrict__ w = W + (int64_t)(z + u < zb ? z + u : zb - 1) * sW;
#pragma unroll
        for (int k = 0; k < 6; ++k) v[u][k] = w[off[k]];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += (ok[k] && z + u < zb) ? sg[k] * v[u][k] : 0.0;
    }
    s = VecGrad{acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]};
  }
  sh[0][range][e] = s.c, sh[1][range][e] = s.lx, sh[2][range][e] = s.ux;
  sh[3][range][e] = s.lA, sh[4][range][e] = s.uA, sh[5][range][e] = s.d;
  __syncthreads();
  // one thread per (block, element) adds the ranges' sums in range order
  const int k = threadIdx.x / VE;
  if (k >= 6 || t >= mx) return;
  double tot = 0.0;
  for (int r = 0; r < VS; ++r) tot += sh[k][r][e];
  double* const dst[6] = {o.c, o.lx, o.ux, o.lA, o.uA, o.d};
  const int len[6] = {n, n, n, m, m, p};
  if (dst[k] && t < len[k]) dst[k][t] = tot;
}

// ---------------------------------------------------------------------------
// One per-QP matrix block: g[i][j] of every QP to dst + z sq + i ld + j, j < n;
// columns [n, ld) and the space between QPs are not touched.  A wave per row
// (grid-stride over the rows), its factors in registers; VEC: 16-byte stores
// (the host checked that dst, ld and sq allow them), n / 2 pairs and, for odd
// n, one last element.  Both forms compute every element by the same
// expression: equal bits.
template <bool VEC, int MODE>
__global__ void __launch_bounds__(NT) k_grad_matrix(const QPDev* __restrict__ qs, const double* __restrict__ W,
                                                    int64_t sW, double* __restrict__ dst, int64_t ld, int64_t sq,
                                                    int rows, int B) {
  const QPDev& q0 = qs[0];
  const int n = q0.n;
  const int lane = threadIdx.x & 63;
  for (int z = blockIdx.y; z < B; z += gridDim.y) {
    const QPDev& q = qs[z];
    const double* __restrict__ w = W + (int64_t)z * sW;  // (w_x = the row's head)
    const double* __restrict__ x = q.v[X];
    double* out = dst + (int64_t)z * sq;
    for (int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6); i < rows; i += gridDim.x * (NT / 64)) {
      double ra, rb;
      grad_row_factors<MODE>(q0, q, w, i, ra, rb);
      double* row = out + (int64_t)i * ld;
      if (VEC) {
        for (int c = 2 * lane; c < n; c += 128) {
          if (c + 1 < n) {
            double2 v;
            v.x = grad_elem<MODE>(ra, rb, x[c], w[c]);
            v.y = grad_elem<MODE>(ra, rb, x[c + 1], w[c + 1]);
            *reinterpret_cast<double2*>(row + c) = v;
          } else {
            row[c] = grad_elem<MODE>(ra, rb, x[c], w[c]);
          }
        }
      } else {
        for (int c = lane; c < n; c += 64) row[c] = grad_elem<MODE>(ra, rb, x[c], w[c]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// One shared matrix block, first launch: G = sum_z ra_z x_z^T (+ rb_z w_x,z^T)
// over the QPs of one chunk, on v_mfma_f64_16x16x4.  Both operands are K-major
// -- QP z's row is contiguous in i and in j -- so the 16 lanes of an operand
// column (fragment layout of gemm.h: row = lane & 15, k = lane >> 4) load 16
// consecutive doubles of one QP: the row factors from W + z sW + the slot's
// offset and the QP's own state, x from QPDev's pointer; no packed copy.  A
// wave owns a 16 x 64 strip (NJ tiles sharing the row operands); waves are
// independent (no LDS, no barrier).  The K tail (a chunk's QP count not a
// multiple of 4) and the M / N tails are zeros in registers: a masked lane
// loads a valid address (the chunk's first QP, index 0) and discards it.  The
// chunk's KCHUNK / 4 steps go in groups of KG (steps past the batch's end are
// all mask).  The chunk's partial goes to part[chunk][rows][n], masked.
template <int MODE>
__global__ void __launch_bounds__(NT) k_grad_shared_part(const QPDev* __restrict__ qs, const double* __restrict__ W,
                                                         int64_t sW, int rows, int B, double* __restrict__ part) {
  typedef Mfma<double> MF;
  const QPDev& q0 = qs[0];
  const int n = q0.n;
  const int lane = threadIdx.x & 63;
  const int nstrip = (n + 16 * NJ - 1) / (16 * NJ), ntile = (rows + 15) / 16;
  const int wid = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (wid >= nstrip * ntile) return;  // (whole waves; nothing below synchronizes)
  const int i0 = (wid / nstrip) * 16, j0 = (wid % nstrip) * 16 * NJ;
  const int z0 = blockIdx.y * KCHUNK, z1 = z0 + KCHUNK < B ? z0 + KCHUNK : B;
  const int i = i0 + (lane & 15);
  const bool iok = i < rows;
  const int ic = iok ? i : 0;
  int jc[NJ];
  bool jok[NJ];
#pragma unroll
  for (int b = 0; b < NJ; ++b) {
    const int j = j0 + 16 * b + (lane & 15);
    jok[b] = j < n;
    jc[b] = jok[b] ? j : 0;
  }
  MF::acc_t acc[NJ];
#pragma unroll
  for (int b = 0; b < NJ; ++b) acc[b] = MF::acc_t{0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < KCHUNK / 4; s0 += KG) {
    // a group's operands into registers first, so that its loads are in flight together, then its MFMAs
    double ra[KG], rb[KG], xv[KG][NJ], wv[KG][NJ];
#pragma unroll
    for (int s = 0; s < KG; ++s) {
      const int z = z0 + 4 * (s0 + s) + (lane >> 4);
      const bool zok = z < z1;
      const QPDev& q = qs[zok ? z : z0];
      const double* __restrict__ w = W + (int64_t)(zok ? z : z0) * sW;
      const double* __restrict__ x = q.v[X];
      grad_row_factors<MODE>(q0, q, w, ic, ra[s], rb[s]);
      if (!(zok && iok)) ra[s] = rb[s] = 0.0;
#pragma unroll
      for (int b = 0; b < NJ; ++b) {
        xv[s][b] = x[jc[b]];
        if (!(zok && jok[b])) xv[s][b] = 0.0;
        if (MODE != G_Q) {
          wv[s][b] = w[jc[b]];
          if (!(zok && jok[b])) wv[s][b] = 0.0;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < KG; ++s)
#pragma unroll
      for (int b = 0; b < NJ; ++b) {
        acc[b] = MF::mma(ra[s], xv[s][b], acc[b]);
        if (MODE != G_Q) acc[b] = MF::mma(rb[s], wv[s][b], acc[b]);
      }
  }
  double* out = part + (int64_t)blockIdx.y * rows * n;
#pragma unroll
  for (int b = 0; b < NJ; ++b) {
    const int j = j0 + 16 * b + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int io = i0 + MF::row(lane, r);
      if (io < rows && j < n) out[(int64_t)io * n + j] = acc[b][r];
    }
  }
}

// second launch: dst[i ld + j] = the chunks' partials summed in chunk order
__global__ void __launch_bounds__(NT) k_grad_shared_sum(const double* __restrict__ part, int rows, int n, int nchunk,
                                                        double* __restrict__ dst, int64_t ld) {
  const int64_t per = (int64_t)rows * n;
  for (int64_t t = blockIdx.x * (int64_t)NT + threadIdx.x; t < per; t += (int64_t)gridDim.x * NT) {
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[c * per + t];
    dst[(t / n) * ld + t % n] = s;
  }
}

int64_t qp_grad_part_elems(const QPBatch& qb) {
  const QPDev& h = qb.h;
  const int64_t rows = h.n > h.m ? (h.n > h.p ? h.n : h.p) : (h.m > h.p ? h.m : h.p);
  return (int64_t)((qb.B + KCHUNK - 1) / KCHUNK) * rows * h.n;
}

static bool grad_vec_ok(const double* p, int64_t ld, int64_t sq) { return !((uintptr_t)p & 15) && !(ld & 1) && !(sq & 1); }

hipError_t qp_data_vjp(const QPBatch& qb, const double* W, int64_t sW, const QpGradOut& o, double* part,
                       hipStream_t st) {
  const QPDev& h = qb.h;
  const int B = qb.B;
  const struct {
    double* p;
    int64_t ld, sq;
    int rows, mode;
  } mats[3] = {{o.Q, o.ldq, o.sQ, h.n, G_Q}, {o.A, o.lda, o.sA, h.m, h.naive ? G_A_NAIVE : G_A}, {o.C, o.ldc, o.sC, h.p, G_C}};
  for (int w = 0; w < 3; ++w) {
    if (!mats[w].p || mats[w].rows == 0) continue;
    const int rows = mats[w].rows, mode = mats[w].mode;
    if (B > 1 && mats[w].sq == 0) {  // shared: the batch is the K dimension
      const int nchunk = (B + KCHUNK - 1) / KCHUNK;
      const int waves = ((h.n + 16 * NJ - 1) / (16 * NJ)) * ((rows + 15) / 16);
      const dim3 grid((waves + NT / 64 - 1) / (NT / 64), nchunk);
#define IPMZ_GRAD_PART(M) hipLaunchKernelGGL((k_grad_shared_part<M>), grid, dim3(NT), 0, st, qb.d, W, sW, rows, B, part)
      if (mode == G_Q) IPMZ_GRAD_PART(G_Q);
      else if (mode == G_A) IPMZ_GRAD_PART(G_A);
      else if (mode == G_A_NAIVE) IPMZ_GRAD_PART(G_A_NAIVE);
      else IPMZ_GRAD_PART(G_C);
#undef IPMZ_GRAD_PART
      hipLaunchKernelGGL(k_grad_shared_sum, grad_grid((int64_t)rows * h.n, 1), dim3(NT), 0, st, part, rows, h.n, nchunk,
                         mats[w].p, mats[w].ld);
      continue;
    }
    const int64_t sq = B > 1 ? mats[w].sq : 0;
    const dim3 grid = grad_grid((int64_t)rows * 64, B);  // a wave per row
    const bool vec = grad_vec_ok(mats[w].p, mats[w].ld, sq);
#define IPMZ_GRAD_MATRIX(M)                                                                                          \
  do {                                                                                                               \
    if (vec)                                                                                                         \
      hipLaunchKernelGGL((k_grad_matrix<true, M>), grid, dim3(NT), 0, st, qb.d, W, sW, mats[w].p, mats[w].ld, sq, rows, B); \
    else                                                                                                             \
      hipLaunchKernelGGL((k_grad_matrix<false, M>), grid, dim3(NT), 0, st, qb.d, W, sW, mats[w].p, mats[w].ld, sq, rows, B); \
  } while (0)
    if (mode == G_Q) IPMZ_GRAD_MATRIX(G_Q);
    else if (mode == G_A) IPMZ_GRAD_MATRIX(G_A);
    else if (mode == G_A_NAIVE) IPMZ_GRAD_MATRIX(G_A_NAIVE);
    else IPMZ_GRAD_MATRIX(G_C);
#undef IPMZ_GRAD_MATRIX
  }
  // the vector blocks: the per-QP ones in one launch, the shared ones in another
  QpGradOut per = o, sh = o;
  const bool one = B == 1;
  double* QpGradOut::*vecs[6] = {&QpGradOut::c, &QpGradOut::lx, &QpGradOut::ux, &QpGradOut::lA, &QpGradOut::uA, &QpGradOut::d};
  int64_t QpGradOut::*strides[6] = {&QpGradOut::sc, &QpGradOut::slx, &QpGradOut::sux, &QpGradOut::slA, &QpGradOut::suA, &QpGradOut::sd};
  bool any_per = false, any_sh = false;
  for (int k = 0; k < 6; ++k) {
    const bool is_per = one || o.*strides[k] != 0;
    if (is_per) sh.*vecs[k] = nullptr;
    else per.*vecs[k] = nullptr;
    any_per = any_per || (per.*vecs[k] != nullptr);
    any_sh = any_sh || (sh.*vecs[k] != nullptr);
  }
  const int mx = h.n > h.m ? (h.n > h.p ? h.n : h.p) : (h.m > h.p ? h.m : h.p);
  if (any_per) hipLaunchKernelGGL(k_grad_vectors, grad_grid(mx, B), dim3(NT), 0, st, qb.d, W, sW, per, B);
  if (any_sh)
    hipLaunchKernelGGL(k_grad_vectors_shared, dim3((mx + VE - 1) / VE), dim3(VNT), 0, st, qb.d, W, sW, sh, B);
  return hipGetLastError();
}

}  // namespace ipmz
