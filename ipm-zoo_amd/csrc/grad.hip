// Gradients of the residual vectors with respect to the problem data
// (ipmz_batch_data_vjp): with w one cotangent row per QP in the layout of
// IPMZ_STATE_RES (the adjoint solve's Out), g_theta = (d r / d theta)^T w at the
// QP's iterate, written into a caller's strided blocks -- per QP, or, for a
// block every QP shares (QP stride 0), summed over the batch.
//
// Every r_v of residual_elem (newton.hip) is affine in the data (data_terms.h
// states each term), and the only bilinear terms are the three matvecs.  Their
// gradients have one shape,
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
//
// A block of cotangent rows per QP (ipmz_batch_data_vjp_multi; row r of QP z at
// W + z sW + r ldw, its blocks at X + z sX + r tX): the (QP, row) pair is the
// looped grid dimension of the per-QP kernels, the row a grid dimension of the
// shared vector blocks.  In a shared matrix block x_z and the iterate's dual rb_z
// do not depend on the row, so a wave that owns a strip keeps them in registers
// over a group of RG rows and accumulates one tile set per row; every element
// still accumulates over the batch in the single row's order, so row r's bits
// are those of a call with that row alone.  The partials of IPMZ_VJP_SLAB rows
// pass through the workspace at a time, one slab after the other.
#include "common.h"
#include "data_terms.h"
#include "kernels.h"

namespace ipmz {

namespace {
constexpr int NT = 256;
constexpr int KCHUNK = IPMZ_VJP_KCHUNK;
constexpr int NJ = 4;  // 16-column tiles of one wave's strip (they share the row operands)
constexpr int KG = 4;  // MFMA steps (4 QPs each) whose operands are loaded together
constexpr int RG = 4;  // cotangent rows that share a strip's row-independent operands (x, the dual)
constexpr int SLAB = IPMZ_VJP_SLAB;
static_assert(SLAB % RG == 0, "whole row groups per slab");

static_assert(NT == GRID_NT, "block_grid's workgroups");

// element i of slot `slot` of a cotangent row in the layout of IPMZ_STATE_RES
__device__ __forceinline__ double cot(const QPDev& q0, const double* __restrict__ w, int slot, int i) {
  return w[slot_off(q0, slot) + i];
}

// Row i's two factors of g[i][j] = ra x[j] + rb w_x[j], by the block and the formulation (MODE, uniform over the
// launch; DM_Q is rank 1, rb unused): ra = the cotangent of the row the product M x enters, rb = the vector M^T
// multiplies in r_x (data_terms.h).  q0: the offsets; q: the QP whose iterate is read.
// (the two halves apart: ra alone depends on the cotangent row, rb alone on the iterate)
template <int MODE>
__device__ __forceinline__ double grad_row_ra(const QPDev& q0, const double* __restrict__ w, int i) {
  if (MODE == DM_Q) return w[i];  // (x leads the Newton order)
  return MODE == DM_A ? cot(q0, w, LA, i) : MODE == DM_A_NAIVE ? cot(q0, w, LH, i) + (-cot(q0, w, LG, i)) : cot(q0, w, LC, i);
}
template <int MODE>
__device__ __forceinline__ double grad_row_rb(const QPDev& q, int i) {
  if (MODE == DM_Q) return 0.0;
  return data_dual<MODE>(q, i);
}
template <int MODE>
__device__ __forceinline__ void grad_row_factors(const QPDev& q0, const QPDev& q, const double* __restrict__ w, int i,
                                                 double& ra, double& rb) {
  ra = grad_row_ra<MODE>(q0, w, i);
  rb = grad_row_rb<MODE>(q, i);
}
template <int MODE>
__device__ __forceinline__ double grad_elem(double ra, double rb, double x, double wx) {
  return MODE == DM_Q ? ra * x : ra * x + rb * wx;
}

// The six vector gradients of element t: vec_term (data_terms.h) of the cotangent of the slot the vector enters; a
// bound the formulation does not have: 0.  q0: the formulation and the offsets; q: the QP whose iterate is read
// (Slacks only).
struct VecGrad {
  double c, lx, ux, lA, uA, d;
};
template <int K>
__device__ __forceinline__ double vec_grad(const QPDev& q0, const QPDev& q, const double* __restrict__ w, int t) {
  return vec_term<K>(q0, q, t, cot(q0, w, vec_slot(K), t));
}
__device__ __forceinline__ VecGrad vec_grad_elem(const QPDev& q0, const QPDev& q, const double* __restrict__ w, int t) {
  VecGrad g{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < q0.n) {
    g.c = vec_grad<0>(q0, q, w, t);
    if (vec_has<1>(q0)) g.lx = vec_grad<1>(q0, q, w, t);
    if (vec_has<2>(q0)) g.ux = vec_grad<2>(q0, q, w, t);
  }
  if (t < q0.m) {
    if (vec_has<3>(q0)) g.lA = vec_grad<3>(q0, q, w, t);
    if (vec_has<4>(q0)) g.uA = vec_grad<4>(q0, q, w, t);
  }
  if (t < q0.p) g.d = vec_grad<5>(q0, q, w, t);
  return g;
}
}  // namespace

// ---------------------------------------------------------------------------
// The per-QP vector blocks (QP stride != 0, or a solver of one QP) in one
// launch: row r of QP z at out + z * stride + r * row stride; the (QP, row) pairs
// are the looped grid dimension.
__global__ void __launch_bounds__(NT) k_grad_vectors(const QPDev* __restrict__ qs, const double* __restrict__ W,
                                                     int64_t sW, int64_t ldw, QpBlocksOut o, int B, int ncot) {
  const QPDev& q0 = qs[0];
  const int n = q0.n, m = q0.m, p = q0.p;
  const int mx = update_rows(q0);
  for (int64_t zr = blockIdx.y; zr < (int64_t)B * ncot; zr += gridDim.y) {
    const int64_t z = zr / ncot, r = zr - z * ncot;
    const double* w = W + z * sW + r * ldw;
    for (int t = blockIdx.x * NT + threadIdx.x; t < mx; t += gridDim.x * NT) {
      const VecGrad g = vec_grad_elem(q0, qs[z], w, t);
      if (t < n) {
        if (o.p[DB_C]) o.p[DB_C][z * o.sq[DB_C] + r * o.tq[DB_C] + t] = g.c;
        if (o.p[DB_LX]) o.p[DB_LX][z * o.sq[DB_LX] + r * o.tq[DB_LX] + t] = g.lx;
        if (o.p[DB_UX]) o.p[DB_UX][z * o.sq[DB_UX] + r * o.tq[DB_UX] + t] = g.ux;
      }
      if (t < m) {
        if (o.p[DB_LA]) o.p[DB_LA][z * o.sq[DB_LA] + r * o.tq[DB_LA] + t] = g.lA;
        if (o.p[DB_UA]) o.p[DB_UA][z * o.sq[DB_UA] + r * o.tq[DB_UA] + t] = g.uA;
      }
      if (t < p && o.p[DB_D]) o.p[DB_D][z * o.sq[DB_D] + r * o.tq[DB_D] + t] = g.d;
    }
  }
}

// The shared vector blocks in one launch: element t of a block = the sum over the batch, in an order fixed by the
// batch size alone -- the batch is cut into VS contiguous ranges of ceil(B / VS) QPs, a thread sums one range in QP
// order (VE elements x VS ranges per workgroup: one thread per element would wait out B dependent load latencies),
// and the ranges' sums are added in range order.  Row r0 + blockIdx.y of every QP into row r0 + blockIdx.y of the
// blocks (the host launches at most VROWS rows at a time).
constexpr int VROWS = 32768;
constexpr int VS = 64, VE = 16, VNT = VS * VE;
__global__ void __launch_bounds__(VNT) k_grad_vectors_shared(const QPDev* __restrict__ qs, const double* __restrict__ W,
                                                             int64_t sW, int64_t ldw, QpBlocksOut o, int B,
                                                             int r0) {
  __shared__ double sh[6][VS][VE];
  const QPDev& q0 = qs[0];
  const int n = q0.n, m = q0.m, p = q0.p;
  const int mx = update_rows(q0);
  const int e = threadIdx.x % VE, range = threadIdx.x / VE;
  const int t = blockIdx.x * VE + e;
  const int zlen = (B + VS - 1) / VS, za = range * zlen, zb = za + zlen < B ? za + zlen : B;
  const int r = r0 + blockIdx.y;  // the cotangent row: a grid dimension
  const double* __restrict__ Wr = W + (int64_t)r * ldw;
  VecGrad s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < mx && q0.slacks) {  // (the iterate enters: vec_grad_elem itself)
    for (int z = za; z < zb; ++z) {
      const VecGrad g = vec_grad_elem(q0, qs[z], Wr + (int64_t)z * sW, t);
      s.c += g.c, s.lx += g.lx, s.ux += g.ux, s.lA += g.lA, s.uA += g.uA, s.d += g.d;
    }
  } else if (t < mx) {
    // every other formulation: vec_term is +w or -w of one slot per block, whatever the QP (vec_sign) -- the slot's
    // offset and the sign once, then plain loads, four QPs' worth in flight together before they are added in QP
    // order (an absent element loads the row's head and adds 0; a QP past the range's end reloads its last one)
    const bool ok[6] = {t < n, t < n && vec_has<1>(q0), t < n && vec_has<2>(q0),
                        t < m && vec_has<3>(q0), t < m && vec_has<4>(q0), t < p};
    int64_t off[6];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) off[k] = ok[k] ? slot_off(q0, vec_slot(k)) + t : 0;
    for (int z = za; z < zb; z += 4) {
      double v[4][6];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double* __restrict__ w = Wr + (int64_t)(z + u < zb ? z + u : zb - 1) * sW;
#pragma unroll
        for (int k = 0; k < 6; ++k) v[u][k] = w[off[k]];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += (ok[k] && z + u < zb) ? vec_sign(k) * v[u][k] : 0.0;
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
  for (int g = 0; g < VS; ++g) tot += sh[k][g][e];
  double* const dst[6] = {o.p[DB_C], o.p[DB_LX], o.p[DB_UX], o.p[DB_LA], o.p[DB_UA], o.p[DB_D]};
  const int64_t tq[6] = {o.tq[DB_C], o.tq[DB_LX], o.tq[DB_UX], o.tq[DB_LA], o.tq[DB_UA], o.tq[DB_D]};
  const int len[6] = {n, n, n, m, m, p};
  if (dst[k] && t < len[k]) dst[k][(int64_t)r * tq[k] + t] = tot;
}

// ---------------------------------------------------------------------------
// One per-QP matrix block: g[i][j] of row r of every QP to dst + z sq + r tq +
// i ld + j, j < n; columns [n, ld) and the space between rows and QPs are not
// touched.  The (QP, row) pairs are the looped grid dimension.  A wave per row
// (grid-stride over the rows), its factors in registers; VEC: 16-byte stores
// (the host checked that dst, ld, sq and tq allow them), n / 2 pairs and, for odd
// n, one last element.  Both forms compute every element by the same
// expression: equal bits.
template <bool VEC, int MODE>
__global__ void __launch_bounds__(NT) k_grad_matrix(const QPDev* __restrict__ qs, const double* __restrict__ W,
                                                    int64_t sW, int64_t ldw, double* __restrict__ dst, int64_t ld,
                                                    int64_t sq, int64_t tq, int rows, int B, int ncot) {
  const QPDev& q0 = qs[0];
  const int n = q0.n;
  const int lane = threadIdx.x & 63;
  for (int64_t zr = blockIdx.y; zr < (int64_t)B * ncot; zr += gridDim.y) {
    const int64_t z = zr / ncot, r = zr - z * ncot;  // the (QP, cotangent row) pair
    const QPDev& q = qs[z];
    const double* __restrict__ w = W + z * sW + r * ldw;  // (w_x = the row's head)
    const double* __restrict__ x = q.v[X];
    double* out = dst + z * sq + r * tq;
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
// all mask).  The chunk's partial goes to part[row][chunk][rows][n], masked.
//
// R cotangent rows per wave (blockIdx.z: the group; rows r0 = blockIdx.z R ..
// of the nr rows at W, ldw apart): x_z and rb_z, which no row enters, are
// loaded once per group of KG steps and serve the R rows' MFMAs; ra and w_x
// are the row's own.  acc[u][b] sees the terms of its element in the order of
// the single row (R = 1): s ascending, ra x before rb w_x.  A row past nr
// (whole waves: blockIdx.z alone decides) is neither loaded nor stored.
template <int MODE, int R>
__global__ void __launch_bounds__(NT) k_grad_shared_part(const QPDev* __restrict__ qs, const double* __restrict__ W,
                                                         int64_t sW, int64_t ldw, int nr, int rows, int B,
                                                         double* __restrict__ part) {
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
  const int r0 = blockIdx.z * R;
  int64_t roff[R];  // the group's rows within a QP's cotangents
#pragma unroll
  for (int u = 0; u < R; ++u) roff[u] = (int64_t)(r0 + u < nr ? r0 + u : r0) * ldw;
  MF::acc_t acc[R][NJ];
#pragma unroll
  for (int u = 0; u < R; ++u)
#pragma unroll
    for (int b = 0; b < NJ; ++b) acc[u][b] = MF::acc_t{0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < KCHUNK / 4; s0 += KG) {
    // a group's operands into registers first, so that its loads are in flight together, then its MFMAs: what no
    // row enters once, then row by row
    double rb[KG], xv[KG][NJ];
    const double* wz[KG];
    bool zk[KG];
#pragma unroll
    for (int s = 0; s < KG; ++s) {
      const int z = z0 + 4 * (s0 + s) + (lane >> 4);
      zk[s] = z < z1;
      const QPDev& q = qs[zk[s] ? z : z0];
      wz[s] = W + (int64_t)(zk[s] ? z : z0) * sW;
      const double* __restrict__ x = q.v[X];
      rb[s] = grad_row_rb<MODE>(q, ic);
      if (!(zk[s] && iok)) rb[s] = 0.0;
#pragma unroll
      for (int b = 0; b < NJ; ++b) {
        xv[s][b] = x[jc[b]];
        if (!(zk[s] && jok[b])) xv[s][b] = 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      // (uniform over the wave: a partial group does no more than its rows; a group's first row always exists, so
      // the single row's kernel has no branch here)
      if (u > 0 && r0 + u >= nr) break;
      double ra[KG], wv[KG][NJ];
#pragma unroll
      for (int s = 0; s < KG; ++s) {
        const double* __restrict__ w = wz[s] + roff[u];
        ra[s] = grad_row_ra<MODE>(q0, w, ic);
        if (!(zk[s] && iok)) ra[s] = 0.0;
        if (MODE != DM_Q) {
#pragma unroll
          for (int b = 0; b < NJ; ++b) {
            wv[s][b] = w[jc[b]];
            if (!(zk[s] && jok[b])) wv[s][b] = 0.0;
          }
        }
      }
#pragma unroll
      for (int s = 0; s < KG; ++s)
#pragma unroll
        for (int b = 0; b < NJ; ++b) {
          acc[u][b] = MF::mma(ra[s], xv[s][b], acc[u][b]);
          if (MODE != DM_Q) acc[u][b] = MF::mma(rb[s], wv[s][b], acc[u][b]);
        }
    }
  }
#pragma unroll
  for (int u = 0; u < R; ++u) {
    if (r0 + u >= nr) break;
    double* out = part + ((int64_t)(r0 + u) * gridDim.y + blockIdx.y) * rows * n;
#pragma unroll
    for (int b = 0; b < NJ; ++b) {
      const int j = j0 + 16 * b + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int io = i0 + MF::row(lane, r);
        if (io < rows && j < n) out[(int64_t)io * n + j] = acc[u][b][r];
      }
    }
  }
}

// second launch: dst[r tq + i ld + j] = the chunks' partials of row r summed in chunk order, for the nr rows of a
// slab (looped grid dimension)
__global__ void __launch_bounds__(NT) k_grad_shared_sum(const double* __restrict__ part, int rows, int n, int nchunk,
                                                        int nr, double* __restrict__ dst, int64_t ld, int64_t tq) {
  const int64_t per = (int64_t)rows * n;
  for (int r = blockIdx.y; r < nr; r += gridDim.y) {
    const double* __restrict__ pr = part + (int64_t)r * nchunk * per;
    double* out = dst + (int64_t)r * tq;
    for (int64_t t = blockIdx.x * (int64_t)NT + threadIdx.x; t < per; t += (int64_t)gridDim.x * NT) {
      double s = 0.0;
      for (int c = 0; c < nchunk; ++c) s += pr[c * per + t];
      out[(t / n) * ld + t % n] = s;
    }
  }
}

int64_t qp_grad_part_elems(const QPBatch& qb, int ncot) {
  const int slab = ncot < SLAB ? (ncot < 1 ? 1 : ncot) : SLAB;
  return (int64_t)((qb.B + KCHUNK - 1) / KCHUNK) * slab * update_rows(qb.h) * qb.h.n;
}

hipError_t qp_data_vjp(const QPBatch& qb, int ncot, const double* W, int64_t ldw, int64_t sW, const QpBlocksOut& o,
                       double* part, hipStream_t st) {
  const QPDev& h = qb.h;
  const int B = qb.B;
  const int dims[3] = {h.n, h.m, h.p};
  if (ncot == 1) ldw = 0;  // (one row: its stride means nothing)
  const int pairs = (int)std::min<int64_t>((int64_t)B * ncot, 1 << 30);  // block_grid's looped dimension
  // the vector blocks: the per-QP ones in one launch, the shared ones in another
  QpBlocksOut per = o, sh = o;
  bool any_per = false, any_sh = false;
  for (int w = 0; w < DB_COUNT; ++w) {
    if (!o.p[w]) continue;
    const bool shared = B > 1 && o.sq[w] == 0;
    if (!DATA_BLOCKS[w].matrix) {
      (shared ? per : sh).p[w] = nullptr;
      (shared ? any_sh : any_per) = true;
      continue;
    }
    const int rows = dims[DATA_BLOCKS[w].dim], mode = data_mode(w, h);
    const int64_t tq = ncot > 1 ? o.tq[w] : 0;
    if (shared) {  // the batch is the K dimension; the rows pass through the workspace a slab at a time
      const int nchunk = (B + KCHUNK - 1) / KCHUNK;
      const int waves = ((h.n + 16 * NJ - 1) / (16 * NJ)) * ((rows + 15) / 16);
      for (int r0 = 0; r0 < ncot; r0 += SLAB) {
        const int nr = ncot - r0 < SLAB ? ncot - r0 : SLAB;
        const double* Wr = W + (int64_t)r0 * ldw;
        with_data_mode(mode, [&](auto M) {
          constexpr int MODE = decltype(M)::value;
          const unsigned gx = (waves + NT / 64 - 1) / (NT / 64);
          if (nr == 1)  // (the single row's kernel)
            hipLaunchKernelGGL((k_grad_shared_part<MODE, 1>), dim3(gx, nchunk, 1), dim3(NT), 0, st, qb.d, Wr, sW, ldw, nr,
                               rows, B, part);
          else
            hipLaunchKernelGGL((k_grad_shared_part<MODE, RG>), dim3(gx, nchunk, (nr + RG - 1) / RG), dim3(NT), 0, st, qb.d,
                               Wr, sW, ldw, nr, rows, B, part);
        });
        hipLaunchKernelGGL(k_grad_shared_sum, block_grid((int64_t)rows * h.n, nr), dim3(NT), 0, st, part, rows, h.n,
                           nchunk, nr, o.p[w] + (int64_t)r0 * tq, o.ld[w], tq);
      }
      continue;
    }
    const int64_t sq = B > 1 ? o.sq[w] : 0;
    const dim3 grid = block_grid((int64_t)rows * 64, pairs);  // a wave per row
    const bool vec = vec16_ok(o.p[w], o.ld[w], sq) && !(tq & 1);
    with_data_mode(mode, [&](auto M) {
      constexpr int MODE = decltype(M)::value;
      if (vec)
        hipLaunchKernelGGL((k_grad_matrix<true, MODE>), grid, dim3(NT), 0, st, qb.d, W, sW, ldw, o.p[w], o.ld[w], sq, tq,
                           rows, B, ncot);
      else
        hipLaunchKernelGGL((k_grad_matrix<false, MODE>), grid, dim3(NT), 0, st, qb.d, W, sW, ldw, o.p[w], o.ld[w], sq, tq,
                           rows, B, ncot);
    });
  }
  const int mx = update_rows(h);
  if (ncot == 1)
    for (int w = 0; w < DB_COUNT; ++w) per.tq[w] = sh.tq[w] = 0;
  if (any_per) hipLaunchKernelGGL(k_grad_vectors, block_grid(mx, pairs), dim3(NT), 0, st, qb.d, W, sW, ldw, per, B, ncot);
  for (int r0 = 0; any_sh && r0 < ncot; r0 += VROWS)
    hipLaunchKernelGGL(k_grad_vectors_shared, dim3((mx + VE - 1) / VE, ncot - r0 < VROWS ? ncot - r0 : VROWS), dim3(VNT),
                       0, st, qb.d, W, sW, ldw, sh, B, r0);
  return hipGetLastError();
}

}  // namespace ipmz
