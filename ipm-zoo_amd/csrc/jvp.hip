// Forward-mode sensitivities of the residual vectors with respect to the
// problem data (ipmz_batch_data_jvp): with D_t one set of tangents of the data
// per row t < ntan, row (q, t) of R = (d r / d theta) D_t at QP q's iterate, in
// the layout of IPMZ_STATE_RES -- the right-hand side whose Newton solve
// (ipmz_*_newton_solve_multi) is the tangent of the whole Newton state.
//
// Every r_v of residual_elem (newton.hip) is affine in the data, so R is r's
// linear part in the data evaluated at the tangents.  The vector tangents enter
// one element each (vec_term, data_terms.h: the terms grad.hip transposes); the
// three matrices enter through their products with the iterate,
//
//     dQ x,   dA x,   dA^T a_dual,   dC x,   dC^T lambda_C
//
// (a_dual = lambda_A, or lambda_h - lambda_g for NaiveSlacks: data_dual, data_terms.h).
//
// Two kinds of launches, stream-ordered, no atomics, nothing waits on another
// workgroup:
//   1. one launch per matrix product into the solver's workspace (JvpPlan):
//      per-QP tangents by k_jvp_matrix (each element read once, row sums by a
//      wave reduction, column sums per lane), shared tangents (QP stride 0 in
//      a batch) by k_jvp_shared on v_mfma_f64_16x16x4 with the batch as a tile
//      dimension.
//   2. k_jvp_rows writes all state_len elements of every row exactly once: the
//      vector tangents' terms plus the products, zeros in every slot no datum
//      enters.  Per-QP and shared vector tangents differ by their QP stride
//      only, so the one launch covers both; nothing is added to R afterwards.
//
// Summation order, fixed by the shape (n, m, p) alone:
//   r_x[j] = ((dc[j] + (dQ x)[j]) + (dA^T a_dual)[j]) + (dC^T lambda_C)[j]
//   per-QP (dM x)[i]: per column tile of CT = 128 NP columns, lane l multiplies
//     its 2 NP elements (columns 128 k + 2 l, + 1, k ascending) and adds them
//     in that order, wave_sum adds the lanes; the tiles' sums are added in
//     tile order (k_jvp_rows).
//   per-QP (dM^T y)[j]: a row chunk of rch rows; wave w adds rows w, w + 4,
//     ... of the chunk in row order, the four waves' sums are added in wave
//     order, the chunks' sums in chunk order (k_jvp_rows).
//   shared: one MFMA accumulator per element over k ascending in steps of 4.
// Neither ntan nor the batch size enters any of these: row t of a call is the
// call with that tangent alone, QP q of a batch the batch of one.
//
// Loops (tests/data_jvp_cases.py lists the smallest shape reaching each):
//   k_jvp_matrix    row-pair loop of a wave: more than 8 rows in a chunk (rch
//                   16 or 32: rows * nct >= 16 * 256); row loop (q, t): batch *
//                   ntan > ROWS_GY
//   k_jvp_shared    K loop: K > KC = 32 (n > 32, or rows > 32 for the
//                   transposed products)
//   k_jvp_rows      partial loops: nct > 1 (n > 512), nchunk > 1 (rows > 8);
//                   row loop: batch * ntan > ROWS_GY; element loop: max(n, m,
//                   p) > 256 * VGX (VGX = 2048) -- out of reach
#include "common.h"
#include "data_terms.h"
#include "kernels.h"

namespace ipmz {

namespace {
constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int ROWS_GY = IPMZ_JVP_ROWS_GY;  // gridDim.y of the launches that loop over the rows (q, t)
constexpr int VGX = 2048;
constexpr int NJ = 4;  // 16-QP tiles of one wave's strip (they share the tangent operand)

__device__ __forceinline__ const double* tan_at(const double* p, int64_t sq, int64_t tq, int z, int t) {
  return p ? p + (int64_t)z * sq + (int64_t)t * tq : nullptr;
}
}  // namespace

// ---------------------------------------------------------------------------
// Launch 1, per-QP tangents: the products of one matrix block, every element
// read once.  blockIdx.x = (row chunk, column tile); a column tile is CT = 128
// NP columns, lane l on the pairs 128 k + 2 l (consecutive lanes on
// consecutive 16 bytes); a wave takes rows w, w + 4, ... of the chunk two at a
// time (both rows' loads in flight together).  Row i's partial dot with x over
// the tile -> ws row part [tile][i]; MODE != DM_Q: the chunk's column sums
// against the dual, per lane, the four waves' sums added in wave order through
// LDS -> ws column part [chunk][j].  VEC: 16-byte loads of whole pairs (the
// host checked pointer and strides, n >= 2); the last element of an odd n is
// loaded alone in both forms, and both form every sum by the same expressions:
// equal bits.  Nothing past column n of a row is read.
template <bool VEC, int MODE, int NP>
__global__ void __launch_bounds__(NT) k_jvp_matrix(const QPDev* __restrict__ qs, const double* __restrict__ T, int64_t ld,
                                                   int64_t sq, int64_t tq, int rows, int ntan, int B, JvpMat pm,
                                                   double* __restrict__ ws, int64_t seg) {
  constexpr int CT = 128 * NP;
  __shared__ double sh[NW - 1][CT];
  const QPDev& q0 = qs[0];
  const int n = q0.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ct = blockIdx.x % pm.nct, chunk = blockIdx.x / pm.nct;
  const int c0 = ct * CT + 2 * lane;
  const int i0 = chunk * pm.rch, i1 = i0 + pm.rch < rows ? i0 + pm.rch : rows;
  const int64_t total = (int64_t)B * ntan;
  for (int64_t zt = blockIdx.y; zt < total; zt += gridDim.y) {
    const int z = (int)(zt / ntan), t = (int)(zt % ntan);
    const QPDev& q = qs[z];
    const double* __restrict__ M = T + (int64_t)z * sq + (int64_t)t * tq;
    const double* __restrict__ x = q.v[X];
    double* __restrict__ w = ws + zt * seg;
    double xv[2 * NP], col[2 * NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = c0 + 128 * k;
      xv[2 * k] = c < n ? x[c] : 0.0;
      xv[2 * k + 1] = c + 1 < n ? x[c + 1] : 0.0;
      col[2 * k] = col[2 * k + 1] = 0.0;
    }
    for (int i = i0 + wave; i < i1; i += 2 * NW) {
      const bool two = i + NW < i1;  // (wave-uniform)
      const double* __restrict__ row[2] = {M + (int64_t)i * ld, M + (int64_t)(two ? i + NW : i) * ld};
      double e[2][2 * NP];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (VEC) {
          // whole pairs as 16 bytes, a masked pair from the row's head; the odd n's last element alone
          const double tail = row[u][(n & 1) ? n - 1 : 0];
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            const int c = c0 + 128 * k;
            const double2 v = *reinterpret_cast<const double2*>(row[u] + (c + 1 < n ? c : 0));
            e[u][2 * k] = c + 1 < n ? v.x : c < n ? tail : 0.0;
            e[u][2 * k + 1] = c + 1 < n ? v.y : 0.0;
          }
        } else {
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            const int c = c0 + 128 * k;
            const double a = row[u][c < n ? c : 0], b = row[u][c + 1 < n ? c + 1 : 0];
            e[u][2 * k] = c < n ? a : 0.0;
            e[u][2 * k + 1] = c + 1 < n ? b : 0.0;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (u == 1 && !two) break;
        const int iu = i + u * NW;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * NP; ++k) s += e[u][k] * xv[k];
        s = wave_sum(s);
        if (lane == 0) w[pm.off_row + (int64_t)ct * rows + iu] = s;
        if (MODE != DM_Q) {
          const double y = data_dual<MODE>(q, iu);
#pragma unroll
          for (int k = 0; k < 2 * NP; ++k) col[k] += e[u][k] * y;
        }
      }
    }
    if (MODE != DM_Q) {
      if (wave > 0) {
#pragma unroll
        for (int k = 0; k < 2 * NP; ++k) sh[wave - 1][128 * (k >> 1) + 2 * lane + (k & 1)] = col[k];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int k = 0; k < 2 * NP; ++k) {
          const int jl = 128 * (k >> 1) + 2 * lane + (k & 1), j = ct * CT + jl;
          double s = col[k];
          for (int v = 0; v < NW - 1; ++v) s += sh[v][jl];
          if (j < n) w[pm.off_col + (int64_t)chunk * n + j] = s;
        }
      }
      __syncthreads();  // (the next row (q, t) writes sh again)
    }
  }
}

// ---------------------------------------------------------------------------
// Launch 1, shared tangents (QP stride 0, batch > 1): out[t][o][q] = sum_k
// T_t(o, k) y_q[k] on v_mfma_f64_16x16x4, TRANS false: o = a row i of the
// block, k = a column, y = x (T's rows are K-major); TRANS true: o = a column
// j, k = a row, y = the dual (T's rows are M-major).  The operands are used
// where they lie: the tangent from the caller's block, y_q from each QP's own
// state through QPDev; no packed copy in memory.  A workgroup owns 64 outputs x
// 64 QPs and walks K in chunks of KC: the chunk of both operands goes through
// LDS, loaded along the direction in which it is contiguous (a QP's y and a
// K-major tangent row along k, an M-major tangent along o), element by
// element -- no alignment is assumed.  Tails in o, q and k are zeros: a masked
// element is loaded from a valid address (index 0, the strip's first QP) and
// replaced.  Wave w owns outputs 16 w .. 16 w + 15 (NJ tiles of 16 QPs sharing
// the tangent operand); the QPs are the accumulator's rows and the outputs its
// columns, so that the 16 lanes of a store write 16 consecutive doubles of one
// row (q, t) of the workspace.  One accumulator over the whole K, k ascending
// in steps of 4: nothing to add afterwards.  blockIdx.y = the tangent t.
constexpr int KC = 32, KCP = KC + 1, SB = 64;  // k per chunk, the padded LDS row, outputs and QPs per workgroup
template <int MODE, bool TRANS>
__global__ void __launch_bounds__(NT) k_jvp_shared(const QPDev* __restrict__ qs, const double* __restrict__ T, int64_t ld,
                                                   int64_t tq, int rows, int ntan, int B, double* __restrict__ ws,
                                                   int64_t seg, int64_t off) {
  typedef Mfma<double> MF;
  __shared__ double Ys[SB][KCP], Ts[SB][KCP];
  const QPDev& q0 = qs[0];
  const int n = q0.n;
  const int O = TRANS ? n : rows, K = TRANS ? rows : n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int nstrip = (B + SB - 1) / SB;
  const int ob = (blockIdx.x / nstrip) * SB, z0 = (blockIdx.x % nstrip) * SB;
  const int t = blockIdx.y;
  const double* __restrict__ M = T + (int64_t)t * tq;
  // staging along k: thread (kk, r0) takes element kk of the rows r0, r0 + 8, ... of the chunk
  const int kk = tid & (KC - 1), r0 = tid / KC;
  constexpr int NR = SB * KC / NT;  // 8 rows per thread
  const double* ya[NR];
  const double* yb[NR];  // (DM_A_NAIVE: lambda_g)
  bool zok[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int z = z0 + r0 + (NT / KC) * r;
    zok[r] = z < B;
    const QPDev& q = qs[zok[r] ? z : z0];
    ya[r] = !TRANS ? q.v[X] : MODE == DM_A ? q.v[LA] : MODE == DM_A_NAIVE ? q.v[LH] : q.v[LC];
    yb[r] = q.v[LG];
  }
  MF::acc_t acc[NJ];
#pragma unroll
  for (int b = 0; b < NJ; ++b) acc[b] = MF::acc_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += KC) {
    const bool kok = k0 + kk < K;
    const int kc = kok ? k0 + kk : 0;
    double yv[NR], tv[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      double y = ya[r][kc];
      if (TRANS && MODE == DM_A_NAIVE) y = y + (-yb[r][kc]);
      yv[r] = (kok && zok[r]) ? y : 0.0;
    }
    if (!TRANS) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int o = ob + r0 + (NT / KC) * r;
        const double v = M[(int64_t)(o < O ? o : 0) * ld + kc];
        tv[r] = (kok && o < O) ? v : 0.0;
      }
    } else {  // along o: thread (lane, wave) takes output `lane` of the rows k0 + wave, + 4, ...
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int o = ob + lane, k = k0 + wave + NW * r;
        const double v = M[(int64_t)(k < K ? k : 0) * ld + (o < O ? o : 0)];
        tv[r] = (k < K && o < O) ? v : 0.0;
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      Ys[r0 + (NT / KC) * r][kk] = yv[r];
      if (!TRANS) Ts[r0 + (NT / KC) * r][kk] = tv[r];
      else Ts[lane][wave + NW * r] = tv[r];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) {
      const double a = Ts[16 * wave + li][4 * s + g];
#pragma unroll
      for (int b = 0; b < NJ; ++b) acc[b] = MF::mma(Ys[16 * b + li][4 * s + g], a, acc[b]);
    }
    __syncthreads();
  }
  const int o = ob + 16 * wave + li;
#pragma unroll
  for (int b = 0; b < NJ; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int z = z0 + 16 * b + MF::row(lane, r);
      if (z < B && o < O) ws[((int64_t)z * ntan + t) * seg + off + o] = acc[b][r];
    }
}

// ---------------------------------------------------------------------------
// Launch 2: every element of every row (q, t) of R, exactly once -- the vector
// tangents' terms plus the products, each a sum of its partials in their
// order, added in the order Q, A, C (file header).  Element e of the n, m and p
// blocks at once (update_rows); every data term is data_terms.h's (vec_term of
// the tangent's element; the row each product enters).  r_s, r_p, the
// complementarity rows of the slacked forms and a row no given tangent enters:
// 0.  Per-QP and shared vector tangents differ by the QP stride only.
__device__ __forceinline__ double part_sum(const double* __restrict__ p, int count, int64_t stride, int idx) {
  double s = p[idx];
  for (int k = 1; k < count; ++k) s += p[(int64_t)k * stride + idx];
  return s;
}
__global__ void __launch_bounds__(NT) k_jvp_rows(const QPDev* __restrict__ qs, QpBlocksIn in, JvpPlan pl, int ntan, int B,
                                                 const double* __restrict__ ws, double* __restrict__ R, int64_t ldr,
                                                 int64_t sR) {
  const QPDev& q0 = qs[0];
  const int n = q0.n, m = q0.m, p = q0.p;
  const int mx = update_rows(q0);
  const JvpMat &mq = pl.mat[0], &ma = pl.mat[1], &mc = pl.mat[2];
  const int64_t total = (int64_t)B * ntan;
  for (int64_t zt = blockIdx.y; zt < total; zt += gridDim.y) {
    const int z = (int)(zt / ntan), t = (int)(zt % ntan);
    const QPDev& q = qs[z];
    double* __restrict__ r = R + (int64_t)z * sR + (int64_t)t * ldr;
    const double* __restrict__ w = ws + zt * pl.seg;
    const double* dc = tan_at(in.p[DB_C], in.sq[DB_C], in.tq[DB_C], z, t);
    const double* dlx = tan_at(in.p[DB_LX], in.sq[DB_LX], in.tq[DB_LX], z, t);
    const double* dux = tan_at(in.p[DB_UX], in.sq[DB_UX], in.tq[DB_UX], z, t);
    const double* dlA = tan_at(in.p[DB_LA], in.sq[DB_LA], in.tq[DB_LA], z, t);
    const double* duA = tan_at(in.p[DB_UA], in.sq[DB_UA], in.tq[DB_UA], z, t);
    const double* dd = tan_at(in.p[DB_D], in.sq[DB_D], in.tq[DB_D], z, t);
    for (int e = blockIdx.x * NT + threadIdx.x; e < mx; e += gridDim.x * NT) {
      if (e < n) {
        double s = dc ? vec_term<0>(q0, q, e, dc[e]) : 0.0;
        if (mq.mode) s = s + part_sum(w + mq.off_row, mq.nct, n, e);
        if (ma.mode) s = s + part_sum(w + ma.off_col, ma.nchunk, n, e);
        if (mc.mode) s = s + part_sum(w + mc.off_col, mc.nchunk, n, e);
        r[e] = s;
        if (q0.vlo) {
          r[slot_off(q0, LY) + e] = dlx ? vec_term<1>(q0, q, e, dlx[e]) : 0.0;
          if (!q0.slacks) r[slot_off(q0, Y) + e] = 0.0;
        }
        if (q0.vup) {
          r[slot_off(q0, LZ) + e] = dux ? vec_term<2>(q0, q, e, dux[e]) : 0.0;
          if (!q0.slacks) r[slot_off(q0, Z) + e] = 0.0;
        }
      }
      if (e < m) {
        const double ax = ma.mode ? part_sum(w + ma.off_row, ma.nct, m, e) : 0.0;
        if (!q0.naive) r[slot_off(q0, LA) + e] = ax, r[slot_off(q0, S) + e] = 0.0;  // ((A*x) - s)
        if (q0.alo) {
          const double v = dlA ? vec_term<3>(q0, q, e, dlA[e]) : 0.0;
          r[slot_off(q0, LG) + e] = (q0.naive && ma.mode) ? v + (-ax) : v;  // (l_A + g - (A*x))
          if (!q0.slacks) r[slot_off(q0, G) + e] = 0.0;
        }
        if (q0.aup) {
          const double v = duA ? vec_term<4>(q0, q, e, duA[e]) : 0.0;
          r[slot_off(q0, LH) + e] = (q0.naive && ma.mode) ? v + ax : v;  // (h + (A*x) - u_A)
          if (!q0.slacks) r[slot_off(q0, H) + e] = 0.0;
        }
      }
      if (e < p) {
        const double v = dd ? vec_term<5>(q0, q, e, dd[e]) : 0.0;  // ((C*x) ... - d)
        r[slot_off(q0, LC) + e] = mc.mode ? part_sum(w + mc.off_row, mc.nct, p, e) + v : v;
        if (!(q0.eqnone || q0.eqpen)) r[slot_off(q0, P) + e] = 0.0;
      }
    }
  }
}

// ---------------------------------------------------------------------------
int jvp_pairs(int n) { return n <= 128 ? 1 : n <= 256 ? 2 : 4; }

JvpPlan qp_jvp_plan(const QPBatch& qb, const QpBlocksIn& in) {
  const QPDev& h = qb.h;
  JvpPlan pl{};
  const int rows[DB_MATS] = {h.n, h.m, h.p};
  int64_t off = 0;
  for (int w = 0; w < DB_MATS; ++w) {
    JvpMat& mt = pl.mat[w];
    if (!in.p[w] || rows[w] == 0) continue;
    if (qb.B > 1 && in.sq[w] == 0) {
      mt.mode = 2, mt.rch = rows[w], mt.nchunk = 1, mt.nct = 1;
    } else {
      mt.mode = 1;
      const int ct = 128 * jvp_pairs(h.n);
      mt.nct = (h.n + ct - 1) / ct;
      mt.rch = 32;  // the largest chunk that still gives one (q, t) 256 workgroups, else the smallest
      while (mt.rch > 8 && (int64_t)((rows[w] + mt.rch - 1) / mt.rch) * mt.nct < 256) mt.rch /= 2;
      mt.nchunk = (rows[w] + mt.rch - 1) / mt.rch;
    }
    mt.off_row = off, off += (int64_t)mt.nct * rows[w];
    if (w) mt.off_col = off, off += (int64_t)mt.nchunk * h.n;
  }
  pl.seg = off;
  return pl;
}

template <bool VEC, int MODE>
static void launch_matrix(int np, dim3 grid, hipStream_t st, const QPDev* qs, const double* T, int64_t ld, int64_t sq,
                          int64_t tq, int rows, int ntan, int B, const JvpMat& pm, double* ws, int64_t seg) {
  if (np == 1)
    hipLaunchKernelGGL((k_jvp_matrix<VEC, MODE, 1>), grid, dim3(NT), 0, st, qs, T, ld, sq, tq, rows, ntan, B, pm, ws, seg);
  else if (np == 2)
    hipLaunchKernelGGL((k_jvp_matrix<VEC, MODE, 2>), grid, dim3(NT), 0, st, qs, T, ld, sq, tq, rows, ntan, B, pm, ws, seg);
  else
    hipLaunchKernelGGL((k_jvp_matrix<VEC, MODE, 4>), grid, dim3(NT), 0, st, qs, T, ld, sq, tq, rows, ntan, B, pm, ws, seg);
}

template <int MODE>
static void launch_shared(bool trans, dim3 grid, hipStream_t st, const QPDev* qs, const double* T, int64_t ld, int64_t tq,
                          int rows, int ntan, int B, double* ws, int64_t seg, int64_t off) {
  if (trans)
    hipLaunchKernelGGL((k_jvp_shared<MODE, true>), grid, dim3(NT), 0, st, qs, T, ld, tq, rows, ntan, B, ws, seg, off);
  else
    hipLaunchKernelGGL((k_jvp_shared<MODE, false>), grid, dim3(NT), 0, st, qs, T, ld, tq, rows, ntan, B, ws, seg, off);
}

hipError_t qp_data_jvp(const QPBatch& qb, int ntan, const QpBlocksIn& in, double* R, int64_t ldr, int64_t sR, double* ws,
                       hipStream_t st) {
  const QPDev& h = qb.h;
  const int B = qb.B;
  const JvpPlan pl = qp_jvp_plan(qb, in);
  const int64_t total = (int64_t)B * ntan;
  const unsigned gy = (unsigned)(total < ROWS_GY ? total : ROWS_GY);
  const int dims[3] = {h.n, h.m, h.p};
  for (int w = 0; w < DB_MATS; ++w) {
    const JvpMat& pm = pl.mat[w];
    if (!pm.mode) continue;
    const int rows = dims[DATA_BLOCKS[w].dim], mode = data_mode(w, h);
    if (pm.mode == 2) {  // shared: the batch is a tile dimension
      const int nstrip = (B + SB - 1) / SB;
      for (int tr = 0; tr < (w ? 2 : 1); ++tr) {
        const int ntile = ((tr ? h.n : rows) + SB - 1) / SB;
        const dim3 grid((unsigned)(ntile * nstrip), (unsigned)ntan);
        const int64_t off = tr ? pm.off_col : pm.off_row;
        with_data_mode(mode, [&](auto M) {
          launch_shared<decltype(M)::value>(tr != 0, grid, st, qb.d, in.p[w], in.ld[w], in.tq[w], rows, ntan, B, ws, pl.seg,
                                            off);
        });
      }
      continue;
    }
    const int64_t sq = B > 1 ? in.sq[w] : 0;
    const dim3 grid((unsigned)(pm.nchunk * pm.nct), gy);
    // 16-byte loads of whole pairs (a call with one tangent does not use the tangent stride)
    const bool vec = h.n >= 2 && vec16_ok(in.p[w], in.ld[w], sq) && !(ntan > 1 && (in.tq[w] & 1));
    const int np = jvp_pairs(h.n);
    with_data_mode(mode, [&](auto M) {
      constexpr int MODE = decltype(M)::value;
      if (vec) launch_matrix<true, MODE>(np, grid, st, qb.d, in.p[w], in.ld[w], sq, in.tq[w], rows, ntan, B, pm, ws, pl.seg);
      else launch_matrix<false, MODE>(np, grid, st, qb.d, in.p[w], in.ld[w], sq, in.tq[w], rows, ntan, B, pm, ws, pl.seg);
    });
  }
  int64_t gx = (update_rows(h) + NT - 1) / NT;
  gx = gx > VGX ? VGX : gx;
  hipLaunchKernelGGL(k_jvp_rows, dim3((unsigned)gx, gy), dim3(NT), 0, st, qb.d, in, pl, ntan, B, ws, R, ldr, sR);
  return hipGetLastError();
}

}  // namespace ipmz
