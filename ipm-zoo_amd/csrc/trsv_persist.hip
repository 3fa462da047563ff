// Single-launch triangular solve with the LDL^T factor:
//   x = L^{-T} D^{-1} L^{-1} b   (LinearSolvers.cpp:44-74)
// on 128-row blocks, with the one hand-off per block that the chain of
// blocks needs reduced to ONE 128 x 128 mat-vec.
//
// Block J (rows J0 .. J0+128), X_J = L_JJ^{-1}:
//   forward : y_J = X_J (b_J - sum_{K<J-1} L_JK y_K) - M_J y_{J-1},
//             M_J = X_J L_{J,J-1}
//   backward: x_J = X_J^T (y_J / D_J - sum_{K>J+1} L_KJ^T x_K) - Q_J x_{J+1},
//             Q_J = (L_{J+1,J} X_J)^T
// X_J, X_J^T, M_J and Q_J are built once per factorization by
// solve_prep_kernel (fp64 MFMA, from the factor's 64 x 64 inverses) -- the
// same two solves of every Newton step (and every refinement solve of the
// mixed-precision path) reuse them.  Everything but the M_J / Q_J product is
// computed before the previous block's vector arrives, so a hand-off costs
// one poll plus one 128-wide dot product per row: 2 * N/128 hops per solve
// instead of 2 * N/64 hops of a 64 x 64 TRSV step each.
//
// Work distribution: the forward sweep (blocks 0..nb-1) and the backward
// sweep (nb-1..0) are two launches whose workgroups dequeue tickets from a
// device counter; a ticket only waits on lower tickets, which belong to
// running workgroups, so a grid cannot deadlock.
//
// Split blocks.  A block's work may be spread over H = 2 or 4 workgroups
// ("parts", RW = 128 / H rows each), so that a hop moves 1/H of a tile
// through each CU.  Forward part h streams rows h RW .. of the tiles L_JK, of
// X_J and of M_J; X_J v needs the v slices of the parts below it (X_J is
// lower triangular), which the parts publish in a sentinel-initialised
// exchange buffer kept like the block vectors (sc1 stores, one aligned store
// per element, one round of loads stages and proves).  Backward part h owns
// columns h RW .. of block column J and rows h RW .. of X_J^T and Q_J, and
// needs the u slices of the parts above it.  Tickets: forward ticket t is
// (block t / H, part t % H), backward ticket t is (block nb-1 - t / H, part
// H-1 - t % H) -- the part nobody in its block waits for comes last.  A ticket
// then waits only for block vectors of earlier blocks and for slices of
// earlier parts of its own block: all lower tickets, drawn by workgroups that
// are running, whatever the dispatch order and however few workgroups are
// resident.  A part of a ragged last block that owns no rows publishes
// nothing and nobody waits for it.  The slices are polled in the same loop
// as the previous block's vector (they arrive together), so the split adds
// no round trip to the chain.  Every element is computed by the operations
// of the unsplit kernel in the same order -- results are bitwise those of
// H = 1.  The exchange buffers follow the discipline of the block vectors:
// the forward launch resets the u slices, the backward launch the v slices.
//
// The bulk L_JK y_K products stream the off-diagonal tiles in order, in
// pairs (512 threads x 2 x 32 elements = two 128 x 128 tiles in flight), a
// pair consumed as soon as its two block vectors are complete.  Readiness
// travels with the data: the vectors start as an all-ones bit pattern (a NaN
// payload arithmetic never produces) and are stored write-through (sc1), one
// aligned store per element (MI355X_MICROARCH.md, R2 granule), so ONE round
// of agent-scope loads both stages a vector and proves it complete.  Spins are bounded: on timeout ctrl[1]
// (SOLVE_ERR_WORD) is raised -- sticky, folded into the host's return codes.
#include "common.h"
#include "kernels.h"
#include "sync.h"

namespace ipmz {

// -DIPMZ_SOLVE_STAMPS: per forward block start / bulk done / critical wait / stored / y_{J-1} seen clocks (tools/kbench)
__device__ unsigned long long g_sstamp[2][256][6];
#ifdef IPMZ_SOLVE_STAMPS
#define SSTAMP(J, i) \
  if (tid == 0 && (J) < 256) g_sstamp[0][J][i] = __builtin_amdgcn_s_memrealtime()
#else
#define SSTAMP(J, i)
#endif
namespace {
constexpr int SB = IPMZ_SOLVE_BLOCK;  // rows per solve block
constexpr int SNT = 512;              // threads per solve workgroup (8 waves, <= 256 VGPRs)
// Register-blocked 128 x 128 tiles, 32 elements per thread (unsplit, H = 1;
// a part of a split block holds 4 / H rows resp. 4 / H columns of these):
//   row phases (L_JK y_K, X_J v, M_J y): thread (rg = t / 16, cg = t % 16)
//     holds rows 4 rg + k (k < 4), columns 2 cg + 32 j + e (j < 4, e < 2):
//     the 16 lanes of a row group read 256 contiguous bytes per load;
//   column phase (L_KJ^T x_K): thread (rg = t / 32, cg = t % 32) holds rows
//     8 rg + k (k < 8), columns 2 cg + 64 j + e (j < 2, e < 2).
constexpr int RP_ROWS = 4, RP_LANES = 16;  // row phases
constexpr int CP_ROWS = 8, CP_LANES = 32;  // column phase
constexpr int XS_LD = SB + 4;              // LDS row stride of the staged X_J
constexpr int TDS = 65;               // LDS row stride of the prep's 64 x 64 tiles
// ticket words; ctrl[SOLVE_ERR_WORD] (1) is sticky.  SC_TICKET_F2: the tickets of a forward sweep that starts
// at a later block row (the tail of a split sweep), zero after solve_reset and after every backward sweep
enum { SC_TICKET = 2, SC_TICKET_B = 3, SC_TICKET_F2 = 4 };

template <typename T>
__device__ __forceinline__ bool is_sentinel(T v);
template <>
__device__ __forceinline__ bool is_sentinel<double>(double v) {
  return __double_as_longlong(v) == (long long)-1;
}
template <>
__device__ __forceinline__ bool is_sentinel<float>(float v) {
  return __float_as_int(v) == -1;
}
template <typename T>
__device__ __forceinline__ T sentinel() {
  if constexpr (sizeof(T) == 8) return __longlong_as_double(-1ll);
  else return __int_as_float(-1);
}

// Workgroup barrier for LDS hand-offs only: unlike __syncthreads() it does not
// wait for the wave's outstanding global loads (the tile prefetches stay in
// flight across it)
__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// all-reduce over the 16 lanes of a row group (DPP quad perms, then xor 4, 8)
template <typename T>
__device__ __forceinline__ T lanes16_sum(T v) {
  v += dpp_t<0xb1>(v);
  v += dpp_t<0x4e>(v);
  v += __shfl_xor(v, 4);
  return v + __shfl_xor(v, 8);
}

// ---------------------------------------------------------------------------
// prep helpers: 64 x 64 fp64 tiles in LDS (stride TDS), 256 threads, the
// v_mfma_f64_16x16x4 layout of Mfma<double> (wave w: output rows 16w..16w+15)
// a 64 x 64 tile into registers (16 loads in flight per thread; f(r, c)
// coalesced along c), then into LDS as is or transposed
template <typename F>
__device__ __forceinline__ void fetch64(double (&v)[16], F f) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = threadIdx.x + 256 * q;
    v[q] = f(i >> 6, i & 63);
  }
}
template <bool TR>
__device__ __forceinline__ void put64(double* dst, const double (&v)[16]) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = threadIdx.x + 256 * q;
    if (TR) dst[(i & 63) * TDS + (i >> 6)] = v[q];
    else dst[(i >> 6) * TDS + (i & 63)] = v[q];
  }
}
// acc[n] += op(A)[16w.., :] B[:, 16n..], op(A) = A or A^T
template <bool TA>
__device__ __forceinline__ void mm64(double4_t (&acc)[4], const double* A, const double* B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int arow = 16 * wave + (lane & 15);
#pragma unroll 4
  for (int s = 0; s < 16; ++s) {
    const int k = 4 * s + (lane >> 4);
    const double a = TA ? A[k * TDS + arow] : A[arow * TDS + k];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = mfma_f64_16x16x4(a, B[k * TDS + 16 * n + (lane & 15)], acc[n]);
  }
}
__device__ __forceinline__ void zero4(double4_t (&acc)[4]) {
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = (double4_t){0.0, 0.0, 0.0, 0.0};
}
__device__ __forceinline__ void put4(double* dst, const double4_t (&acc)[4], double sgn) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      dst[(16 * wave + Mfma<double>::row(lane, g)) * TDS + 16 * n + (lane & 15)] = sgn * acc[n][g];
}
// acc -> 128 x 128 row-major output, quadrant (r0, c0); rows >= rmax zeroed
template <typename T>
__device__ __forceinline__ void out4(T* dst, int r0, int c0, const double4_t (&acc)[4], int rmax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int r = r0 + 16 * wave + Mfma<double>::row(lane, g);
      dst[r * SB + c0 + 16 * n + (lane & 15)] = r < rmax ? (T)acc[n][g] : T(0);
    }
}
}  // namespace

// Five workgroups per 128-row block J (blockIdx.y = part): each builds
// X_J from the two 64 x 64 inverses (X = [[Xa, 0], [-Xb L_ba Xa, Xb]]);
// part 0 stores X_J and X_J^T, parts 1-2 the column halves of M_J, parts 3-4
// those of Q_J (fp64 MFMA, stored as T).  A part's two L operands are loaded
// with the X operands.  Rows / columns past N are zero.  Block rows: J =
// jbase + blockIdx.x; X_J / M_J are built for jx0 <= J < jx1, Q_J for jq0 <=
// J < jq1 (solve_prep_split; the whole preparation: both [0, nb)).
template <typename T>
__global__ __launch_bounds__(256) void solve_prep_kernel(const T* __restrict__ K, int64_t ld, int N,
                                                         const T* __restrict__ Linv, T* __restrict__ X,
                                                         T* __restrict__ XT, T* __restrict__ M, T* __restrict__ Q,
                                                         int nb, int jbase, int jx0, int jx1, int jq0,
                                                         int jq1) {
  __shared__ double S[4][64 * TDS];  // 133 KB: Xa, Xb, X21, one L operand
  const int J = jbase + blockIdx.x, part = blockIdx.y, J0 = J * SB;
  if (part <= 2 ? (J < jx0 || J >= jx1) : (J < jq0 || J >= jq1)) return;
  if ((part == 1 || part == 2) && J == 0) return;
  if (part >= 3 && J + 1 >= nb) return;
  const int h = (part - 1) & 1;
  const int R = N - J0 < SB ? N - J0 : SB;
  const bool two = R > 64;
  double* Xa = S[0];
  double* Xb = S[1];
  double* X21 = S[2];
  double* Ls = S[3];
  auto Kat = [&](int r, int c) -> double { return (r < N && c < N) ? (double)K[(int64_t)r * ld + c] : 0.0; };
  const int64_t lb = (int64_t)2 * J * 64 * 64;  // Linv block of rows J0 .. J0+63
  double v0[16], v1[16], v2[16], va[16], vb[16];
  fetch64(v0, [&](int r, int c) { return (double)Linv[lb + r * 64 + c]; });
  fetch64(v1, [&](int r, int c) { return two ? (double)Linv[lb + 4096 + r * 64 + c] : 0.0; });
  fetch64(v2, [&](int r, int c) { return two ? Kat(J0 + 64 + r, J0 + c) : 0.0; });  // L_ba
  if (part == 1 || part == 2) {  // L_{J,J-1}, column half h: rows a, rows b
    const int C0 = J0 - SB + 64 * h;
    fetch64(va, [&](int r, int c) { return Kat(J0 + r, C0 + c); });
    fetch64(vb, [&](int r, int c) { return Kat(J0 + 64 + r, C0 + c); });
  } else if (part >= 3) {  // L_{J+1,J}, row half h: columns a, columns b (transposed into LDS)
    const int RR = J0 + SB + 64 * h;
    fetch64(va, [&](int r, int c) { return Kat(RR + r, J0 + c); });
    fetch64(vb, [&](int r, int c) { return Kat(RR + r, J0 + 64 + c); });
  }
  put64<false>(Xa, v0);
  put64<false>(Xb, v1);
  put64<false>(Ls, v2);
  __syncthreads();
  double4_t acc[4], bot[4];
  zero4(acc);
  mm64<false>(acc, Ls, Xa);  // L_ba Xa
  __syncthreads();
  put4(Ls, acc, 1.0);
  __syncthreads();
  zero4(acc);
  mm64<false>(acc, Xb, Ls);  // X21 = -Xb (L_ba Xa)
  put4(X21, acc, -1.0);
  __syncthreads();
  if (part == 0) {
    T* Xo = X + (int64_t)J * SB * SB;
    T* XTo = XT + (int64_t)J * SB * SB;
    for (int i = threadIdx.x; i < SB * SB; i += 256) {
      const int r = i >> 7, c = i & 127;
      double v = 0.0;
      if (r < R && c < R) v = r < 64 ? (c < 64 ? Xa[r * TDS + c] : 0.0)
                                     : (c < 64 ? X21[(r - 64) * TDS + c] : Xb[(r - 64) * TDS + c - 64]);
      Xo[r * SB + c] = (T)v;
      XTo[c * SB + r] = (T)v;
    }
    return;
  }
  zero4(acc);
  zero4(bot);
  if (part <= 2) {  // M_J = X_J L_{J,J-1}, column half h
    T* Mo = M + (int64_t)J * SB * SB;
    put64<false>(Ls, va);  // L_a,h
    __syncthreads();
    mm64<false>(acc, Xa, Ls);
    mm64<false>(bot, X21, Ls);
    __syncthreads();
    put64<false>(Ls, vb);  // L_b,h
    __syncthreads();
    mm64<false>(bot, Xb, Ls);
    out4(Mo, 0, 64 * h, acc, R);
    out4(Mo, 64, 64 * h, bot, R);
  } else {  // Q_J = X_J^T L_{J+1,J}^T, column half h (= row half of block J+1)
    T* Qo = Q + (int64_t)J * SB * SB;
    put64<true>(Ls, va);  // (L_{h,a})^T
    __syncthreads();
    mm64<true>(acc, Xa, Ls);
    __syncthreads();
    put64<true>(Ls, vb);  // (L_{h,b})^T
    __syncthreads();
    mm64<true>(acc, X21, Ls);
    mm64<true>(bot, Xb, Ls);
    out4(Qo, 0, 64 * h, acc, R);
    out4(Qo, 64, 64 * h, bot, R);
  }
}

// ---------------------------------------------------------------------------
// One sweep.  H = workgroups ("parts") per 128-row block, each owning RW =
// 128 / H rows (forward) or columns (backward) of the block's tiles; H = 1 is
// the unsplit form.  Every element goes through the same operations in the
// same order for every H: a row's 16 lanes hold the same columns, a column's
// 16 row groups the same 8 rows; only the rows (columns) per thread change.
template <typename T, bool BWD, int H>
__global__ __launch_bounds__(SNT) void trsv128_kernel(const T* __restrict__ K, int64_t ld, int N,
                                                      const T* __restrict__ D, const T* __restrict__ X,
                                                      const T* __restrict__ XT, const T* __restrict__ M,
                                                      const T* __restrict__ Q, T* b, T* ybuf, T* xbuf,
                                                      unsigned* ctrl, int nb, const unsigned* __restrict__ skip,
                                                      int inject, int nbv, int jfirst) {
  typedef typename Mfma<T>::vec2_t V2;
  constexpr int RW = SB / H;        // rows / columns a part owns
  constexpr int RPR = RP_ROWS / H;  // row phases: rows per thread
  constexpr int CPT = 4 / H;        // column phase: columns per thread
  constexpr int TE = 8 * RPR;       // elements of a register tile (= CP_ROWS * CPT)
  static_assert(H == 1 || H == 2 || H == 4, "parts per block");
  typedef T Tile[TE];  // [k][j][e] (row phases, k < RPR) / [k][i] (column phase, k < 8, i < CPT)
  if (skip && *skip) return;  // mixed-precision refinement already converged
  __shared__ T vs[2][SB];     // staged block vectors (bulk), then the critical vector
  __shared__ T red[SB / CP_ROWS][RW];
  __shared__ T vec[SB], bj[RW];
  // the part's rows of X_J (forward) / X_J^T (backward), staged at the start
  // of the ticket so the row phase after the bulk reads LDS, not HBM (stride
  // padded: the row groups of a wave hit different banks)
  __shared__ __attribute__((aligned(16))) T xs[RW * XS_LD];
  __shared__ unsigned sh_ticket, sh_stop, sh_nr[2];
  unsigned* err = ctrl + SOLVE_ERR_WORD;
  // the parts' exchange vectors (v slices forward, u slices backward) follow
  // the block vectors in the same ranges (nbv block rows: those of the whole
  // system, also when this sweep covers its leading nb only)
  T* const vbuf = ybuf + (int64_t)nbv * SB;
  T* const ubuf = xbuf + (int64_t)nbv * SB;
  const int tid = threadIdx.x;
  const int rg = tid / RP_LANES, cg = tid % RP_LANES;  // row phases
  if (tid == 0) sh_nr[0] = sh_nr[1] = 0u;

  // uniform: stage up to two vectors (c0 entries at p0 into d0 by threads
  // 0..127, c1 at p1 into d1 by threads 128..255; p1 may be null), polled
  // until all are complete (no sentinel left); entries c .. f-1 of a
  // destination are zeroed.  false: gave up -- after SPIN_TICKS, or when
  // another workgroup raised err (read every 32nd round, so a poll round is
  // one load latency)
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  auto stage2 = [&](const T* p0, int c0, int f0, T* d0, const T* p1, int c1, int f1, T* d1) -> bool {
    for (unsigned it = 1;; ++it) {
      lds_sync();  // earlier reads of vs / vec / sh_nr / sh_stop are done
      const int bsel = tid / SB, e = tid % SB;
      if (tid == 0) sh_nr[(it + 1) & 1] = 0u;  // the next round's flag
      const T* const p = bsel ? p1 : p0;
      if (bsel < 2 && p) {
        const int cnt = bsel ? c1 : c0, nfill = bsel ? f1 : f0;
        T* const d = bsel ? d1 : d0;
        const T v = e < cnt ? ld_sc1(&p[e]) : T(0);
        if (e < cnt && is_sentinel(v)) sh_nr[it & 1] = 1u;
        if (e < cnt || e < nfill) d[e] = v;
      }
      if (tid == 0)
        sh_stop = __builtin_amdgcn_s_memrealtime() - t_start > SPIN_TICKS || ((it & 31u) == 0u && ld_sc1(err) != 0u);
      lds_sync();
      if (!sh_nr[it & 1]) return true;
      if (sh_stop) {
        if (tid == 0) st_sc1(err, 1u);
        return false;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  };
  // block vectors kb0, kb0 + dir (nk <= 2 of them) of buf into vs
  auto stage = [&](const T* buf, int kb0, int nk, int dir) -> bool {
    const int kb1 = kb0 + dir;
    const int n0 = N - kb0 * SB < SB ? N - kb0 * SB : SB;
    const int n1 = N - kb1 * SB < SB ? N - kb1 * SB : SB;
    return stage2(buf + (int64_t)kb0 * SB, n0, SB, vs[0], nk > 1 ? buf + (int64_t)kb1 * SB : nullptr, n1, SB, vs[1]);
  };
  // row phases: RW rows of a 128-column row-major tile (row stride SB) at p
  // into t (one base address per thread, immediate offsets)
  auto load_rows = [&](Tile& t, const T* p) {
    const T* q = p + RPR * rg * SB + 2 * cg;
#pragma unroll
    for (int k = 0; k < RPR; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const V2 v2 = *reinterpret_cast<const V2*>(q + k * SB + 32 * j);
        t[8 * k + 2 * j] = v2.x;
        t[8 * k + 2 * j + 1] = v2.y;
      }
  };
  auto put_xs = [&](const Tile& t) {
#pragma unroll
    for (int k = 0; k < RPR; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<V2*>(&xs[(RPR * rg + k) * XS_LD + 2 * cg + 32 * j]) = V2{t[8 * k + 2 * j], t[8 * k + 2 * j + 1]};
  };
  // acc[k] += xs[row k, :] . v[columns of this thread]
  auto dot_xs = [&](T (&acc)[RPR], const T* v) {
    T vv[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const V2 v2 = *reinterpret_cast<const V2*>(v + 2 * cg + 32 * j);
      vv[2 * j] = v2.x;
      vv[2 * j + 1] = v2.y;
    }
#pragma unroll
    for (int k = 0; k < RPR; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const V2 x2 = *reinterpret_cast<const V2*>(&xs[(RPR * rg + k) * XS_LD + 2 * cg + 32 * j]);
        acc[k] = fma(x2.x, vv[2 * j], acc[k]);
        acc[k] = fma(x2.y, vv[2 * j + 1], acc[k]);
      }
  };
  // acc[k] += t[k, :] . v[columns of this thread]
  auto dot_rows = [&](T (&acc)[RPR], const Tile& t, const T* v) {
    T vv[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const V2 v2 = *reinterpret_cast<const V2*>(v + 2 * cg + 32 * j);
      vv[2 * j] = v2.x;
      vv[2 * j + 1] = v2.y;
    }
#pragma unroll
    for (int k = 0; k < RPR; ++k)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[k] = fma(t[8 * k + i], vv[i], acc[k]);
  };

  for (;;) {
    lds_sync();
    // (a forward sweep from block row jfirst > 0 on: its own counter, tickets
    // from that block's first; the rows before it are complete -- stream order)
    if (tid == 0) sh_ticket = atomicAdd(&ctrl[BWD ? SC_TICKET_B : jfirst ? SC_TICKET_F2 : SC_TICKET], 1u);
    lds_sync();
    const int ticket = (int)sh_ticket + (BWD ? 0 : jfirst * H);
    if (ticket >= nb * H) return;
    // the other sweep's ticket counter, for the next launch of that sweep
    // (the previous one has completed: stream order)
    if (ticket == 0 && tid == 0) {
      st_sc1(&ctrl[BWD ? SC_TICKET : SC_TICKET_B], 0u);
      if (BWD) st_sc1(&ctrl[SC_TICKET_F2], 0u);
    }

    if constexpr (!BWD) {
      // ============================================================ forward
      const int J = ticket / H, h = ticket % H, J0 = J * SB, r0 = h * RW;
      const int R = N - J0 < SB ? N - J0 : SB;
      const int Rh = R - r0 < RW ? R - r0 : RW;  // rows of this part
      if (Rh <= 0) continue;                     // ragged last block: nothing to own, nobody waits for it
#ifdef IPMZ_SOLVE_STAMPS
      const bool stamp = h == H - 1 || Rh < RW || R == r0 + RW;  // the block's last part
#define SSTAMPH(J, i) \
  if (stamp) SSTAMP(J, i)
#else
#define SSTAMPH(J, i)
#endif
      SSTAMPH(J, 0);
      if (tid < Rh) {  // for this solve's backward launch
        st_sc1(&xbuf[J0 + r0 + tid], sentinel<T>());
        if (H > 1) st_sc1(&ubuf[J0 + r0 + tid], sentinel<T>());
      }
      // rows past N read the part's first row (finite data): their sums are never used
      const T* Lrow = K + (int64_t)(J0 + r0) * ld;
      const int64_t ldr = ld;
      auto row_ok = [&](int k) { return RPR * rg + k < Rh; };
      T acc[RPR];
#pragma unroll
      for (int k = 0; k < RPR; ++k) acc[k] = T(0);
      Tile ta, tb;  // the next two tiles in flight
      // the part's rows of X_J and b_J -> LDS up front
      load_rows(ta, X + (int64_t)J * SB * SB + r0 * SB);
      if (tid < RW) bj[tid] = tid < Rh ? b[J0 + r0 + tid] : T(0);
      put_xs(ta);
      auto load_tile = [&](Tile& t, int Kb) {
    #pragma unroll
        for (int k = 0; k < RPR; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int64_t row = row_ok(k) ? RPR * rg + k : 0;
            const V2 v2 = *reinterpret_cast<const V2*>(Lrow + row * ldr + (int64_t)Kb * SB + 2 * cg + 32 * j);
            t[8 * k + 2 * j] = v2.x;
            t[8 * k + 2 * j + 1] = v2.y;
          }
      };
      // bulk: K < J-1.  Tiles K < J-2 in pairs as their vectors complete, the
      // next pair in flight; the last one, L_{J,J-2}, alone, so that M_J is
      // loaded into the other register tile as soon as y_{J-3} has been
      // consumed -- two hops before the hand-off needs it (loaded after the
      // bulk, its reload sat on the chain: DESIGN.md §4, the solve)
      const int Kp = J - 2;  // pairs region [0, Kp)
      const T* Mj = M + (int64_t)J * SB * SB + r0 * SB;
      if (Kp > 0) {
        load_tile(ta, 0);
        if (Kp > 1) load_tile(tb, 1);
        else load_rows(tb, Mj);
      } else if (J >= 1) {
        if (J == 2) load_tile(ta, 0);
        load_rows(tb, Mj);
      }
      for (int Kc = 0; Kc < Kp; Kc += 2) {
        const bool two = Kc + 1 < Kp;
        if (!stage(ybuf, Kc, two ? 2 : 1, 1)) return;
        dot_rows(acc, ta, vs[0]);
        if (two) dot_rows(acc, tb, vs[1]);
        load_tile(ta, Kc + 2 < Kp ? Kc + 2 : J - 2);
        if (two) {  // tb consumed: the next pair's second tile, or M_J
          if (Kc + 3 < Kp) load_tile(tb, Kc + 3);
          else load_rows(tb, Mj);
        }
      }
      if (J >= 2) {  // L_{J,J-2} y_{J-2}
        if (!stage(ybuf, J - 2, 1, 1)) return;
        dot_rows(acc, ta, vs[0]);
      }
      SSTAMPH(J, 1);
#pragma unroll
      for (int k = 0; k < RPR; ++k) acc[k] = lanes16_sum(acc[k]);
      lds_sync();  // vec / vs reuse; xs, bj staged
      // v = b_J - sum_{K<J-1} L_JK y_K: this part's slice, published for the
      // parts above it (X_J is lower triangular: they need it, it needs
      // theirs not); the slices above count as zero
      if (cg == 0) {
#pragma unroll
        for (int k = 0; k < RPR; ++k) {
          const int rr = RPR * rg + k;
          const T v = bj[rr] - acc[k];
          vec[r0 + rr] = v;
          if (H > 1 && h < H - 1 && rr < Rh) st_sc1(&vbuf[J0 + r0 + rr], v);
        }
      }
      if (H > 1 && tid < SB && tid >= r0 + RW) vec[tid] = T(0);
      // the slices below (complete parts: this one has rows) are polled
      // together with y_{J-1}: the two arrive about together (block J-1
      // publishes 0.2 us after it sees y_{J-2}, the siblings their slices
      // after the same y_{J-2}), and one poll loop for both is one global
      // round trip less on the chain than one after the other
      const bool both = H > 1 && h > 0 && J > 0;
      if (H > 1 && h > 0) {
        SSTAMPH(J, 2);
        if (!stage2(vbuf + J0, r0, 0, vec, both ? ybuf + (int64_t)(J - 1) * SB : nullptr, SB, SB, vs[0])) return;
        SSTAMPH(J, 5);
      } else {
        lds_sync();
      }
      T y[RPR];
#pragma unroll
      for (int k = 0; k < RPR; ++k) y[k] = T(0);
      dot_xs(y, vec);  // X_J v
      if (J > 0) {     // the hand-off: y_J = X_J v - M_J y_{J-1}
        if (!both) {
          SSTAMPH(J, 2);
          if (!stage(ybuf, J - 1, 1, 1)) return;
        }
        SSTAMPH(J, 4);
        T d[RPR];
#pragma unroll
        for (int k = 0; k < RPR; ++k) d[k] = T(0);
        dot_rows(d, tb, vs[0]);
#pragma unroll
        for (int k = 0; k < RPR; ++k) y[k] -= d[k];
      }
      // inject (tests only): no part of block 0 publishes -> every consumer times out
#pragma unroll
      for (int k = 0; k < RPR; ++k) {
        const T yk = lanes16_sum(y[k]);
        const int rr = RPR * rg + k;
        if (cg == 0 && rr < Rh && !(inject && J == 0)) st_sc1(&ybuf[J0 + r0 + rr], yk);
      }
      SSTAMPH(J, 3);
#undef SSTAMPH
    } else {
      // =========================================================== backward
      // the part with the highest columns draws the lowest ticket: X_J^T is
      // upper triangular, so a part needs the u slices of the parts above it
      const int J = nb - 1 - ticket / H, h = H - 1 - ticket % H, J0 = J * SB, c0 = h * RW;
      const int R = N - J0 < SB ? N - J0 : SB;
      const int Rh = R - c0 < RW ? R - c0 : RW;  // columns (= rows of x_J) of this part
      if (Rh <= 0) continue;                     // ragged last block: nothing to own, nobody waits for it
      const bool last = J + 1 >= nb;
      // bulk: column phase; columns past the block's R give sums that are
      // never used; rows past N (ragged last block) are not read and meet
      // zero vector entries
      const int crg = tid / CP_LANES, ccg = tid % CP_LANES;
      auto col = [&](int i) { return CPT == 4 ? 2 * ccg + 64 * (i >> 1) + (i & 1) : CPT == 2 ? 2 * ccg + i : ccg; };
      const bool ragged = N % SB != 0;
      T acc[CPT];  // columns col(i) of the part
#pragma unroll
      for (int i = 0; i < CPT; ++i) acc[i] = T(0);
      Tile ta, tb;
      // the part's rows of X_J^T and of z_J = y_J / D_J -> LDS up front (y_J
      // from the forward launch: complete)
      load_rows(ta, XT + (int64_t)J * SB * SB + c0 * SB);
      if (tid < RW) bj[tid] = tid < Rh ? ybuf[J0 + c0 + tid] / D[J0 + c0 + tid] : T(0);
      if (tid < Rh) {  // only this part reads its y_J rows: reset for the next solve
        st_sc1(&ybuf[J0 + c0 + tid], sentinel<T>());
        if (H > 1) st_sc1(&vbuf[J0 + c0 + tid], sentinel<T>());
      }
      put_xs(ta);
      auto load_tile = [&](Tile& t, int Kb) {
            const int R0 = Kb * SB + CP_ROWS * crg;
        const T* p = K + (int64_t)R0 * ld + J0 + c0 + (CPT > 1 ? 2 * ccg : ccg);
        const bool rag = ragged && Kb == nb - 1;
#pragma unroll
        for (int k = 0; k < CP_ROWS; ++k) {
          const bool in = !rag || R0 + k < N;
          if constexpr (CPT > 1) {
#pragma unroll
            for (int j = 0; j < CPT / 2; ++j) {
              const V2 v2 = in ? *reinterpret_cast<const V2*>(p + (int64_t)k * ld + 64 * j) : V2{T(0), T(0)};
              t[CPT * k + 2 * j] = v2.x;
              t[CPT * k + 2 * j + 1] = v2.y;
            }
          } else {
            t[k] = in ? p[(int64_t)k * ld] : T(0);
          }
        }
      };
      auto dot_cols = [&](const Tile& t, const T* v) {
            T xv[CP_ROWS];
#pragma unroll
        for (int k = 0; k < CP_ROWS; k += 2) {
          const V2 v2 = *reinterpret_cast<const V2*>(v + CP_ROWS * crg + k);
          xv[k] = v2.x;
          xv[k + 1] = v2.y;
        }
#pragma unroll
        for (int k = 0; k < CP_ROWS; ++k)
#pragma unroll
          for (int i = 0; i < CPT; ++i) acc[i] = fma(t[CPT * k + i], xv[k], acc[i]);
      };
      // bulk: K > J+1 from the bottom.  Tiles K > J+2 in pairs as their
      // vectors complete; the last one, block J+2, alone, so that Q_J is
      // loaded into the other register tile as soon as x_{J+3} has been
      // consumed (the forward sweep's M_J schedule, mirrored)
      const int Klo = J + 3;  // pairs region [Klo, nb)
      const T* Qj = Q + (int64_t)J * SB * SB + c0 * SB;
      if (nb - 1 >= Klo) {
        load_tile(ta, nb - 1);
        if (nb - 2 >= Klo) load_tile(tb, nb - 2);
        else load_rows(tb, Qj);
      } else if (!last) {
        if (J + 2 <= nb - 1) load_tile(ta, J + 2);
        load_rows(tb, Qj);
      }
      for (int Kc = nb - 1; Kc >= Klo; Kc -= 2) {
        const bool two = Kc - 1 >= Klo;
        if (!stage(xbuf, Kc, two ? 2 : 1, -1)) return;
        dot_cols(ta, vs[0]);
        if (two) dot_cols(tb, vs[1]);
        load_tile(ta, Kc - 2 >= Klo ? Kc - 2 : J + 2);
        if (two) {  // tb consumed: the next pair's second tile, or Q_J
          if (Kc - 3 >= Klo) load_tile(tb, Kc - 3);
          else load_rows(tb, Qj);
        }
      }
      if (J + 2 <= nb - 1) {  // L_{J+2,J}^T x_{J+2}
        if (!stage(xbuf, J + 2, 1, 1)) return;
        dot_cols(ta, vs[0]);
      }
      lds_sync();
#pragma unroll
      for (int i = 0; i < CPT; ++i) red[crg][col(i)] = acc[i];
      lds_sync();
      // u = z_J - sum L_KJ^T x_K (zero past R): this part's slice, published
      // for the parts below it; the slices below count as zero
      if (tid < RW) {
        T t = T(0);
#pragma unroll
        for (int k = 0; k < SB / CP_ROWS; ++k) t += red[k][tid];
        const T u = bj[tid] - t;
        vec[c0 + tid] = u;
        if (H > 1 && h > 0 && tid < Rh) st_sc1(&ubuf[J0 + c0 + tid], u);
      }
      if (H > 1 && tid < c0) vec[tid] = T(0);
      // the slices above, as far as the block has rows, polled together
      // with x_{J+1} (the forward sweep's joint poll, mirrored)
      const bool both = H > 1 && h < H - 1 && !last;
      if (H > 1 && h < H - 1) {
        const int up = c0 + RW;
        const int n1 = N - (J + 1) * SB < SB ? N - (J + 1) * SB : SB;
        if (!stage2(ubuf + J0 + up, R - up, SB - up, vec + up, both ? xbuf + (int64_t)(J + 1) * SB : nullptr, n1, SB,
                    vs[0]))
          return;
      } else {
        lds_sync();
      }
      T x[RPR];
#pragma unroll
      for (int k = 0; k < RPR; ++k) x[k] = T(0);
      dot_xs(x, vec);  // X_J^T u
      if (!last) {     // the hand-off: x_J = X_J^T u - Q_J x_{J+1}
        if (!both && !stage(xbuf, J + 1, 1, 1)) return;
        T d[RPR];
#pragma unroll
        for (int k = 0; k < RPR; ++k) d[k] = T(0);
        dot_rows(d, tb, vs[0]);
#pragma unroll
        for (int k = 0; k < RPR; ++k) x[k] -= d[k];
      }
#pragma unroll
      for (int k = 0; k < RPR; ++k) {
        const T xk = lanes16_sum(x[k]);
        const int rr = RPR * rg + k;
        if (cg == 0 && rr < Rh) {
          st_sc1(&xbuf[J0 + c0 + rr], xk);
          b[J0 + c0 + rr] = xk;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
int64_t solve_prep_elems(int N) {
  const int64_t nb = (N + SB - 1) / SB;
  return 4 * nb * SB * SB;
}

// block rows [jx0, jx1) of X / M and [jq0, jq1) of Q
template <typename T>
static hipError_t solve_prep_t(const T* K, int64_t ld, int N, const T* Linv, T* P, hipStream_t st, int jx0 = 0,
                               int jx1 = 1 << 30, int jq0 = 0, int jq1 = 1 << 30) {
  if (N <= 0) return hipSuccess;
  const int nb = (N + SB - 1) / SB;
  const int64_t q = (int64_t)nb * SB * SB;
  jx1 = jx1 < nb ? jx1 : nb;
  jq1 = jq1 < nb ? jq1 : nb;
  const int lo = jx0 < jq0 ? jx0 : jq0, hi = jx1 > jq1 ? jx1 : jq1;
  if (hi <= lo) return hipSuccess;
  hipLaunchKernelGGL(solve_prep_kernel<T>, dim3(hi - lo, 5), dim3(256), 0, st, K, ld, N, Linv, P, P + q, P + 2 * q,
                     P + 3 * q, nb, lo, jx0, jx1, jq0, jq1);
  return hipGetLastError();
}
hipError_t solve_prep_split(const double* K, int64_t ld, int N, const double* Linv, double* P, int R, bool head,
                            hipStream_t st) {
  if (R <= 0 || R >= N || R % SB) return hipErrorInvalidValue;
  const int j = R / SB;  // Q_{j-1} reads L_{j,j-1}: rows >= R
  return head ? solve_prep_t<double>(K, ld, N, Linv, P, st, 0, j, 0, j - 1)
              : solve_prep_t<double>(K, ld, N, Linv, P, st, j, 1 << 30, j - 1, 1 << 30);
}
hipError_t solve_stamps(unsigned long long* out) {  // DEBUG
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sstamp), sizeof(unsigned long long) * 2 * 256 * 6);
}
hipError_t solve_prep(const double* K, int64_t ld, int N, const double* Linv, double* P, hipStream_t st) {
  return solve_prep_t<double>(K, ld, N, Linv, P, st);
}
hipError_t solve_prep(const float* K, int64_t ld, int N, const float* Linv, float* P, hipStream_t st) {
  return solve_prep_t<float>(K, ld, N, Linv, P, st);
}

int64_t solve_vec_elems(int N) {
  const int64_t nb = (N + SB - 1) / SB;
  return 2 * nb * SB;
}

// Parts per block (H).  Debug bits force 2 or 4 (both: 1); otherwise from the measured
// solves of profiles/solve_split/solve_hops.txt (the solve),
// which rank the same in fp64 and fp32: one block has nothing to split; H = 4
// is fastest at N = 640 .. 11264 (0.377 against 0.520 ms per fp64 solve at
// N = 11264), H = 2 at N = 16384 (0.626 against 0.655 for H = 4 and 0.783
// unsplit), where four parts per block no longer find a CU each
template <typename T>
static int solve_parts(int N) {
  const int dbg = debug_inject_mask();
  if ((dbg & IPMZ_DEBUG_SOLVE_H2) && (dbg & IPMZ_DEBUG_SOLVE_H4)) return 1;
  if (dbg & IPMZ_DEBUG_SOLVE_H4) return 4;
  if (dbg & IPMZ_DEBUG_SOLVE_H2) return 2;
  if (N <= SB) return 1;
  return N <= 12288 ? 4 : 2;
}

// a forward sweep's range of block rows: the leading `lead` rows only (a
// multiple of 128, < N; 0 = all), or from block row `first` on
struct SweepRange {
  int lead = 0, first = 0;
};
// one sweep's launch.  No workgroup waits for one that has not started (the
// tickets), so the grid is only capped by what could be resident: 256 CUs, a
// part's LDS (mostly its RW rows of X_J) and its threads of the CU's 2048
template <typename T, bool BWD, int H>
static hipError_t launch_sweep(const T* K, int64_t ld, int N, const T* D, const T* P, T* b, T* ybuf, T* xbuf,
                               unsigned* ctrl, hipStream_t st, const unsigned* skip, const SweepRange& sr) {
  // (a forward sweep over the leading rows only: N and nb are those rows',
  // the operators and the exchange vectors lie as the whole system's do)
  const int nb = ((sr.lead ? sr.lead : N) + SB - 1) / SB, nbv = (N + SB - 1) / SB;
  const int64_t q = (int64_t)nbv * SB * SB;
  if (sr.lead) N = sr.lead;
  constexpr int RW = SB / H;
  constexpr int64_t lds = (int64_t)sizeof(T) * (RW * XS_LD + (SB / CP_ROWS) * RW + 3 * SB + RW) + 64;
  constexpr int by_threads = 2048 / SNT;
  constexpr int per_cu = 160 * 1024 / lds < by_threads ? (int)(160 * 1024 / lds) : by_threads;
  static_assert(per_cu >= 1, "a part's LDS fits a CU");
  const int tickets = (nb - sr.first) * H, cap = 256 * per_cu;
  const int grid = tickets < cap ? tickets : cap;
  const int inject = debug_inject_mask() & IPMZ_INJECT_SOLVE;
  hipLaunchKernelGGL((trsv128_kernel<T, BWD, H>), dim3(grid), dim3(SNT), 0, st, K, ld, N, D, P, P + q, P + 2 * q,
                     P + 3 * q, b, ybuf, xbuf, ctrl, nb, skip, inject, nbv, sr.first);
  return hipGetLastError();
}
template <typename T, bool BWD>
static hipError_t sweep_t(const T* K, int64_t ld, int N, const T* D, const T* P, T* b, T* ybuf, T* xbuf,
                          unsigned* ctrl, hipStream_t st, const unsigned* skip, const SweepRange& sr = SweepRange()) {
  if (N <= 0) return hipSuccess;
  if (ld % 2) return hipErrorInvalidValue;  // 2-element vector loads of the tiles
  if (BWD && (sr.lead || sr.first)) return hipErrorInvalidValue;
  if (sr.lead % SB || sr.lead >= N || (sr.lead && sr.first) || sr.first * SB >= N) return hipErrorInvalidValue;
  switch (solve_parts<T>(N)) {  // of the whole system, whatever the range
    case 4: return launch_sweep<T, BWD, 4>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, skip, sr);
    case 2: return launch_sweep<T, BWD, 2>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, skip, sr);
    default: return launch_sweep<T, BWD, 1>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, skip, sr);
  }
}

// no per-solve memsets: each launch leaves the state the next one needs (the
// forward resets x, the u slices and the backward ticket, the backward resets
// y, the v slices and the forward ticket); solve_reset establishes it after a
// factorization.  The two sweeps are two launches (each its own register
// allocation) of the same H.  An unsplit solve neither writes nor resets the
// slices, so solves of different H may follow each other on one factor.
template <typename T>
static hipError_t solve_persistent_t(const T* K, int64_t ld, int N, const T* D, const T* P, T* b, T* ybuf, T* xbuf,
                                     unsigned* ctrl, hipStream_t st, const unsigned* skip) {
  const hipError_t e = sweep_t<T, false>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, skip);
  if (e != hipSuccess) return e;
  return sweep_t<T, true>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, skip);
}

hipError_t ldlt_solve_persistent_head(const double* K, int64_t ld, int N, const double* D, const double* P,
                                      const double* b, double* ybuf, double* xbuf, unsigned* ctrl, int R,
                                      hipStream_t st) {
  if (R <= 0) return hipErrorInvalidValue;
  // (the forward sweep only reads b)
  return sweep_t<double, false>(K, ld, N, D, P, const_cast<double*>(b), ybuf, xbuf, ctrl, st, nullptr,
                                SweepRange{R, 0});
}
hipError_t ldlt_solve_persistent_tail(const double* K, int64_t ld, int N, const double* D, const double* P, double* b,
                                      double* ybuf, double* xbuf, unsigned* ctrl, int R, hipStream_t st) {
  if (R <= 0 || R % SB) return hipErrorInvalidValue;
  const hipError_t e = sweep_t<double, false>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, nullptr, SweepRange{0, R / SB});
  if (e != hipSuccess) return e;
  return sweep_t<double, true>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, nullptr);
}

// one sweep of the persistent solve (forward: y = L^{-1} b into ybuf;
// backward: b = L^{-T} (ybuf / D)) -- the Bunch-Kaufman solve applies its
// block-diagonal D between the two (bk_fast_dsolve on ybuf, D = ones here)
hipError_t ldlt_solve_persistent_sweep(const double* K, int64_t ld, int N, const double* D, const double* P,
                                       double* b, double* ybuf, double* xbuf, unsigned* ctrl, bool backward,
                                       hipStream_t st, const unsigned* skip) {
  return backward ? sweep_t<double, true>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, skip)
                  : sweep_t<double, false>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, skip);
}

namespace {
// up to 6 word ranges, each filled with its own value: one launch for what
// would be one memset (and one launch gap) each
struct FillJob {
  unsigned* p[6];
  int64_t n[6];
  unsigned v[6];
};
__global__ __launch_bounds__(256) void fill_words_kernel(FillJob f) {
  const int r = blockIdx.y;
  unsigned* const p = f.p[r];
  const unsigned v = f.v[r];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < f.n[r]; i += (int64_t)gridDim.x * 256) p[i] = v;
}
}  // namespace

hipError_t solve_reset(void* ybuf, void* xbuf, size_t elem, int N, unsigned* ctrl, hipStream_t st, int* info,
                       unsigned* words, int64_t nwords, int* info2) {
  FillJob f{};
  int cnt = 0;
  int64_t most = 0;
  auto add = [&](void* p, int64_t n, unsigned v) {
    if (!p || n <= 0) return;
    f.p[cnt] = static_cast<unsigned*>(p);
    f.n[cnt] = n;
    f.v[cnt++] = v;
    most = n > most ? n : most;
  };
  add(ctrl, IPMZ_SOLVE_CTRL_WORDS, 0u);  // tickets + sticky error
  add(ybuf, solve_vec_elems(N) * (int64_t)elem / 4, ~0u);  // block vectors + the parts' slices
  add(xbuf, solve_vec_elems(N) * (int64_t)elem / 4, ~0u);
  add(info, 1, 0x7f7f7f7fu);  // "no pivot failed" (the byte pattern of hipMemset 0x7f)
  add(info2, 1, 0x7f7f7f7fu);
  add(words, nwords, 0u);
  if (!cnt) return hipSuccess;
  const int64_t gx = (most + 255) / 256;
  hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)(gx < 64 ? gx : 64), cnt), dim3(256), 0, st, f);
  return hipGetLastError();
}

hipError_t ldlt_solve_persistent(const double* K, int64_t ld, int N, const double* D, const double* P, double* b,
                                 double* ybuf, double* xbuf, unsigned* ctrl, hipStream_t st) {
  return solve_persistent_t<double>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, nullptr);
}
hipError_t ldlt_solve_persistent(const float* K, int64_t ld, int N, const float* D, const float* P, float* b,
                                 float* ybuf, float* xbuf, unsigned* ctrl, hipStream_t st, const unsigned* skip) {
  return solve_persistent_t<float>(K, ld, N, D, P, b, ybuf, xbuf, ctrl, st, skip);
}

}  // namespace ipmz
