// How the problem data enter the residual vectors, stated once for the gradient (grad.hip: the transposed map),
// the tangents (jvp.hip: the map itself) and the step (newton.hip: the dual A^T multiplies), with the launch helpers
// the data calls share (io.hip too).
//
// Every r_v of residual_elem (newton.hip) is affine in the data.  The six vectors enter one element each: vec_term
// below.  The three matrices enter through their products with the iterate:
//   Q  r_x has + (Q*x)
//   A  r_x has + (A^T*a), a = data_dual: lambda_A, or (lambda_h - lambda_g) for NaiveSlacks; the row (A*x) enters is
//      r_lambda_A = ((A*x) - s), or for NaiveSlacks r_lambda_g = (l_A + g - (A*x)) and r_lambda_h = (h + (A*x) - u_A)
//   C  r_x has + (C^T*lambda_C); r_lambda_C has + (C*x) in all three equality handlings
// NaiveSlacks' -+(A*x) is the one pairing stated twice: grad_row_factors' ra = w_lambda_h + (-w_lambda_g) is the
// transpose of k_jvp_rows adding -(dA x) to r_lambda_g and +(dA x) to r_lambda_h.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace ipmz {

// A matrix block's term, a template argument of its kernels
enum DataMode { DM_Q = 0, DM_A, DM_A_NAIVE, DM_C };
inline int data_mode(int block, const QPDev& h) {  // block: DB_Q, DB_A, DB_CEQ
  return block == DB_Q ? DM_Q : block == DB_CEQ ? DM_C : h.naive ? DM_A_NAIVE : DM_A;
}
// f(std::integral_constant<int, mode>): the run-time mode as a template argument (decltype(M)::value)
template <class F>
inline void with_data_mode(int mode, F&& f) {
  if (mode == DM_Q) f(std::integral_constant<int, DM_Q>{});
  else if (mode == DM_A) f(std::integral_constant<int, DM_A>{});
  else if (mode == DM_A_NAIVE) f(std::integral_constant<int, DM_A_NAIVE>{});
  else f(std::integral_constant<int, DM_C>{});
}

// element i of the vector the transposed product multiplies in r_x ("(A^T * (lambda_h - lambda_g))",
// formulations.txt)
template <int MODE>
__device__ __forceinline__ double data_dual(const QPDev& q, int i) {
  if (MODE == DM_A) return q.v[LA][i];
  if (MODE == DM_A_NAIVE) return q.v[LH][i] + (-q.v[LG][i]);
  return q.v[LC][i];
}
__device__ __forceinline__ double a_dual(const QPDev& q, int i) {
  return q.naive ? data_dual<DM_A_NAIVE>(q, i) : data_dual<DM_A>(q, i);
}

// where slot `slot` starts in a row of the layout of IPMZ_STATE_RES.  The offsets are those of any QP of the batch
// (one formulation, one shape): q0 = qs[0], so that they are uniform loads, hoisted out of every loop
__device__ __forceinline__ int64_t slot_off(const QPDev& q0, int slot) { return q0.r[slot] - q0.r[0]; }

// The vector blocks, K = block - DB_C: c, l_x, u_x, l_A, u_A, d.  Vector K enters element t of the residual slot
// vec_slot(K) -- when the formulation has that row (vec_has) -- with the term
//
//             Slacks          otherwise
//   c         v               v             r_x = (c + ...)
//   l_x, l_A  -(lambda*v)     v             ((X - L_x)*lambda_y), ((S - L_A)*lambda_g) | (l + y - x), (l_A + g - s | (A*x))
//   u_x, u_A  lambda*v        -v            ((U_x - X)*lambda_z), ((U_A - S)*lambda_h) | (x + z - u), (h + s | (A*x) - u_A)
//   d         -v              -v            every r_lambda_C has - d
//
// lambda = the slot's own dual of the QP q whose iterate is read; l_A and u_A take the Slacks form under
// InequalityHandling::Slacks alone (slacks and naive exclude each other, create_solver).  The gradient calls
// vec_term with v = the cotangent of that slot, the tangents with v = the tangent's element.  vec_sign: the
// `otherwise` column as a factor, for a sum that applies it to plain loads (k_grad_vectors_shared).
__host__ __device__ constexpr int vec_slot(int K) {
  return K == 0 ? X : K == 1 ? LY : K == 2 ? LZ : K == 3 ? LG : K == 4 ? LH : LC;
}
__host__ __device__ constexpr double vec_sign(int K) { return K == 0 || K == 1 || K == 3 ? 1.0 : -1.0; }
template <int K>
__device__ __forceinline__ bool vec_has(const QPDev& q0) {  // the formulation has the row (c, d: always)
  return K == 1 ? q0.vlo : K == 2 ? q0.vup : K == 3 ? q0.alo : K == 4 ? q0.aup : true;
}
template <int K>
__device__ __forceinline__ double vec_term(const QPDev& q0, const QPDev& q, int t, double v) {
  if (K == 0) return v;
  if (K == 5) return -v;
  const bool sl = K <= 2 ? q0.slacks : q0.slacks && !q0.naive;
  if (K == 1 || K == 3) return sl ? -(q.v[vec_slot(K)][t] * v) : v;
  return sl ? q.v[vec_slot(K)][t] * v : -v;
}

// a grid of at most ~4096 workgroups of GRID_NT threads: x over one QP's `per` work items (grid-stride), y over the
// QPs (looped)
constexpr int GRID_NT = 256;
inline dim3 block_grid(int64_t per, int B) {
  int64_t gx = (per + GRID_NT - 1) / GRID_NT;
  gx = gx < 1 ? 1 : gx > 2048 ? 2048 : gx;
  int64_t gy = 4096 / gx;
  gy = gy < 1 ? 1 : gy > B ? B : gy;
  return dim3((unsigned)gx, (unsigned)gy);
}
// 16-byte accesses to whole pairs of a block's rows
inline bool vec16_ok(const double* p, int64_t ld, int64_t sq) { return !((uintptr_t)p & 15) && !(ld & 1) && !(sq & 1); }

}  // namespace ipmz
