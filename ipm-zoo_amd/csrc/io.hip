// Whole batches in and out of a solver without a trip through host memory
// (ipmz_batch_load_device, ipmz_batch_copy_state): build_environment's bound
// check over every QP of a caller's strided device blocks, the copy of those
// blocks into the storage the QPDev descriptors name, and the state vectors
// of every QP into the rows of one matrix in the reference's Newton order --
// and back (ipmz_batch_set_state_device): the rows of such a matrix, pushed
// into the interior and checked, into the iterates.
//
// All of them are plain loads and stores, HBM-bound.  The QP index is a looped
// grid dimension (any batch size), every offset is 64-bit, and consecutive
// threads take consecutive elements of a row.
#include <climits>

#include "common.h"
#include "data_terms.h"
#include "kernels.h"

namespace ipmz {

namespace {
constexpr int NT = GRID_NT;  // (block_grid's workgroups)

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
}  // namespace

// ---------------------------------------------------------------------------
// EnvironmentBuilder.cpp:12-17 over the batch: item k < n of QP z is the pair
// (l_x[k], u_x[k]), item n + k the pair (l_A[k], u_A[k]).  A side the caller
// does not supply is the one the solver holds; a pair with neither side
// supplied is not an item (nx / na = 0).  The smallest key of a violated item
// wins whatever the schedule: one atomicMin per wave that saw one.
__global__ void __launch_bounds__(NT) k_io_validate(const QPDev* __restrict__ qs, QpBlocksIn in, int B, int nx, int na,
                                                    unsigned long long* __restrict__ verdict) {
  const int per = nx + na;
  unsigned long long key = IPMZ_IO_VALID;
  for (int z = blockIdx.y; z < B; z += gridDim.y) {
    const QPDev& q = qs[z];
    const double* lx = in.p[DB_LX] ? in.p[DB_LX] + (int64_t)z * in.sq[DB_LX] : q.lx;
    const double* ux = in.p[DB_UX] ? in.p[DB_UX] + (int64_t)z * in.sq[DB_UX] : q.ux;
    const double* lA = in.p[DB_LA] ? in.p[DB_LA] + (int64_t)z * in.sq[DB_LA] : q.lA;
    const double* uA = in.p[DB_UA] ? in.p[DB_UA] + (int64_t)z * in.sq[DB_UA] : q.uA;
    for (int t = blockIdx.x * NT + threadIdx.x; t < per; t += gridDim.x * NT) {
      bool bad;
      int kind, k;
      if (t < nx) {
        kind = 0, k = t;
        bad = !(lx[k] < ux[k]);
      } else {
        kind = 1, k = t - nx;
        bad = !(lA[k] <= uA[k]);
      }
      if (bad) {
        const unsigned long long cand = io_key(z, kind, k);
        key = cand < key ? cand : key;
      }
    }
  }
  key = wave_min_u64(key);
  if ((threadIdx.x & 63) == 0 && key != IPMZ_IO_VALID) atomicMin(verdict, key);
}

hipError_t qp_io_validate(const QPBatch& qb, const QpBlocksIn& in, unsigned long long* verdict, hipStream_t st) {
  const int nx = (in.p[DB_LX] || in.p[DB_UX]) ? qb.h.n : 0, na = (in.p[DB_LA] || in.p[DB_UA]) ? qb.h.m_usr : 0;
  hipError_t e = hipMemsetAsync(verdict, 0xff, sizeof(unsigned long long), st);  // IPMZ_IO_VALID
  if (e != hipSuccess || nx + na == 0) return e;
  hipLaunchKernelGGL(k_io_validate, block_grid(nx + na, qb.B), dim3(NT), 0, st, qb.d, in, qb.B, nx, na, verdict);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// One matrix block: rows x n elements of every QP from src + z sq + i ld + j
// to the QP's own Q / A / C (which = 0 / 1 / 2) at i ldn + j; columns [n, ldn)
// are not touched.  VEC: 16-byte accesses (the host checked that src, ld and
// sq allow them; the destination rows are 64-byte aligned) -- a row is
// n / 2 pairs and, for odd n, one last element.
template <bool VEC>
__global__ void __launch_bounds__(NT) k_io_pack_matrix(const QPDev* __restrict__ qs, const double* __restrict__ src,
                                                       int64_t ld, int64_t sq, int rows, int which, int B) {
  const int n = qs[0].n;
  const int64_t ldn = qs[0].ldn;
  const int ipr = VEC ? (n + 1) / 2 : n;  // work items per row
  const int64_t per = (int64_t)rows * ipr;
  const bool small = per <= INT_MAX;  // (32-bit division where it serves)
  for (int z = blockIdx.y; z < B; z += gridDim.y) {
    const QPDev& q = qs[z];
    double* dst = const_cast<double*>(which == 0 ? q.Q : which == 1 ? q.A : q.C);
    const double* s = src + (int64_t)z * sq;
    for (int64_t t = blockIdx.x * (int64_t)NT + threadIdx.x; t < per; t += (int64_t)gridDim.x * NT) {
      int64_t i;
      int j;
      if (small) {
        i = (unsigned)t / (unsigned)ipr;
        j = (unsigned)t % (unsigned)ipr;
      } else {
        i = t / ipr;
        j = (int)(t % ipr);
      }
      if (VEC) {
        const int c = 2 * j;
        if (c + 1 < n)
          *reinterpret_cast<double2*>(dst + i * ldn + c) = *reinterpret_cast<const double2*>(s + i * ld + c);
        else
          dst[i * ldn + c] = s[i * ld + c];
      } else {
        dst[i * ldn + j] = s[i * ld + j];
      }
    }
  }
}

// The vector blocks in one launch: c, l_x, u_x (n), l_A, u_A (m_usr), d
// (p_usr); with eqss the equality rows m_usr.. of l_A and u_A receive d too.
__global__ void __launch_bounds__(NT) k_io_pack_vectors(const QPDev* __restrict__ qs, QpBlocksIn in, int B) {
  const int n = qs[0].n, m = qs[0].m_usr, p = qs[0].p_usr;
  for (int z = blockIdx.y; z < B; z += gridDim.y) {
    const QPDev& q = qs[z];
    for (int t = blockIdx.x * NT + threadIdx.x; t < n || t < m || t < p; t += gridDim.x * NT) {
      if (t < n) {
        if (in.p[DB_C]) const_cast<double*>(q.c)[t] = in.p[DB_C][(int64_t)z * in.sq[DB_C] + t];
        if (in.p[DB_LX]) const_cast<double*>(q.lx)[t] = in.p[DB_LX][(int64_t)z * in.sq[DB_LX] + t];
        if (in.p[DB_UX]) const_cast<double*>(q.ux)[t] = in.p[DB_UX][(int64_t)z * in.sq[DB_UX] + t];
      }
      if (t < m) {
        if (in.p[DB_LA]) const_cast<double*>(q.lA)[t] = in.p[DB_LA][(int64_t)z * in.sq[DB_LA] + t];
        if (in.p[DB_UA]) const_cast<double*>(q.uA)[t] = in.p[DB_UA][(int64_t)z * in.sq[DB_UA] + t];
      }
      if (t < p && in.p[DB_D]) {
        const double v = in.p[DB_D][(int64_t)z * in.sq[DB_D] + t];
        const_cast<double*>(q.d)[t] = v;
        if (q.eqss) const_cast<double*>(q.lA)[m + t] = const_cast<double*>(q.uA)[m + t] = v;
      }
    }
  }
}

hipError_t qp_io_pack(const QPBatch& qb, const QpBlocksIn& in, hipStream_t st) {
  const QPDev& h = qb.h;
  const int dims[3] = {h.n, h.m_usr, h.p_usr};  // (the data's rows: the equality-slack handlings run C's as A's)
  bool vectors = false;
  for (int w = 0; w < DB_COUNT; ++w) {
    if (!in.p[w]) continue;
    if (!DATA_BLOCKS[w].matrix) {
      vectors = true;
      continue;
    }
    const int rows = dims[DATA_BLOCKS[w].dim];
    if (vec16_ok(in.p[w], in.ld[w], in.sq[w]))
      hipLaunchKernelGGL(k_io_pack_matrix<true>, block_grid((int64_t)rows * ((h.n + 1) / 2), qb.B), dim3(NT), 0, st, qb.d,
                         in.p[w], in.ld[w], in.sq[w], rows, w, qb.B);
    else
      hipLaunchKernelGGL(k_io_pack_matrix<false>, block_grid((int64_t)rows * h.n, qb.B), dim3(NT), 0, st, qb.d, in.p[w],
                         in.ld[w], in.sq[w], rows, w, qb.B);
  }
  if (vectors) {
    const int mp = dims[1] > dims[2] ? dims[1] : dims[2];
    hipLaunchKernelGGL(k_io_pack_vectors, block_grid(h.n > mp ? h.n : mp, qb.B), dim3(NT), 0, st, qb.d, in, qb.B);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Row z of dst (row stride ld) <- the state_len doubles of QP z's iterate,
// affine direction, direction or residuals (which = IPMZ_STATE_*) in the
// reference's Newton order; columns [state_len, ld) are not written.  With
// the equality-slack formulations that order is a permutation of the step's
// slots: eqss_source (kernels.h), which the host read-back uses too.
__global__ void __launch_bounds__(NT) k_io_gather_state(const QPDev* __restrict__ qs, int which, double* __restrict__ dst,
                                                        int64_t ld, int B) {
  const int64_t L = qs[0].state_len;
  const bool eqss = qs[0].eqss;
  for (int z = blockIdx.y; z < B; z += gridDim.y) {
    const QPDev& q = qs[z];
    const double* src = which == 0 ? q.v[0] : which == 1 ? q.daff[0] : which == 2 ? q.dir[0] : q.r[0];
    double* row = dst + (int64_t)z * ld;
    for (int64_t k = blockIdx.x * (int64_t)NT + threadIdx.x; k < L; k += (int64_t)gridDim.x * NT)
      row[k] = src[eqss ? eqss_source(k, q) : k];
  }
}

hipError_t qp_gather_state(const QPBatch& qb, int which, double* dst, int64_t ld, hipStream_t st) {
  hipLaunchKernelGGL(k_io_gather_state, block_grid(qb.h.state_len, qb.B), dim3(NT), 0, st, qb.d, which, dst, ld, qb.B);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The warm start (ipmz_batch_set_state_device): the gather's inverse, with the
// interior push and, in a kernel of its own, the check of what ratio_elem
// (newton.hip) needs of an iterate.  Both walk the rows the same way and share
// warm_elem: component k of a caller's row -> the step-vector index j it goes
// to, its value after the push, and whether the iterate may not hold it.
namespace {
// the slot step-vector index j lies in and the index i within it: the last
// slot in the vector's order (slot_in_order) that starts at or before j --
// the absent ones, of length 0, start where the next present one does
__device__ __forceinline__ int state_slot(const QPDev& q, int64_t j, int& i) {
  int slot = X;
  int64_t off = 0;
#pragma unroll
  for (int k = 1; k < NSLOT; ++k) {
    const int sl = slot_in_order(q.naive, k);
    const int64_t o = q.v[sl] - q.v[X];
    if (o <= j) slot = sl, off = o;
  }
  i = (int)(j - off);
  return slot;
}

__device__ __forceinline__ double warm_elem(const QPDev& q, const double* __restrict__ row, int64_t k, double floor,
                                            int64_t& j, bool& bad) {
  j = q.eqss ? eqss_source(k, q) : k;
  int i;
  const int slot = state_slot(q, j, i);
  double v = row[k];
  if (nonneg_slot(slot)) {
    v = v < floor ? floor : v;
    bad = !(v > 0.0);  // (a NaN passes the push and fails here)
  } else if (explicit_bounds(q) && slot == X) {
    bad = !(q.lx[i] < v && v < q.ux[i]);
  } else if (explicit_bounds(q) && slot == S) {
    bad = !(q.lA[i] < v && v < q.uA[i]);
  } else {
    bad = v != v;
  }
  return v;
}
}  // namespace

// The thread index runs over the SOURCE row, the caller's order: the loads of
// a wave are consecutive whatever the row's alignment and stride, a row that
// is not taken and the padding of one that is are never touched, and the
// check's key is the index the caller knows.  The stores are the permuted
// side, but eqss_source maps the row piecewise by translation (at most nine
// pieces: x / the duals, four of each equality-slack block, the rest), so
// they are consecutive too except in the waves that straddle a piece's end --
// the gather's argument with load and store exchanged.  Indexing the
// destination instead would need the inverse map stated a second time and
// gain nothing: one side is cut at the piece ends either way.
__global__ void __launch_bounds__(NT) k_io_scatter_state(const QPDev* __restrict__ qs, const double* __restrict__ src,
                                                         int64_t ld, const int32_t* __restrict__ take, double floor,
                                                         int B) {
  const int64_t L = qs[0].state_len;
  for (int z = blockIdx.y; z < B; z += gridDim.y) {
    if (take && !take[z]) continue;
    const QPDev& q = qs[z];
    const double* row = src + (int64_t)z * ld;
    double* dst = q.v[X];
    for (int64_t k = blockIdx.x * (int64_t)NT + threadIdx.x; k < L; k += (int64_t)gridDim.x * NT) {
      int64_t j;
      bool bad;
      const double v = warm_elem(q, row, k, floor, j, bad);
      dst[j] = v;
    }
  }
}

hipError_t qp_scatter_state(const QPBatch& qb, const double* src, int64_t ld, const int32_t* take, double floor,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_io_scatter_state, block_grid(qb.h.state_len, qb.B), dim3(NT), 0, st, qb.d, src, ld, take, floor,
                     qb.B);
  return hipGetLastError();
}

// The smallest key z * state_len + k of a violation wins whatever the
// schedule: one atomicMin per wave that saw one (as k_io_validate).
__global__ void __launch_bounds__(NT) k_io_scatter_validate(const QPDev* __restrict__ qs, const double* __restrict__ src,
                                                            int64_t ld, const int32_t* __restrict__ take, double floor,
                                                            int B, unsigned long long* __restrict__ verdict) {
  const int64_t L = qs[0].state_len;
  unsigned long long key = IPMZ_IO_VALID;
  for (int z = blockIdx.y; z < B; z += gridDim.y) {
    if (take && !take[z]) continue;
    const QPDev& q = qs[z];
    const double* row = src + (int64_t)z * ld;
    for (int64_t k = blockIdx.x * (int64_t)NT + threadIdx.x; k < L; k += (int64_t)gridDim.x * NT) {
      int64_t j;
      bool bad;
      warm_elem(q, row, k, floor, j, bad);
      if (bad) {
        const unsigned long long cand = (unsigned long long)z * (unsigned long long)L + (unsigned long long)k;
        key = cand < key ? cand : key;
      }
    }
  }
  key = wave_min_u64(key);
  if ((threadIdx.x & 63) == 0 && key != IPMZ_IO_VALID) atomicMin(verdict, key);
}

hipError_t qp_scatter_validate(const QPBatch& qb, const double* src, int64_t ld, const int32_t* take, double floor,
                               unsigned long long* verdict, hipStream_t st) {
  hipError_t e = hipMemsetAsync(verdict, 0xff, sizeof(unsigned long long), st);  // IPMZ_IO_VALID
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_io_scatter_validate, block_grid(qb.h.state_len, qb.B), dim3(NT), 0, st, qb.d, src, ld, take,
                     floor, qb.B, verdict);
  return hipGetLastError();
}

}  // namespace ipmz
