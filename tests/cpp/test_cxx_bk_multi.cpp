// C++ API test of LinearSolvers::overwriting_solve_bunch_kaufman_multi: a
// small KKT system with a zero trailing block (N = 70, two 64-column blocks:
// interchanges and 2x2 pivots) with 3 and 14 right-hand sides (the looped and
// the blocked path), each row against the single-vector function.  Built by
// the Makefile's cxxtest target and run by tests/test_gpu_cxx_bk_multi.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "ipmz/NumericalOptimization.hpp"

using namespace ipmz::NumericalOptimization;

#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

int main() {
  const int N = 70, NX = 50;
  unsigned long long z = 4711;
  auto rnd = [&]() {
    z = z * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(z >> 11) * 0x1.0p-52 - 1.0;
  };
  // [[H, A^T], [A, 0]] with a weak diagonal of H
  Matrix K(N, Vector(N, 0.0));
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i && j < NX; ++j) K[i][j] = K[j][i] = (i == j ? 0.01 : 1.0) * rnd();
  auto [F, ipiv] = LinearSolvers::symmetric_indefinite_factorization(K);
  bool pair = false, swap = false;
  for (int k = 0; k < N; ++k) {
    pair = pair || ipiv[k] < 0;
    swap = swap || (ipiv[k] >= 0 && ipiv[k] != k);
  }
  EXPECT(pair && swap);
  double worst = 0.0;
  for (int nrhs : {3, 14}) {
    Matrix B(nrhs, Vector(N));
    for (auto& row : B)
      for (auto& v : row) v = rnd();
    Matrix X = B;
    LinearSolvers::overwriting_solve_bunch_kaufman_multi(F, ipiv, X);
    for (int r = 0; r < nrhs; ++r) {
      Vector x = B[r];
      LinearSolvers::overwriting_solve_bunch_kaufman(F, ipiv, x);
      double scale = 1.0;
      for (int j = 0; j < N; ++j) scale = std::fmax(scale, std::fabs(x[j]));
      for (int j = 0; j < N; ++j) {
        EXPECT(std::isfinite(X[r][j]));
        const double e = std::fabs(X[r][j] - x[j]);
        worst = std::fmax(worst, e);
        EXPECT(e < 1e-10 * scale);
      }
      // and the residual of the original system
      for (int i = 0; i < N; ++i) {
        double s = -B[r][i];
        for (int j = 0; j < N; ++j) s += K[i][j] * X[r][j];
        EXPECT(std::fabs(s) < 1e-10 * scale);
      }
    }
  }
  // size mismatches throw AssertionError (a std::logic_error); empty B is a no-op
  bool threw = false;
  try {
    Matrix bad(2, Vector(N - 1));
    LinearSolvers::overwriting_solve_bunch_kaufman_multi(F, ipiv, bad);
  } catch (const std::logic_error&) {
    threw = true;
  }
  EXPECT(threw);
  Matrix none;
  LinearSolvers::overwriting_solve_bunch_kaufman_multi(F, ipiv, none);
  std::printf("cxx bk multi ok: N = %d, max |x_multi - x_single| = %.3e\n", N, worst);
  return 0;
}
