// C++ API test of LinearSolvers::overwriting_solve_ldlt_multi: a small
// quasi-definite system (N = 70, two 64-column blocks) with 3 right-hand
// sides, each row against the single-vector function.  Built by the
// Makefile's cxxtest target and run by tests/test_gpu_cxx_multi.py.
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
  const int N = 70, NP = 50, NRHS = 3;
  // [[H, A^T], [A, -E]] with H, E diagonally dominant: quasi-definite
  unsigned long long z = 12345;
  auto rnd = [&]() {
    z = z * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(z >> 11) * 0x1.0p-53 - 0.5;
  };
  Matrix K(N, Vector(N, 0.0));
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < i; ++j) K[i][j] = K[j][i] = rnd();
    K[i][i] = (i < NP ? 1.0 : -1.0) * (N + 2.0 + rnd());
  }
  auto [L, D] = LinearSolvers::ldlt_decomposition(K);
  Matrix B(NRHS, Vector(N));
  for (auto& row : B)
    for (auto& v : row) v = rnd();
  Matrix X = B;
  LinearSolvers::overwriting_solve_ldlt_multi(L, D, X);
  double worst = 0.0;
  for (int r = 0; r < NRHS; ++r) {
    Vector x = B[r];
    LinearSolvers::overwriting_solve_ldlt(L, D, x);
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
      EXPECT(std::fabs(s) < 1e-11);
    }
  }
  // size mismatches throw AssertionError (a std::logic_error); empty B is a no-op
  bool threw = false;
  try {
    Matrix bad(2, Vector(N - 1));
    LinearSolvers::overwriting_solve_ldlt_multi(L, D, bad);
  } catch (const std::logic_error&) {
    threw = true;
  }
  EXPECT(threw);
  Matrix none;
  LinearSolvers::overwriting_solve_ldlt_multi(L, D, none);
  std::printf("cxx solve multi ok: N = %d, %d right-hand sides, max |x_multi - x_single| = %.3e\n", N, NRHS, worst);
  return 0;
}
