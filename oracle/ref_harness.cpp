// Golden-vector harness for the upstream reference (albfre/ipm-zoo).
//
// TEST INFRASTRUCTURE ONLY.  Linked against the reference objects built by
// oracle/Makefile.ref into oracle/_ref/; it never ships in the product
// library and nothing on the GPU box runs it (the reference does not travel).
// Its outputs are the small fixtures committed under tests/golden/ by
// tests/golden/make_golden.py.
//
// Modes (all write to the directory given as argv[2]):
//   formulation <dir>               formulation strings per Settings
//   ldlt <dir> <N> <seed> <tag>     LinearSolvers::ldlt_decomposition +
//                                   overwriting_solve_ldlt on a generated
//                                   quasi-definite K (LinearSolvers.cpp:14-74)
//   bk <dir> <N> <seed> <tag>       symmetric_indefinite_factorization +
//                                   overwriting_solve_bunch_kaufman
//                                   (LinearSolvers.cpp:76-318)
//   bk_rand <dir> <N> <seed> <zeros> <tag>
//                                   the same pair on a dense indefinite K that
//                                   forces interchanges and 2 x 2 pivots
//   bk_zeros_at <dir> <N> <seed> <i,j,..> <tag>
//                                   the same with zero rows/columns at i, j, ..
//   bk_file <dir> <N> <tag>         the same pair on the K (N x N, row-major)
//                                   and b read from <dir>/<tag>_K.bin and
//                                   <tag>_b.bin (tests/bk_pivot_cases.py: tied
//                                   maxima, threshold equalities, a NaN pivot);
//                                   writes <tag>_F, _ipiv, _x
//   newton <dir> <n> <m> <seed> <iters> <tag>
//                                   SlackedSlacks (box [+ ineq]) Newton
//                                   iterations through the reference's own
//                                   Optimizer private methods
//                                   (Optimizer.cpp:127-219)
//     [<ineq> <ineq bounds> <var bounds> [<p> <equality handling>]]
//   component_eq <dir> <n> <m> <p> <seed> <tag>
//                                   C3 structure (Regularization equalities):
//                                   reference Evaluation for every non-scalar
//                                   block, scalar/zero blocks expanded here
//                                   to s*I / 0, reference ldlt + solve.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "Expr.h"
#include "ExprFactory.h"
#include "NumericalOptimization/EnvironmentBuilder.h"
#include "NumericalOptimization/Evaluation.h"
#include "NumericalOptimization/LinearSolvers.h"
#include "SymbolicOptimization.h"
#include "Utils/Helpers.h"
#define private public
#include "NumericalOptimization/Optimizer.h"
#undef private

using Mat = std::vector<std::vector<double>>;
using Vec = std::vector<double>;
namespace SO = SymbolicOptimization;
namespace NO = NumericalOptimization;

// ---------------------------------------------------------------------------
// Counter-based generator -- identical to
// ipm-zoo_amd/csrc/qpgen.h and oracle/ipmz_oracle.cpp.
static inline uint64_t splitmix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ULL;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
static inline double u01(uint64_t seed, uint64_t tag, uint64_t i, uint64_t j) {
  const uint64_t key = seed ^ (tag << 56) ^ ((i << 32) + j);
  return (double)(splitmix64(key) >> 11) * 0x1.0p-53;
}
enum : uint64_t { TAG_Q = 1, TAG_C = 2, TAG_A = 3, TAG_C_EQ = 4, TAG_D = 5, TAG_K = 6, TAG_B = 7 };

struct QP {
  size_t n, m, p;
  Mat Q, A, C;
  Vec c, lA, uA, d, lx, ux;
};

static QP make_qp(size_t n, size_t m, size_t p, uint64_t seed) {
  QP q{n, m, p};
  q.Q.assign(n, Vec(n));
  for (size_t i = 0; i < n; ++i) {
    for (size_t j = 0; j < i; ++j) {
      const double v = (2.0 * u01(seed, TAG_Q, i, j) - 1.0) / (double)n;
      q.Q[i][j] = v;
      q.Q[j][i] = v;
    }
    q.Q[i][i] = 1.0 + u01(seed, TAG_Q, i, i);
  }
  q.c.resize(n);
  for (size_t i = 0; i < n; ++i) q.c[i] = 2.0 * u01(seed, TAG_C, i, 0) - 1.0;
  const double sn = std::sqrt((double)n);
  q.A.assign(m, Vec(n));
  for (size_t i = 0; i < m; ++i)
    for (size_t j = 0; j < n; ++j) q.A[i][j] = (2.0 * u01(seed, TAG_A, i, j) - 1.0) / sn;
  q.C.assign(p, Vec(n));
  for (size_t i = 0; i < p; ++i)
    for (size_t j = 0; j < n; ++j) q.C[i][j] = (2.0 * u01(seed, TAG_C_EQ, i, j) - 1.0) / sn;
  q.lA.assign(m, -1.0);
  q.uA.assign(m, 1.0);
  q.d.resize(p);
  for (size_t i = 0; i < p; ++i) q.d[i] = (2.0 * u01(seed, TAG_D, i, 0) - 1.0) * 0.1;
  q.lx.assign(n, -1.0);
  q.ux.assign(n, 1.0);
  return q;
}

// ---------------------------------------------------------------------------
static void write_bin(const std::string& path, const Vec& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(double)));
}
static Vec flatten(const Mat& M) {
  Vec out;
  for (const auto& r : M) out.insert(out.end(), r.begin(), r.end());
  return out;
}
static Vec lower_packed(const Mat& M) {  // row-major packed lower triangle
  Vec out;
  for (size_t i = 0; i < M.size(); ++i)
    for (size_t j = 0; j <= i; ++j) out.push_back(M[i][j]);
  return out;
}

struct Silence {  // the reference prints O(N^2) per iteration
  std::streambuf* old;
  std::ostringstream sink;
  Silence() : old(std::cout.rdbuf()) { std::cout.rdbuf(sink.rdbuf()); }
  ~Silence() { std::cout.rdbuf(old); }
};

static std::string to_s(const Expression::ExprPtr& e) { return e ? e->to_string() : std::string("<null>"); }

// ---------------------------------------------------------------------------
static SO::Settings settings_from(const std::string& ineq, const std::string& eq, bool has_ineq) {
  SO::Settings s;
  s.inequalities = has_ineq ? SO::Bounds::Both : SO::Bounds::None;
  s.variable_bounds = SO::Bounds::Both;
  if (ineq == "Slacks") s.inequality_handling = SO::InequalityHandling::Slacks;
  else if (ineq == "NaiveSlacks") s.inequality_handling = SO::InequalityHandling::NaiveSlacks;
  else s.inequality_handling = SO::InequalityHandling::SlackedSlacks;
  s.equalities = eq != "none";
  if (eq == "None") s.equality_handling = SO::EqualityHandling::None;
  else if (eq == "Regularization") s.equality_handling = SO::EqualityHandling::Regularization;
  else if (eq == "PenaltyFunction") s.equality_handling = SO::EqualityHandling::PenaltyFunction;
  else if (eq == "SlackedSlacks") s.equality_handling = SO::EqualityHandling::SlackedSlacks;
  else if (eq == "Slacks") s.equality_handling = SO::EqualityHandling::Slacks;
  else if (eq == "NaiveSlacks") s.equality_handling = SO::EqualityHandling::NaiveSlacks;
  else if (eq == "PenaltyFunctionWithExtraDual") s.equality_handling = SO::EqualityHandling::PenaltyFunctionWithExtraDual;
  return s;
}

static void dump_system(std::ostream& os, const SO::NewtonSystem& ns) {
  os << "  variables:";
  for (auto& v : ns.variables) os << " [" << to_s(v) << "]";
  os << "\n  lhs:\n";
  for (auto& row : ns.lhs) {
    os << "   ";
    for (auto& e : row) os << " | " << to_s(e);
    os << "\n";
  }
  os << "  rhs:\n";
  for (auto& e : ns.rhs) os << "    " << to_s(e) << "\n";
  os << "  delta_definitions:\n";
  for (auto& [v, d] : ns.delta_definitions) os << "    " << to_s(v) << " := " << to_s(d) << "\n";
}

static SO::Bounds bounds_from(const std::string& b) {
  if (b == "None") return SO::Bounds::None;
  if (b == "Lower") return SO::Bounds::Lower;
  if (b == "Upper") return SO::Bounds::Upper;
  return SO::Bounds::Both;
}

// one Settings' formulation to stdout (exploration; fixtures use mode_formulation)
static int mode_formulation_one(const std::string& ineq, const std::string& ineq_bounds,
                                const std::string& var_bounds, const std::string& eq = "none") {
  SO::Settings s = settings_from(ineq, eq, ineq_bounds != "None");
  s.inequalities = bounds_from(ineq_bounds);
  s.variable_bounds = bounds_from(var_bounds);
  const SO::VariableNames names;
  const auto ns = SO::get_newton_system(s, names);
  std::cout << "-- newton system\n";
  dump_system(std::cout, ns);
  const auto sh = SO::get_shorthand_rhs(ns);
  std::cout << "-- shorthand definitions\n";
  for (auto& [v, d] : sh.vector_definitions) std::cout << "    " << to_s(v) << " := " << to_s(d) << "\n";
  auto ns2 = ns;
  ns2.rhs = sh.shorthand_rhs;
  const auto aug = SO::get_augmented_system(ns2);
  std::cout << "-- augmented system\n";
  dump_system(std::cout, aug);
  return 0;
}

static int mode_formulation(const std::string& dir) {
  std::ofstream os(dir + "/formulations.txt");
  const SO::VariableNames names;
  struct Case { const char* ineq; const char* eq; bool has_ineq; const char* ib; const char* vb; };
  const Case cases[] = {
      {"SlackedSlacks", "none", false, "None", "Both"}, {"SlackedSlacks", "none", true, "Both", "Both"},
      {"SlackedSlacks", "Regularization", true, "Both", "Both"}, {"Slacks", "none", true, "Both", "Both"},
      {"SlackedSlacks", "None", true, "Both", "Both"}, {"SlackedSlacks", "PenaltyFunction", true, "Both", "Both"},
      // one-sided / absent bounds (Settings::inequalities, Settings::variable_bounds) and box-only Slacks
      {"SlackedSlacks", "none", true, "Both", "Lower"}, {"SlackedSlacks", "none", true, "Both", "Upper"},
      {"SlackedSlacks", "none", true, "Both", "None"}, {"SlackedSlacks", "none", true, "Lower", "Both"},
      {"SlackedSlacks", "none", true, "Upper", "Both"}, {"Slacks", "none", false, "None", "Both"},
      // equality handlings beyond the numerically used ones (their Newton
      // systems: PenaltyFunctionWithExtraDual is the system PenaltyFunction is
      // mapped to, SymbolicOptimization.cpp:364-366), and NaiveSlacks
      {"SlackedSlacks", "PenaltyFunctionWithExtraDual", true, "Both", "Both"},
      {"SlackedSlacks", "SlackedSlacks", true, "Both", "Both"},
      {"NaiveSlacks", "none", true, "Both", "Both"},
  };
  for (const auto& c : cases) {
    auto s = settings_from(c.ineq, c.eq, c.has_ineq);
    s.inequalities = bounds_from(c.ib);
    s.variable_bounds = bounds_from(c.vb);
    os << "=== inequality_handling=" << c.ineq << " equalities=" << c.eq << " inequalities=" << c.ib;
    if (std::string(c.vb) != "Both") os << " variable_bounds=" << c.vb;
    os << "\n";
    const auto ns = SO::get_newton_system(s, names);
    os << "-- newton system\n";
    dump_system(os, ns);
    const auto sh = SO::get_shorthand_rhs(ns);
    os << "-- shorthand definitions\n";
    for (auto& [v, d] : sh.vector_definitions) os << "    " << to_s(v) << " := " << to_s(d) << "\n";
    auto ns2 = ns;
    ns2.rhs = sh.shorthand_rhs;
    const auto aug = SO::get_augmented_system(ns2);
    os << "-- augmented system\n";
    dump_system(os, aug);
    const auto ne = SO::get_normal_equations(aug);
    os << "-- normal equations\n";
    dump_system(os, ne);
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Seeded quasi-definite K = [H B^T; B -G] with H SPD and G positive diagonal.
static Mat make_qd(size_t N, uint64_t seed) {
  const size_t n1 = (N * 3 + 3) / 4;  // leading SPD block
  Mat K(N, Vec(N, 0.0));
  for (size_t i = 0; i < N; ++i) {
    for (size_t j = 0; j < i; ++j) {
      double v;
      if (i < n1) v = (2.0 * u01(seed, TAG_K, i, j) - 1.0) / (double)n1;
      else if (j < n1) v = (2.0 * u01(seed, TAG_K, i, j) - 1.0) / std::sqrt((double)n1);
      else v = 0.0;
      K[i][j] = v;
      K[j][i] = v;
    }
    K[i][i] = i < n1 ? 1.0 + u01(seed, TAG_K, i, i) : -(0.5 + u01(seed, TAG_K, i, i));
  }
  return K;
}

static int mode_ldlt(const std::string& dir, size_t N, uint64_t seed, const std::string& tag) {
  const Mat K = make_qd(N, seed);
  Vec b(N);
  for (size_t i = 0; i < N; ++i) b[i] = 2.0 * u01(seed, TAG_B, i, 0) - 1.0;
  auto [L, D] = NO::LinearSolvers::ldlt_decomposition(K);
  Vec x = b;
  NO::LinearSolvers::overwriting_solve_ldlt(L, D, x);
  write_bin(dir + "/" + tag + "_K.bin", lower_packed(K));
  write_bin(dir + "/" + tag + "_L.bin", lower_packed(L));
  write_bin(dir + "/" + tag + "_D.bin", D);
  write_bin(dir + "/" + tag + "_b.bin", b);
  write_bin(dir + "/" + tag + "_x.bin", x);
  return 0;
}

static int mode_bk(const std::string& dir, size_t N, uint64_t seed, const std::string& tag) {
  // Indefinite K with a zero trailing diagonal block (EqualityHandling::None
  // structure): [H C^T; C 0].
  Mat K = make_qd(N, seed);
  const size_t n1 = (N * 3 + 3) / 4;
  for (size_t i = n1; i < N; ++i) K[i][i] = 0.0;
  Vec b(N);
  for (size_t i = 0; i < N; ++i) b[i] = 2.0 * u01(seed, TAG_B, i, 0) - 1.0;
  auto [F, ipiv] = NO::LinearSolvers::symmetric_indefinite_factorization(K);
  Vec x = b;
  NO::LinearSolvers::overwriting_solve_bunch_kaufman(F, ipiv, x);
  Vec piv(ipiv.begin(), ipiv.end());
  write_bin(dir + "/" + tag + "_K.bin", flatten(K));
  write_bin(dir + "/" + tag + "_F.bin", flatten(F));
  write_bin(dir + "/" + tag + "_ipiv.bin", piv);
  write_bin(dir + "/" + tag + "_b.bin", b);
  write_bin(dir + "/" + tag + "_x.bin", x);
  return 0;
}

// Dense symmetric indefinite K with a small diagonal, so the reference's
// Bunch-Kaufman takes row/column interchanges and 2 x 2 pivots; `zeros`
// rows/columns (indices N/2, N/2 + 1, ...) are set to zero, which exercises
// the zero-column branch (and, for a second zero column, the kp = 0 defect,
// LinearSolvers.cpp:111-116).
static int write_bk(const std::string& dir, const Mat& K, uint64_t seed, const std::string& tag);
static Mat bk_dense(size_t N, uint64_t seed) {
  Mat K(N, Vec(N, 0.0));
  for (size_t i = 0; i < N; ++i) {
    for (size_t j = 0; j < i; ++j) {
      const double v = 2.0 * u01(seed, TAG_K, i, j) - 1.0;
      K[i][j] = v;
      K[j][i] = v;
    }
    K[i][i] = 0.05 * (2.0 * u01(seed, TAG_K, i, i) - 1.0);
  }
  return K;
}
// The same dense indefinite K with zero rows/columns at the listed indices
// (comma-separated): a zero column 0 keeps the reference's 0-based info at 0
// (LinearSolvers.cpp:113-116), so a later zero column again takes kp = k.
static int mode_bk_zeros_at(const std::string& dir, size_t N, uint64_t seed, const std::string& list,
                            const std::string& tag) {
  Mat K = bk_dense(N, seed);
  std::stringstream ss(list);
  std::string item;
  while (std::getline(ss, item, ',')) {
    const size_t r = std::stoul(item);
    for (size_t j = 0; j < N; ++j) K[r][j] = K[j][r] = 0.0;
  }
  return write_bk(dir, K, seed, tag);
}
static int write_bk(const std::string& dir, const Mat& K, uint64_t seed, const std::string& tag) {
  const size_t N = K.size();
  Vec b(N);
  for (size_t i = 0; i < N; ++i) b[i] = 2.0 * u01(seed, TAG_B, i, 0) - 1.0;
  auto [F, ipiv] = NO::LinearSolvers::symmetric_indefinite_factorization(K);
  Vec x = b;
  NO::LinearSolvers::overwriting_solve_bunch_kaufman(F, ipiv, x);
  Vec piv(ipiv.begin(), ipiv.end());
  write_bin(dir + "/" + tag + "_K.bin", flatten(K));
  write_bin(dir + "/" + tag + "_F.bin", flatten(F));
  write_bin(dir + "/" + tag + "_ipiv.bin", piv);
  write_bin(dir + "/" + tag + "_b.bin", b);
  write_bin(dir + "/" + tag + "_x.bin", x);
  return 0;
}

static int mode_bk_rand(const std::string& dir, size_t N, uint64_t seed, size_t zeros, const std::string& tag) {
  Mat K(N, Vec(N, 0.0));
  for (size_t i = 0; i < N; ++i) {
    for (size_t j = 0; j < i; ++j) {
      const double v = 2.0 * u01(seed, TAG_K, i, j) - 1.0;
      K[i][j] = v;
      K[j][i] = v;
    }
    K[i][i] = 0.05 * (2.0 * u01(seed, TAG_K, i, i) - 1.0);
  }
  for (size_t z = 0; z < zeros; ++z) {
    const size_t r = N / 2 + z;
    for (size_t j = 0; j < N; ++j) K[r][j] = K[j][r] = 0.0;
  }
  Vec b(N);
  for (size_t i = 0; i < N; ++i) b[i] = 2.0 * u01(seed, TAG_B, i, 0) - 1.0;
  auto [F, ipiv] = NO::LinearSolvers::symmetric_indefinite_factorization(K);
  Vec x = b;
  NO::LinearSolvers::overwriting_solve_bunch_kaufman(F, ipiv, x);
  Vec piv(ipiv.begin(), ipiv.end());
  write_bin(dir + "/" + tag + "_K.bin", flatten(K));
  write_bin(dir + "/" + tag + "_F.bin", flatten(F));
  write_bin(dir + "/" + tag + "_ipiv.bin", piv);
  write_bin(dir + "/" + tag + "_b.bin", b);
  write_bin(dir + "/" + tag + "_x.bin", x);
  return 0;
}

// bk_rand without the generator: K and b come from files
static Vec read_bin(const std::string& path, size_t count) {
  Vec v(count);
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(double)));
  if (!f || f.peek() != std::ifstream::traits_type::eof()) throw std::runtime_error("bad size: " + path);
  return v;
}
static int mode_bk_file(const std::string& dir, size_t N, const std::string& tag) {
  const Vec flat = read_bin(dir + "/" + tag + "_K.bin", N * N);
  const Vec b = read_bin(dir + "/" + tag + "_b.bin", N);
  Mat K(N, Vec(N, 0.0));
  for (size_t i = 0; i < N; ++i)
    for (size_t j = 0; j < N; ++j) K[i][j] = flat[i * N + j];
  auto [F, ipiv] = NO::LinearSolvers::symmetric_indefinite_factorization(K);
  Vec x = b;
  NO::LinearSolvers::overwriting_solve_bunch_kaufman(F, ipiv, x);
  Vec piv(ipiv.begin(), ipiv.end());
  write_bin(dir + "/" + tag + "_F.bin", flatten(F));
  write_bin(dir + "/" + tag + "_ipiv.bin", piv);
  write_bin(dir + "/" + tag + "_x.bin", x);
  return 0;
}

// ---------------------------------------------------------------------------
// One reference Newton iteration, restated around the reference's own private
// methods (Optimizer.cpp:127-219), recording KKT, directions and scalars.
struct IterRecord {
  double f, res, mu, alpha_aff, mu_aff, sigma, alpha;
  Mat kkt;
  Vec D;
  Mat vars, d_aff, d;
};

// The augmented lhs as get_as_matrix_ (Optimizer.cpp:387-391) builds it, with
// the scalar blocks the reference's evaluate_matrix asserts on
// (Evaluation.cpp:57-60) expanded here: a scalar diagonal block -> s*I, a
// scalar off-diagonal block must be 0 (EqualityHandling::SlackedSlacks has a
// zero lambda_A / lambda_C block).  Matrix blocks are the reference's own.
static Mat augmented_kkt(NO::Optimizer& opt) {
  const auto& lhs = opt.augmented_system_.lhs;
  const auto& vars = opt.augmented_system_.variables;
  const size_t nb = lhs.size();
  std::vector<size_t> off(nb + 1, 0);
  for (size_t i = 0; i < nb; ++i) off[i + 1] = off[i] + opt.vector_sizes_.at(vars[i]);
  Mat K(off[nb], Vec(off[nb], 0.0));
  for (size_t bi = 0; bi < nb; ++bi)
    for (size_t bj = 0; bj < nb; ++bj) {
      const auto val = NO::Evaluation::evaluate(lhs[bi][bj], opt.env_);
      if (std::holds_alternative<double>(val)) {
        const double sv = std::get<double>(val);
        if (bi == bj) {
          for (size_t k = off[bi]; k < off[bi + 1]; ++k) K[k][k] = sv;
        } else if (sv != 0.0) {
          throw std::runtime_error("non-zero scalar off-diagonal block");
        }
        continue;
      }
      const Mat M = NO::Evaluation::evaluate_matrix(lhs[bi][bj], opt.env_);
      for (size_t a = 0; a < M.size(); ++a)
        for (size_t b = 0; b < M[a].size(); ++b) K[off[bi] + a][off[bj] + b] = M[a][b];
    }
  return K;
}

static IterRecord reference_iteration(NO::Optimizer& opt) {
  IterRecord r{};
  auto& env = opt.env_;
  const auto& oe = opt.optimization_expressions_;
  const auto& full_rhs = opt.newton_system_.rhs;
  r.f = NO::Evaluation::evaluate_scalar(opt.objective_, env);
  r.res = opt.get_residual_norm_(full_rhs);
  r.mu = opt.get_mu_(full_rhs);
  r.kkt = augmented_kkt(opt);
  auto [L, D] = NO::LinearSolvers::ldlt_decomposition(r.kkt);
  r.D = D;
  env.at(oe.mu) = NO::Evaluation::val_scalar(0.0);
  for (const auto& [vec, def] : opt.shorthand_rhs_.vector_definitions) env[vec] = NO::Evaluation::evaluate(def, env);
  r.vars = opt.eval_vector_of_expressions_<Vec>(opt.newton_system_.variables);
  r.d_aff = opt.compute_search_direction_(opt.augmented_system_, L, D);
  {
    r.alpha_aff = opt.get_max_step_(r.vars, r.d_aff);
    std::vector<std::unique_ptr<NO::ScopedEnvironmentOverride>> temps;
    for (const auto& var : opt.newton_system_.variables) {
      auto val = NO::Evaluation::evaluate(var, env);
      temps.push_back(std::make_unique<NO::ScopedEnvironmentOverride>(env, var, val));
    }
    opt.update_variables_(r.alpha_aff, r.vars, r.d_aff);
    r.mu_aff = opt.get_mu_(full_rhs);
    r.sigma = r.mu > 0.0 ? std::pow(r.mu_aff / r.mu, 3) : 0.0;
    env.at(oe.mu) = NO::Evaluation::val_scalar(r.mu * r.sigma);
  }
  {
    std::vector<Expression::ExprPtr> delta_aff_variables;
    for (const auto& v : opt.newton_system_.variables) {
      const auto dv = SO::get_delta_variable(v);
      const auto& var = std::get<Expression::Variable>(dv->get_impl());
      delta_aff_variables.push_back(Expression::ExprFactory::variable(var.name + "_affine"));
    }
    for (const auto& [shorthand, expr] : opt.shorthand_rhs_.vector_definitions) {
      auto val = NO::Evaluation::evaluate(expr, env);
      if ((expr->contains_subexpression(oe.e_var) || expr->contains_subexpression(oe.e_ineq) ||
           expr->contains_subexpression(oe.e_eq)) &&
          expr->contains_subexpression(oe.mu)) {
        auto dexpr = expr->replace_subexpression(oe.mu, Expression::zero);
        for (auto& var : expr->get_variables()) {
          const auto idx = opt.variable_index_.at(var);
          env[delta_aff_variables.at(idx)] = NO::Evaluation::val_vector(r.d_aff.at(idx));
          dexpr = dexpr->replace_subexpression(var, delta_aff_variables.at(idx));
        }
        val = NO::Evaluation::add(val, NO::Evaluation::evaluate(dexpr, env));
      }
      env[shorthand] = val;
    }
    r.d = opt.compute_search_direction_(opt.augmented_system_, L, D);
    r.alpha = opt.get_max_step_(r.vars, r.d);
    opt.update_variables_(0.995 * r.alpha, r.vars, r.d);
  }
  return r;
}

static int mode_newton(const std::string& dir, size_t n, size_t m, uint64_t seed, int iters, const std::string& tag,
                       const std::string& ineq = "SlackedSlacks", const std::string& ineq_bounds = "",
                       const std::string& var_bounds = "Both", size_t p = 0, const std::string& eq = "none") {
  const QP q = make_qp(n, m, p, seed);
  NO::Data data;
  data.Q = q.Q;
  data.c = q.c;
  data.A_ineq = q.A;
  data.l_A_ineq = q.lA;
  data.u_A_ineq = q.uA;
  data.A_eq = q.C;
  data.b_eq = q.d;
  data.l_x = q.lx;
  data.u_x = q.ux;
  const SO::VariableNames names;
  SO::Settings s = settings_from(ineq, eq, m > 0);
  if (!ineq_bounds.empty()) s.inequalities = bounds_from(ineq_bounds);
  s.variable_bounds = bounds_from(var_bounds);
  const auto oe = SO::get_optimization_expressions(names);
  auto env = NO::build_environment(names, data);
  const auto ns = SO::get_newton_system(s, names);
  Silence quiet;
  NO::Optimizer opt(env, oe, ns);
  std::ofstream meta(dir + "/" + tag + "_trace.txt");
  meta.precision(17);
  meta << "variables";
  for (auto& v : opt.newton_system_.variables) meta << " " << to_s(v);
  meta << "\n";
  for (int it = 0; it < iters; ++it) {
    {
      const double res = opt.get_residual_norm_(opt.newton_system_.rhs);
      const double mu = opt.get_mu_(opt.newton_system_.rhs);
      if (res < 1e-8 && mu < 1e-8) {  // Optimizer.cpp:133
        meta << "converged " << it << " res " << res << " mu " << mu << "\n";
        break;
      }
    }
    const IterRecord r = reference_iteration(opt);
    meta << "iter " << it << " f " << r.f << " res " << r.res << " mu " << r.mu << " alpha_aff " << r.alpha_aff
         << " mu_aff " << r.mu_aff << " sigma " << r.sigma << " alpha " << r.alpha << "\n";
    const std::string p = dir + "/" + tag + "_it" + std::to_string(it);
    if (it == 0) write_bin(p + "_kkt.bin", lower_packed(r.kkt));
    write_bin(p + "_D.bin", r.D);
    write_bin(p + "_vars.bin", flatten(r.vars));
    write_bin(p + "_daff.bin", flatten(r.d_aff));
    write_bin(p + "_d.bin", flatten(r.d));
  }
  return 0;
}

// C3 structure, component level: the reference's numeric path asserts on the
// scalar (-delta^2) and zero blocks (Evaluation.cpp:57-60), so those blocks
// are expanded here; every other block is the reference's own evaluation.
static int mode_component_eq(const std::string& dir, size_t n, size_t m, size_t p, uint64_t seed,
                             const std::string& tag) {
  const QP q = make_qp(n, m, p, seed);
  NO::Data data;
  data.Q = q.Q;
  data.c = q.c;
  data.A_ineq = q.A;
  data.l_A_ineq = q.lA;
  data.u_A_ineq = q.uA;
  data.A_eq = q.C;
  data.b_eq = q.d;
  data.l_x = q.lx;
  data.u_x = q.ux;
  const SO::VariableNames names;
  SO::Settings s = settings_from("SlackedSlacks", "Regularization", true);
  auto env = NO::build_environment(names, data);
  const auto ns = SO::get_newton_system(s, names);
  auto ns2 = ns;
  const auto sh = SO::get_shorthand_rhs(ns);
  ns2.rhs = sh.shorthand_rhs;
  const auto aug = SO::get_augmented_system(ns2);
  const size_t sizes[3] = {n, m, p};
  const size_t nb = aug.lhs.size();
  size_t N = 0;
  for (size_t i = 0; i < nb; ++i) N += sizes[i];
  Mat K(N, Vec(N, 0.0));
  std::ofstream meta(dir + "/" + tag + "_blocks.txt");
  size_t r0 = 0;
  for (size_t bi = 0; bi < nb; ++bi) {
    size_t c0 = 0;
    for (size_t bj = 0; bj < nb; ++bj) {
      const auto& e = aug.lhs[bi][bj];
      const auto val = NO::Evaluation::evaluate(e, env);
      meta << bi << " " << bj << " " << to_s(e) << " kind " << val.index() << "\n";
      if (std::holds_alternative<double>(val)) {
        const double sv = std::get<double>(val);
        if (bi == bj) {
          for (size_t k = 0; k < sizes[bi]; ++k) K[r0 + k][c0 + k] = sv;  // s*I expansion
        } else if (sv != 0.0) {
          std::cerr << "non-zero scalar off-diagonal block\n";
          return 4;
        }
      } else {
        const Mat M = NO::Evaluation::evaluate_matrix(e, env);
        for (size_t a = 0; a < M.size(); ++a)
          for (size_t b = 0; b < M[a].size(); ++b) K[r0 + a][c0 + b] = M[a][b];
      }
      c0 += sizes[bj];
    }
    r0 += sizes[bi];
  }
  Vec b(N);
  for (size_t i = 0; i < N; ++i) b[i] = 2.0 * u01(seed, TAG_B, i, 0) - 1.0;
  auto [L, D] = NO::LinearSolvers::ldlt_decomposition(K);
  Vec x = b;
  NO::LinearSolvers::overwriting_solve_ldlt(L, D, x);
  write_bin(dir + "/" + tag + "_K.bin", lower_packed(K));
  write_bin(dir + "/" + tag + "_D.bin", D);
  write_bin(dir + "/" + tag + "_b.bin", b);
  write_bin(dir + "/" + tag + "_x.bin", x);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: ref_harness <mode> <dir> ...\n";
    return 2;
  }
  const std::string mode = argv[1], dir = argv[2];
  try {
    if (mode == "formulation") return mode_formulation(dir);
    if (mode == "formulation_one" && argc == 5) return mode_formulation_one(argv[2], argv[3], argv[4]);
    if (mode == "formulation_one" && argc == 6) return mode_formulation_one(argv[2], argv[3], argv[4], argv[5]);
    if (mode == "ldlt" && argc == 6) return mode_ldlt(dir, std::stoul(argv[3]), std::stoull(argv[4]), argv[5]);
    if (mode == "bk" && argc == 6) return mode_bk(dir, std::stoul(argv[3]), std::stoull(argv[4]), argv[5]);
    if (mode == "bk_zeros_at" && argc == 7)
      return mode_bk_zeros_at(dir, std::stoul(argv[3]), std::stoull(argv[4]), argv[5], argv[6]);
    if (mode == "bk_file" && argc == 5) return mode_bk_file(dir, std::stoul(argv[3]), argv[4]);
    if (mode == "bk_rand" && argc == 7)
      return mode_bk_rand(dir, std::stoul(argv[3]), std::stoull(argv[4]), std::stoul(argv[5]), argv[6]);
    if (mode == "newton" && argc == 8)
      return mode_newton(dir, std::stoul(argv[3]), std::stoul(argv[4]), std::stoull(argv[5]), std::stoi(argv[6]),
                         argv[7]);
    if (mode == "newton" && argc == 11)  // + <ineq handling> <inequality bounds> <variable bounds>
      return mode_newton(dir, std::stoul(argv[3]), std::stoul(argv[4]), std::stoull(argv[5]), std::stoi(argv[6]),
                         argv[7], argv[8], argv[9], argv[10]);
    if (mode == "newton" && argc == 13)  // + <p> <equality handling>
      return mode_newton(dir, std::stoul(argv[3]), std::stoul(argv[4]), std::stoull(argv[5]), std::stoi(argv[6]),
                         argv[7], argv[8], argv[9], argv[10], std::stoul(argv[11]), argv[12]);
    if (mode == "component_eq" && argc == 8)
      return mode_component_eq(dir, std::stoul(argv[3]), std::stoul(argv[4]), std::stoul(argv[5]),
                               std::stoull(argv[6]), argv[7]);
  } catch (const std::exception& e) {
    std::cerr << "reference threw: " << e.what() << "\n";
    return 3;
  }
  std::cerr << "bad arguments\n";
  return 2;
}
