// TEST HARNESS: the per-row functions of probabilit_amd/csrc/pbh_mvar.h compiled for the HOST
// (they are __host__ __device__), so that tests/test_multivariate_host.py can compare them with
// scipy on the CPU, on uniforms numpy supplies.  This never ships in the product library; the
// kernels that run the same functions are checked by tests/test_gpu_multivariate.py.
#include <vector>

#include "pbh_mvar.h"

using namespace pbh;

extern "C" {

// the counter-based uniforms of the samplers: u (n, d) row-major
void mvh_uniforms(unsigned long long seed, long row0, long n, int d, double* u) {
  const Philox ph(seed);
  for (long i = 0; i < n; ++i)
    for (int j = 0; j < d; ++j) u[i * d + j] = mvar::uniform_at(ph, (uint64_t)(row0 + i), (uint32_t)j);
}

// u, out: (n, d) row-major; A: (d, d) row-major
void mvh_mvn(const double* mean, const double* A, int d, const double* u, long n, double* out) {
  const int dp = mvar::mvn_ld(d);
  std::vector<double> At((size_t)d * dp, 0.0), m((size_t)dp, 0.0), z((size_t)d);
  for (int c = 0; c < d; ++c) {
    m[c] = mean[c];
    for (int j = 0; j < d; ++j) At[(size_t)j * dp + c] = A[(size_t)c * d + j];
  }
  for (long i = 0; i < n; ++i) {
    for (int j = 0; j < d; ++j) z[j] = sf::ppnd16(u[i * d + j]);
    mvar::mvn_row(m.data(), At.data(), d, z.data(), 1, out + i * d, 1);
  }
}

// guided != 0: every component reads a guide built on the host as the device builds it.
// bad[i] = 1 for a row whose sum is 0 or not finite.
void mvh_dirichlet(const double* alpha, int d, int guided, const double* u, long n, double* out, int* bad) {
  const int m = sf::kGammaGuideM;
  std::vector<std::vector<double>> tabs((size_t)d);
  std::vector<mvar::GammaComp> comp((size_t)d);
  for (int j = 0; j < d; ++j) {
    const double a = alpha[j];
    const double* guide = nullptr;
    if (guided) {
      std::vector<double>& tb = tabs[j];
      tb.assign(4 * (size_t)m, 0.0);
      sf::GammaGuide T{tb.data(), tb.data() + m, tb.data() + 2 * m, tb.data() + 3 * m, m, sf::kGammaGuideZ0,
                       sf::kGammaGuideH, 1.0 / sf::kGammaGuideH};
      for (int k = 0; k < m; ++k) sf::gamma_guide_entry(a, T.z0 + k * T.h, &tb[k], &tb[m + k], &tb[2 * m + k]);
      for (int k = 0; k < m; ++k) tb[3 * m + k] = k < m - 1 ? sf::gamma_guide_check(a, T, k) : 0.0;
      guide = tb.data();
    }
    comp[j] = mvar::GammaComp{a, sf::gamma_aux(a), guide};
  }
  std::vector<double> g((size_t)d);
  for (long i = 0; i < n; ++i) {
    const double* ui = u + i * d;
    bad[i] = mvar::dirichlet_row([ui](int j) { return ui[j]; }, comp.data(), d, g.data(), 1, out + i * d, 1) ? 1 : 0;
  }
}

void mvh_multinomial(double trials, const double* pc, int d, const double* u, long n, long long* out) {
  for (long i = 0; i < n; ++i) {
    const double* ui = u + i * d;
    mvar::multinomial_row([ui](int j) { return ui[j]; }, trials, pc, d, (int64_t*)(out + i * d), 1);
  }
}
}
