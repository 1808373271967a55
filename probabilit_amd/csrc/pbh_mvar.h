// Per-row math of the multivariate samplers (multivariate_normal, dirichlet, multinomial), host-
// and device-callable: the kernels of pbh_mvar.hip and the host build of
// tests/native/multivariate_host.cpp run these same functions.
//
// The reference draws the three with scipy.stats.<name>(...).rvs(size=N, random_state=seed)
// (modeling.py:806-812): numpy's legacy MT19937 samplers.  Here each is a per-row composition of
// inverse CDFs the library already gates against scipy, on the counter-based uniforms
//     u(i, j) = Philox(seed).uniform(row0 + i, j, kPurposeUniform)      (pbh_fill_uniform's),
// with u == 0 replaced by 2^-53: the same law, a different stream.
//
//   multivariate_normal  x_c = mean_c + sum_j A[c, j] z_j, z_j = ppnd16(u_j) (the norm ppf kernel's
//                        quantile), A = V diag(sqrt(max(lambda, 0))) of eigh(cov) from the host
//   dirichlet            g_j = igami(alpha_j, u_j) (through the gamma guide when the component has
//                        one), x_j = g_j / sum_k g_k
//   multinomial          the chain of conditional binomials: rem = n; for j < d - 1
//                        x_j = binom_ppf01(u_j, rem, pc_j), rem -= x_j; x_{d-1} = rem, with
//                        pc_j = p_j / (1 - sum_{k<j} p_k) from the host
#pragma once

#include "pbh_rng.h"
#include "pbh_special.h"
#include "pbh_special_ext.h"

namespace pbh {
namespace mvar {

constexpr int kMaxD = 128;  // components (correlation.MAX_VARIABLES)

PBH_HD inline double uniform_at(const Philox& ph, uint64_t row, uint32_t col) {
  const double u = ph.uniform(row, col, kPurposeUniform);
  return u == 0.0 ? 0x1.0p-53 : u;
}

// ---------------------------------------------------------------- multivariate_normal
// The factor is passed transposed and padded, At[j * dp + c] = A[c, j] with dp = mvn_ld(d) and
// zeros in the padding, so that a block of kMvnBlock outputs reads kMvnBlock consecutive entries
// per z_j (every lane the same address: a broadcast) and forms them with one read of z_j.
constexpr int kMvnBlock = 8;
PBH_HD inline int mvn_ld(int d) { return (d + kMvnBlock - 1) / kMvnBlock * kMvnBlock; }

// one row: z[j * zs] the row's normals, out[c * os] its d outputs.  The sum runs over j = 0 .. d - 1
// in order with fused multiply-adds, whatever the launch geometry.
PBH_HD inline bool mvn_row(const double* __restrict__ mean, const double* __restrict__ At, int d,
                           const double* __restrict__ z, int64_t zs, double* __restrict__ out, int64_t os) {
  const int dp = mvn_ld(d);
  bool bad = false;
  for (int c0 = 0; c0 < d; c0 += kMvnBlock) {
    double acc[kMvnBlock];
#pragma unroll
    for (int k = 0; k < kMvnBlock; ++k) acc[k] = c0 + k < d ? mean[c0 + k] : 0.0;
    for (int j = 0; j < d; ++j) {
      const double zj = z[(int64_t)j * zs];
      const double* a = At + (int64_t)j * dp + c0;
#pragma unroll
      for (int k = 0; k < kMvnBlock; ++k) acc[k] = __builtin_fma(a[k], zj, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < kMvnBlock; ++k) {
      if (c0 + k < d) {
        out[(int64_t)(c0 + k) * os] = acc[k];
        bad |= !isfinite(acc[k]);
      }
    }
  }
  return bad;
}

// ---------------------------------------------------------------- dirichlet
struct GammaComp {      // one component: its shape, igami's hoisted constants and its guide table
  double a;
  sf::GammaAux aux;
  const double* guide;  // 4 x sf::kGammaGuideM doubles (y, d1, d2, ok), NULL: plain igami
};

PBH_HD inline double gamma_of(const GammaComp& c, double u) {
  if (!c.guide) return sf::igami(c.a, u);
  const int m = sf::kGammaGuideM;
  const sf::GammaGuide T{c.guide, c.guide + m, c.guide + 2 * m, c.guide + 3 * m, m, sf::kGammaGuideZ0,
                         sf::kGammaGuideH, 1.0 / sf::kGammaGuideH};
  return sf::igami_guided<true>(c.a, u, &c.aux, T);
}

// one row: g[j * gs] holds the row's gamma draws between the two passes, out[j * os] = g_j / sum.
// true when the sum is 0 or not finite (the row is then not a point of the simplex).
template <class U>
PBH_HD inline bool dirichlet_row(U&& u, const GammaComp* __restrict__ comp, int d, double* __restrict__ g, int64_t gs,
                                 double* __restrict__ out, int64_t os) {
  double sum = 0.0;
  for (int j = 0; j < d; ++j) {
    const double gj = gamma_of(comp[j], u(j));
    g[(int64_t)j * gs] = gj;
    sum += gj;
  }
  for (int j = 0; j < d; ++j) out[(int64_t)j * os] = g[(int64_t)j * gs] / sum;
  return !(sum > 0.0 && isfinite(sum));
}

// ---------------------------------------------------------------- multinomial
template <class U>
PBH_HD inline void multinomial_row(U&& u, double n, const double* __restrict__ pc, int d, int64_t* __restrict__ out,
                                   int64_t os) {
  double rem = n;
  for (int j = 0; j < d - 1; ++j) {
    double k = 0.0;
    if (rem > 0.0) {
      const double p = pc[j];
      k = p == 0.0 ? 0.0 : p == 1.0 ? rem : sfx::binom_ppf01(u(j), rem, p);
    }
    out[(int64_t)j * os] = (int64_t)k;
    rem -= k;
  }
  out[(int64_t)(d - 1) * os] = (int64_t)rem;
}

}  // namespace mvar
}  // namespace pbh
