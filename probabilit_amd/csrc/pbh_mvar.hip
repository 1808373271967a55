// Fused samplers of the multivariate distributions (pbh_mvar.h): one launch draws a row's
// uniforms in registers (Philox, counter-addressed by the global row), forms the row's d
// components and writes them, 8 B per element -- no stored uniforms, no N-sized workspace, no second
// N-sized pass.  One thread owns one row, so every column store is coalesced across the wave.
//
// A row's d intermediate values (the normals z_j, the gamma draws g_j) do not fit registers for
// d up to 128, so a block keeps a tile of R rows x d of them in LDS, laid out [j][r]: lane r reads and
// writes only its own column (consecutive 8-byte words across the wave: conflict-free, and no
// barrier between the passes).  multivariate_normal stages the factor (transposed and padded,
// mvn_ld) behind the tile, where every lane reads the same entry (a broadcast); a factor too
// large for the budget (d > 64) stays in global memory, read through wave-uniform addresses.
// R is the largest multiple of 64 up to 256 with tile + factor <= 64 KiB, so two workgroups
// always fit a CU's 160 KiB; blocks stride over the tiles, so the factor is staged once per block.
// FP64-VALU bound: ppnd16 / igami / binom_ppf01 per element, plus d FMAs for the normal.
#include <math.h>

#include <map>
#include <vector>

#include "pbh_error.h"
#include "pbh_mvar.h"
#include "pbh_ppf_ext.h"

namespace pbh {
namespace {

constexpr int kMvarLds = 64 * 1024;
constexpr int kMvarMaxBlock = 256;

template <bool A_LDS>
__global__ void __launch_bounds__(kMvarMaxBlock)
    k_mvn(uint64_t seed, int64_t row0, int64_t nrows, int d, const double* __restrict__ mean,
          const double* __restrict__ At, double* __restrict__ out, int64_t ld, int32_t* __restrict__ flag) {
  extern __shared__ double lds[];
  const int R = blockDim.x, tid = threadIdx.x;
  double* z = lds;  // [d][R]
  const double* at = At;
  if constexpr (A_LDS) {
    double* as = lds + (size_t)d * R;  // [d][mvn_ld(d)]
    const int na = d * mvar::mvn_ld(d);
    for (int k = tid; k < na; k += R) as[k] = At[k];
    __syncthreads();
    at = as;
  }
  const Philox ph(seed);
  const int64_t ntiles = (nrows + R - 1) / R;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i = t * R + tid;
    bool bad = false;
    if (i < nrows) {
      for (int j = 0; j < d; ++j) z[(size_t)j * R + tid] = sf::ppnd16(mvar::uniform_at(ph, (uint64_t)(row0 + i), (uint32_t)j));
      bad = mvar::mvn_row(mean, at, d, z + tid, R, out + i, ld);
    }
    flag_nonfinite(flag, bad);
  }
}

__global__ void __launch_bounds__(kMvarMaxBlock)
    k_dirichlet(uint64_t seed, int64_t row0, int64_t nrows, int d, const mvar::GammaComp* __restrict__ comp,
                double* __restrict__ out, int64_t ld, int32_t* __restrict__ flag) {
  extern __shared__ double lds[];  // g: [d][R]
  const int R = blockDim.x, tid = threadIdx.x;
  const Philox ph(seed);
  const int64_t ntiles = (nrows + R - 1) / R;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i = t * R + tid;
    bool bad = false;
    if (i < nrows) {
      const uint64_t row = (uint64_t)(row0 + i);
      bad = mvar::dirichlet_row([&](int j) { return mvar::uniform_at(ph, row, (uint32_t)j); }, comp, d, lds + tid, R,
                                out + i, ld);
    }
    flag_nonfinite(flag, bad);
  }
}

__global__ void __launch_bounds__(kMvarMaxBlock)
    k_multinomial(uint64_t seed, int64_t row0, int64_t nrows, int d, double n, const double* __restrict__ pc,
                  int64_t* __restrict__ out, int64_t ld) {
  const Philox ph(seed);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t row = (uint64_t)(row0 + i);
    mvar::multinomial_row([&](int j) { return mvar::uniform_at(ph, row, (uint32_t)j); }, n, pc, d, out + i, ld);
  }
}

// rows per block: the largest multiple of 64 up to kMvarMaxBlock whose tile fits beside `fixed` bytes
int tile_rows(int d, size_t fixed) {
  const size_t per_row = (size_t)d * sizeof(double);
  int R = (int)((kMvarLds - fixed) / per_row / kWave) * kWave;
  return R > kMvarMaxBlock ? kMvarMaxBlock : R;
}

// a stream-ordered device copy of a host table (freed stream-ordered, after the launch).  The
// host side is the caller's (or this call's) pageable memory, so the copy is waited for: the
// table is a few KiB and the Python layer has just read q[0] on this stream anyway.
int upload(const void* host, size_t bytes, Scratch<void>& dev, hipStream_t s) {
  PBH_CHECK_HIP(dev.get(bytes, s));
  hipError_t e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    dev.reset();
    set_error("hipMemcpyAsync of a parameter table failed: %s", hipGetErrorString(e));
    return PBH_ERR_HIP;
  }
  return PBH_OK;
}

int check_common(const char* what, int64_t row0, int64_t nrows, int d, const void* out, int64_t ld) {
  PBH_REQUIRE(row0 >= 0 && nrows >= 0, "%s: bad row range", what);
  PBH_REQUIRE(d >= 1 && d <= mvar::kMaxD, "%s: d must be in [1, %d], got %d", what, mvar::kMaxD, d);
  PBH_REQUIRE(ld >= nrows, "%s: ld < nrows", what);
  PBH_REQUIRE(out != nullptr || nrows == 0, "%s: out must not be NULL", what);
  return PBH_OK;
}

unsigned tile_grid(int64_t nrows, int R) { return grid_for(nrows, R, 8192); }

}  // namespace
}  // namespace pbh

using namespace pbh;

extern "C" int pbh_multivariate_normal(uint64_t seed, int64_t row0, int64_t nrows, int32_t d, const double* mean_host,
                                       const double* a_host, double* out, int64_t ld, int32_t* nonfinite_flag,
                                       void* stream) {
  if (int st = check_common("pbh_multivariate_normal", row0, nrows, d, out, ld)) return st;
  PBH_REQUIRE(mean_host && a_host, "pbh_multivariate_normal: mean and A must be host arrays");
  if (nrows == 0) return PBH_OK;
  hipStream_t s = as_stream(stream);
  const int dp = mvar::mvn_ld(d);
  // [mean (dp) | At (d x dp)]: A transposed, zero padding
  std::vector<double> h((size_t)dp + (size_t)d * dp, 0.0);
  for (int c = 0; c < d; ++c) {
    h[c] = mean_host[c];
    for (int j = 0; j < d; ++j) h[(size_t)dp + (size_t)j * dp + c] = a_host[(size_t)c * d + j];
  }
  Scratch<void> dev;
  if (int st = upload(h.data(), h.size() * sizeof(double), dev, s)) return st;
  const double* mean = (const double*)dev.get();
  const double* At = mean + dp;
  const size_t abytes = (size_t)d * dp * sizeof(double);
  const bool a_lds = abytes + (size_t)kWave * d * sizeof(double) <= (size_t)kMvarLds;
  const int R = tile_rows(d, a_lds ? abytes : 0);
  const size_t lds = (size_t)R * d * sizeof(double) + (a_lds ? abytes : 0);
  const dim3 g(tile_grid(nrows, R)), b((unsigned)R);
  if (a_lds)
    hipLaunchKernelGGL(k_mvn<true>, g, b, lds, s, seed, row0, nrows, (int)d, mean, At, out, ld, nonfinite_flag);
  else
    hipLaunchKernelGGL(k_mvn<false>, g, b, lds, s, seed, row0, nrows, (int)d, mean, At, out, ld, nonfinite_flag);
  PBH_CHECK_LAUNCH();
  return PBH_OK;
}

extern "C" int pbh_dirichlet(uint64_t seed, int64_t row0, int64_t nrows, int32_t d, const double* alpha_host,
                             double* out, int64_t ld, int32_t* nonfinite_flag, void* stream) {
  if (int st = check_common("pbh_dirichlet", row0, nrows, d, out, ld)) return st;
  PBH_REQUIRE(alpha_host != nullptr, "pbh_dirichlet: alpha must be a host array");
  for (int j = 0; j < d; ++j)
    PBH_REQUIRE(alpha_host[j] > 0.0 && isfinite(alpha_host[j]), "pbh_dirichlet: alpha[%d] = %g is not positive", j,
                alpha_host[j]);
  if (nrows == 0) return PBH_OK;
  hipStream_t s = as_stream(stream);
  // one guide per distinct shape (the process cache's when it has room); a shape whose guide
  // cannot be had takes plain igami
  std::map<double, TableRef> guides;
  std::vector<mvar::GammaComp> comp((size_t)d);
  for (int j = 0; j < d; ++j) {
    const double a = alpha_host[j];
    auto it = guides.find(a);
    if (it == guides.end()) it = guides.emplace(a, gamma_guide_table(a, s)).first;
    comp[j] = mvar::GammaComp{a, sf::gamma_aux(a), it->second.get()};
  }
  Scratch<void> dev;  // (freed before the guides are given back)
  if (int st = upload(comp.data(), comp.size() * sizeof(mvar::GammaComp), dev, s)) return st;
  const int R = tile_rows(d, 0);
  hipLaunchKernelGGL(k_dirichlet, dim3(tile_grid(nrows, R)), dim3((unsigned)R), (size_t)R * d * sizeof(double), s, seed,
                     row0, nrows, (int)d, (const mvar::GammaComp*)dev.get(), out, ld, nonfinite_flag);
  PBH_CHECK_LAUNCH();
  return PBH_OK;
}

extern "C" int pbh_multinomial(uint64_t seed, int64_t row0, int64_t nrows, int32_t d, double n, const double* pc_host,
                               int64_t* out, int64_t ld, int32_t* nonfinite_flag, void* stream) {
  (void)nonfinite_flag;  // integer outputs: nothing to flag
  if (int st = check_common("pbh_multinomial", row0, nrows, d, out, ld)) return st;
  PBH_REQUIRE(pc_host != nullptr, "pbh_multinomial: pc must be a host array");
  PBH_REQUIRE(n >= 0.0 && n == floor(n) && n <= 0x1.0p53, "pbh_multinomial: n = %g is not a count", n);
  for (int j = 0; j < d; ++j)
    PBH_REQUIRE(pc_host[j] >= 0.0 && pc_host[j] <= 1.0, "pbh_multinomial: pc[%d] = %g is outside [0, 1]", j, pc_host[j]);
  if (nrows == 0) return PBH_OK;
  hipStream_t s = as_stream(stream);
  Scratch<void> dev;
  if (int st = upload(pc_host, (size_t)d * sizeof(double), dev, s)) return st;
  hipLaunchKernelGGL(k_multinomial, dim3(grid_for(nrows, kMvarMaxBlock, 8192)), dim3(kMvarMaxBlock), 0, s, seed, row0,
                     nrows, (int)d, n, (const double*)dev.get(), out, ld);
  PBH_CHECK_LAUNCH();
  return PBH_OK;
}
