// Conditional sums of sample columns on the device (include/probabilit_hip.h, "summaries of
// samples"):
//
//   pbh_binned_sums    per bin of column i's edges the number of rows, sum(y - c) and sum((y - c)^2)
//                      of column j, for a list of (i, j) pairs in one launch: what
//                      scipy.stats.binned_statistic's count / sum / mean / std and the correlation
//                      ratio are finished from
//
// An HBM-bound sweep like pbh_histogram2d: 16 B per row per pair read, nothing written per row.
#include <math.h>
#include <stddef.h>

#include "pbh_bins.h"
#include "pbh_error.h"
#include "pbh_summary.h"

namespace pbh {
namespace {

constexpr int kBinnedMaxBins = PBH_BINNED_MAX_BINS;
constexpr int kBinnedMaxCols = PBH_BINNED_MAX_COLUMNS;
constexpr int kBinnedMaxPairs = PBH_BINNED_MAX_PAIRS;

// the tables behind the edges in the workspace, all of fixed size
struct BinnedTables {
  const double* cols[kBinnedMaxCols];
  double centres[kBinnedMaxCols];
  int32_t bins[kBinnedMaxCols];
  int32_t pairs[2 * kBinnedMaxPairs];
  uint8_t uniform[kBinnedMaxCols];
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}

template <bool UX>
__device__ __forceinline__ void binned_sweep(const double* __restrict__ x, const double* __restrict__ y, int64_t n,
                                             const double* e, int m, double c, uint32_t* cnt, double* s1, double* s2) {
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const double lo = e[0], hi = e[m];
  const double scale = (double)m / (hi - lo);
  const int64_t tiles = (n + kSumTile - 1) / kSumTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kSumTile + t;
    double xv[kSumItems], yv[kSumItems];
#pragma unroll
    for (int j = 0; j < kSumItems; ++j) {
      const int64_t i = base + (int64_t)j * kSumThreads;
      xv[j] = i < n ? x[i] : NAN;
      yv[j] = i < n ? y[i] : NAN;
    }
#pragma unroll
    for (int j = 0; j < kSumItems; ++j) {
      const double a = xv[j];
      const bool in = a >= lo && a <= hi;  // false for NaN
      int b = 0;
      if (in) b = joint_bin<UX>(e, m, lo, scale, a);
      const double d = yv[j] - c, q = d * d;  // (-ffp-contract=off: the square rounds once)
      const uint64_t active = __ballot(in);
      if (active == 0ull) continue;  // wave-uniform
      const int leader = __builtin_ctzll(active);
      const int b0 = __shfl(b, leader, kWave);
      if (__ballot(in && b == b0) == active) {  // a constant binning column, or one bin for the wave's rows
        const double w1 = wave_sum(in ? d : 0.0), w2 = wave_sum(in ? q : 0.0);
        if (lane == leader) {
          atomicAdd(&cnt[b0], (uint32_t)__popcll(active));
          unsafeAtomicAdd(&s1[b0], w1);
          unsafeAtomicAdd(&s2[b0], w2);
        }
      } else if (in) {
        atomicAdd(&cnt[b], 1u);
        unsafeAtomicAdd(&s1[b], d);
        unsafeAtomicAdd(&s2[b], q);
      }
    }
  }
}

// grid (row tiles, pairs): a block sums its tiles of one pair into m 32-bit LDS counters (n < 2^32
// rows: none wraps) and 2 m LDS doubles, and adds the non-empty bins to the pair's output.
__global__ __launch_bounds__(kSumThreads) void k_binned_sums(const BinnedTables* __restrict__ tb, int64_t n,
                                                             const double* __restrict__ edges,
                                                             unsigned long long* __restrict__ counts,
                                                             double* __restrict__ sum1, double* __restrict__ sum2) {
  extern __shared__ double dyn[];  // edges (m + 1), s1 (m), s2 (m), then m uint32 counters
  const int p = blockIdx.y, t = threadIdx.x;
  const int ci = tb->pairs[2 * p], cj = tb->pairs[2 * p + 1];
  const int m = tb->bins[ci];
  int eoff = 0, ooff = 0;  // (uniform over the block: scalar loops)
  for (int c = 0; c < ci; ++c) eoff += tb->bins[c] ? tb->bins[c] + 1 : 0;
  for (int q = 0; q < p; ++q) ooff += tb->bins[tb->pairs[2 * q]];
  double* e = dyn;
  double* s1 = dyn + m + 1;
  double* s2 = s1 + m;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(s2 + m);
  for (int i = t; i <= m; i += kSumThreads) e[i] = edges[eoff + i];
  for (int i = t; i < m; i += kSumThreads) {
    s1[i] = 0.0;
    s2[i] = 0.0;
    cnt[i] = 0;
  }
  __syncthreads();
  const double* __restrict__ x = tb->cols[ci];
  const double* __restrict__ y = tb->cols[cj];
  const double c = tb->centres[cj];
  if (tb->uniform[ci] != 0)
    binned_sweep<true>(x, y, n, e, m, c, cnt, s1, s2);
  else
    binned_sweep<false>(x, y, n, e, m, c, cnt, s1, s2);
  __syncthreads();
  for (int i = t; i < m; i += kSumThreads)
    if (cnt[i]) {
      atomicAdd(&counts[ooff + i], (unsigned long long)cnt[i]);
      unsafeAtomicAdd(&sum1[ooff + i], s1[i]);
      unsafeAtomicAdd(&sum2[ooff + i], s2[i]);
    }
}

int check_bins(const char* what, int32_t k, const int32_t* bins_host, size_t* edge_count) {
  PBH_REQUIRE(k >= 1 && k <= kBinnedMaxCols, "%s: k = %d columns is outside [1, %d]", what, (int)k, kBinnedMaxCols);
  PBH_REQUIRE(bins_host != nullptr, "%s: bins is NULL", what);
  size_t total = 0;
  for (int c = 0; c < k; ++c) {  // 0 bins: a column that only gives values, without edges
    PBH_REQUIRE(bins_host[c] >= 0 && bins_host[c] <= kBinnedMaxBins, "%s: bins[%d] = %d is outside [0, %d]", what, c,
                (int)bins_host[c], kBinnedMaxBins);
    total += bins_host[c] ? (size_t)bins_host[c] + 1 : 0;
  }
  *edge_count = total;
  return PBH_OK;
}

}  // namespace
}  // namespace pbh

using namespace pbh;

extern "C" int pbh_binned_sums_workspace_size(int32_t k, const int32_t* bins_host, size_t* bytes) {
  PBH_REQUIRE(bytes != nullptr, "pbh_binned_sums_workspace_size: bytes is NULL");
  size_t total = 0;
  if (int st = check_bins("pbh_binned_sums_workspace_size", k, bins_host, &total)) return st;
  *bytes = total * sizeof(double) + sizeof(BinnedTables);
  return PBH_OK;
}

extern "C" int pbh_binned_sums(const double* const* cols_host, int32_t k, int64_t n, const double* edges_host,
                               const int32_t* bins_host, const uint8_t* uniform_host, const double* centres_host,
                               const int32_t* pairs_host, int32_t npairs, int64_t* counts, double* s1, double* s2,
                               void* ws, size_t ws_bytes, void* stream) {
  const char* what = "pbh_binned_sums";
  PBH_REQUIRE(cols_host && edges_host && bins_host && uniform_host && centres_host && pairs_host && counts && s1 &&
                  s2 && ws,
              "%s: cols / edges / bins / uniform / centres / pairs / counts / s1 / s2 / ws is NULL", what);
  size_t total = 0;
  if (int st = check_bins(what, k, bins_host, &total)) return st;
  PBH_REQUIRE(n >= 1, "%s: n = %lld; a conditional sum needs at least one sample", what, (long long)n);
  PBH_REQUIRE(n < ((int64_t)1 << 32), "%s: n = %lld; a block's counters are 32-bit", what, (long long)n);
  for (int c = 0; c < k; ++c)
    PBH_REQUIRE(cols_host[c] != nullptr && ((uintptr_t)cols_host[c] & 7) == 0,
                "%s: column %d is NULL or not 8-byte aligned", what, c);
  PBH_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: ws must be 8-byte aligned", what);
  PBH_REQUIRE(npairs >= 1 && npairs <= kBinnedMaxPairs, "%s: npairs = %d is outside [1, %d]", what, (int)npairs,
              kBinnedMaxPairs);
  const double* e = edges_host;
  for (int c = 0; c < k; ++c) {
    const int b = bins_host[c];
    if (b == 0) continue;
    for (int i = 0; i <= b; ++i) PBH_REQUIRE(isfinite(e[i]), "%s: edge %d of column %d is not finite", what, i, c);
    for (int i = 0; i < b; ++i)
      PBH_REQUIRE(e[i] <= e[i + 1], "%s: column %d: edges[%d] > edges[%d]", what, c, i, i + 1);
    PBH_REQUIRE(e[0] < e[b], "%s: column %d: the range [%g, %g] is not increasing", what, c, e[0], e[b]);
    e += b + 1;
  }
  for (int c = 0; c < k; ++c) PBH_REQUIRE(isfinite(centres_host[c]), "%s: centre %d is not finite", what, c);
  size_t all_bins = 0, lds = 0;
  for (int p = 0; p < npairs; ++p) {
    const int i = pairs_host[2 * p], j = pairs_host[2 * p + 1];
    PBH_REQUIRE(i >= 0 && i < k && j >= 0 && j < k, "%s: pair %d = (%d, %d) is outside [0, %d)", what, p, i, j, (int)k);
    PBH_REQUIRE(bins_host[i] >= 1, "%s: pair %d bins by column %d, which has no bins", what, p, i);
    all_bins += (size_t)bins_host[i];
    const size_t need_lds = ((size_t)bins_host[i] + 1) * sizeof(double) +
                            (size_t)bins_host[i] * (2 * sizeof(double) + sizeof(uint32_t));
    lds = need_lds > lds ? need_lds : lds;  // at most 8200 + 20480 B
  }
  const size_t need = total * sizeof(double) + sizeof(BinnedTables);
  if (ws_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
    return PBH_ERR_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  double* edges_dev = (double*)ws;
  char* tb = (char*)ws + total * sizeof(double);
  PBH_CHECK_HIP(hipMemcpyAsync(edges_dev, edges_host, total * sizeof(double), hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(BinnedTables, cols), cols_host, (size_t)k * sizeof(double*),
                               hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(BinnedTables, centres), centres_host, (size_t)k * sizeof(double),
                               hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(BinnedTables, bins), bins_host, (size_t)k * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(BinnedTables, pairs), pairs_host, (size_t)npairs * 2 * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(BinnedTables, uniform), uniform_host, (size_t)k, hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemsetAsync(counts, 0, all_bins * sizeof(int64_t), s));
  PBH_CHECK_HIP(hipMemsetAsync(s1, 0, all_bins * sizeof(double), s));
  PBH_CHECK_HIP(hipMemsetAsync(s2, 0, all_bins * sizeof(double), s));
  hipLaunchKernelGGL(k_binned_sums, dim3((unsigned)summary_blocks(n), (unsigned)npairs), dim3(kSumThreads), lds, s,
                     (const BinnedTables*)tb, n, (const double*)edges_dev, (unsigned long long*)counts, s1, s2);
  PBH_CHECK_LAUNCH();
  return PBH_OK;
}
