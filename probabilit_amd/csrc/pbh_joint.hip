// Joint histograms of sample columns on the device (include/probabilit_hip.h, "summaries of
// samples"):
//
//   pbh_histogram2d    np.histogram2d(x_i, x_j, bins=(edges_i, edges_j))[0] for a list of column
//                      pairs (numpy lib/_histograms_impl.py histogramdd) in one launch
//
// An HBM-bound sweep like pbh_histogram: 16 B per row per pair read, nothing written per row.
#include <math.h>
#include <stddef.h>

#include "pbh_bins.h"
#include "pbh_error.h"
#include "pbh_summary.h"

namespace pbh {
namespace {

constexpr int kJointMaxBins = PBH_HISTOGRAM2D_MAX_BINS;
constexpr int kJointMaxCells = PBH_HISTOGRAM2D_MAX_CELLS;
constexpr int kJointMaxCols = PBH_HISTOGRAM2D_MAX_COLUMNS;
constexpr int kJointMaxPairs = PBH_HISTOGRAM2D_MAX_PAIRS;

// the tables behind the edges in the workspace, all of fixed size
struct JointTables {
  const double* cols[kJointMaxCols];
  int32_t bins[kJointMaxCols];
  int32_t pairs[2 * kJointMaxPairs];
  uint8_t uniform[kJointMaxCols];
};

template <bool UX, bool UY>
__device__ __forceinline__ void joint_sweep(const double* __restrict__ x, const double* __restrict__ y, int64_t n,
                                            const double* ex, int bx, const double* ey, int by, uint32_t* cnt) {
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const double xlo = ex[0], xhi = ex[bx], ylo = ey[0], yhi = ey[by];
  const double xscale = (double)bx / (xhi - xlo), yscale = (double)by / (yhi - ylo);
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
      const double a = xv[j], b = yv[j];
      const bool in = a >= xlo && a <= xhi && b >= ylo && b <= yhi;  // false for NaN
      int cell = 0;
      if (in) cell = joint_bin<UX>(ex, bx, xlo, xscale, a) * by + joint_bin<UY>(ey, by, ylo, yscale, b);
      const uint64_t active = __ballot(in);
      if (active == 0ull) continue;  // wave-uniform
      const int leader = __builtin_ctzll(active);
      const int c0 = __shfl(cell, leader, kWave);
      if (__ballot(in && cell == c0) == active) {  // constant or perfectly correlated columns
        if (lane == leader) atomicAdd(&cnt[c0], (uint32_t)__popcll(active));
      } else if (in) {
        atomicAdd(&cnt[cell], 1u);
      }
    }
  }
}

// grid (row tiles, pairs): a block counts its tiles of one pair into bx * by 32-bit LDS counters
// (n < 2^32 rows: none wraps) and adds the non-empty ones to the pair's matrix.
__global__ __launch_bounds__(kSumThreads) void k_histogram2d(const JointTables* __restrict__ tb, int64_t n,
                                                             const double* __restrict__ edges,
                                                             unsigned long long* __restrict__ counts) {
  extern __shared__ double dyn[];  // x edges (bx + 1), y edges (by + 1), then bx * by uint32 counters
  const int p = blockIdx.y, t = threadIdx.x;
  const int ci = tb->pairs[2 * p], cj = tb->pairs[2 * p + 1];
  const int bx = tb->bins[ci], by = tb->bins[cj], cells = bx * by;
  int offi = 0, offj = 0;  // (uniform over the block: scalar loops)
  for (int c = 0; c < ci; ++c) offi += tb->bins[c] + 1;
  for (int c = 0; c < cj; ++c) offj += tb->bins[c] + 1;
  int64_t coff = 0;
  for (int q = 0; q < p; ++q) coff += (int64_t)tb->bins[tb->pairs[2 * q]] * tb->bins[tb->pairs[2 * q + 1]];
  double* ex = dyn;
  double* ey = dyn + bx + 1;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(dyn + bx + by + 2);
  for (int i = t; i <= bx; i += kSumThreads) ex[i] = edges[offi + i];
  for (int i = t; i <= by; i += kSumThreads) ey[i] = edges[offj + i];
  for (int i = t; i < cells; i += kSumThreads) cnt[i] = 0;
  __syncthreads();
  const double* __restrict__ x = tb->cols[ci];
  const double* __restrict__ y = tb->cols[cj];
  const bool ux = tb->uniform[ci] != 0, uy = tb->uniform[cj] != 0;
  if (ux && uy)
    joint_sweep<true, true>(x, y, n, ex, bx, ey, by, cnt);
  else if (ux)
    joint_sweep<true, false>(x, y, n, ex, bx, ey, by, cnt);
  else if (uy)
    joint_sweep<false, true>(x, y, n, ex, bx, ey, by, cnt);
  else
    joint_sweep<false, false>(x, y, n, ex, bx, ey, by, cnt);
  __syncthreads();
  unsigned long long* out = counts + coff;
  for (int i = t; i < cells; i += kSumThreads)
    if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
}

int check_bins(const char* what, int32_t k, const int32_t* bins_host, size_t* edge_count) {
  PBH_REQUIRE(k >= 2 && k <= kJointMaxCols, "%s: k = %d columns is outside [2, %d]", what, (int)k, kJointMaxCols);
  PBH_REQUIRE(bins_host != nullptr, "%s: bins is NULL", what);
  size_t total = 0;
  for (int c = 0; c < k; ++c) {
    PBH_REQUIRE(bins_host[c] >= 1 && bins_host[c] <= kJointMaxBins, "%s: bins[%d] = %d is outside [1, %d]", what, c,
                (int)bins_host[c], kJointMaxBins);
    total += (size_t)bins_host[c] + 1;
  }
  *edge_count = total;
  return PBH_OK;
}

}  // namespace
}  // namespace pbh

using namespace pbh;

extern "C" int pbh_histogram2d_workspace_size(int32_t k, const int32_t* bins_host, size_t* bytes) {
  PBH_REQUIRE(bytes != nullptr, "pbh_histogram2d_workspace_size: bytes is NULL");
  size_t total = 0;
  if (int st = check_bins("pbh_histogram2d_workspace_size", k, bins_host, &total)) return st;
  *bytes = total * sizeof(double) + sizeof(JointTables);
  return PBH_OK;
}

extern "C" int pbh_histogram2d(const double* const* cols_host, int32_t k, int64_t n, const double* edges_host,
                               const int32_t* bins_host, const uint8_t* uniform_host, const int32_t* pairs_host,
                               int32_t npairs, int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "pbh_histogram2d";
  PBH_REQUIRE(cols_host && edges_host && bins_host && uniform_host && pairs_host && counts && ws,
              "%s: cols / edges / bins / uniform / pairs / counts / ws is NULL", what);
  size_t total = 0;
  if (int st = check_bins(what, k, bins_host, &total)) return st;
  PBH_REQUIRE(n >= 1, "%s: n = %lld; a histogram needs at least one sample", what, (long long)n);
  PBH_REQUIRE(n < ((int64_t)1 << 32), "%s: n = %lld; a block's counters are 32-bit", what, (long long)n);
  for (int c = 0; c < k; ++c)
    PBH_REQUIRE(cols_host[c] != nullptr && ((uintptr_t)cols_host[c] & 7) == 0,
                "%s: column %d is NULL or not 8-byte aligned", what, c);
  PBH_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: ws must be 8-byte aligned", what);
  PBH_REQUIRE(npairs >= 1 && npairs <= kJointMaxPairs, "%s: npairs = %d is outside [1, %d]", what, (int)npairs,
              kJointMaxPairs);
  const double* e = edges_host;
  for (int c = 0; c < k; ++c) {
    const int b = bins_host[c];
    for (int i = 0; i <= b; ++i) PBH_REQUIRE(isfinite(e[i]), "%s: edge %d of column %d is not finite", what, i, c);
    for (int i = 0; i < b; ++i)
      PBH_REQUIRE(e[i] <= e[i + 1], "%s: column %d: edges[%d] > edges[%d]", what, c, i, i + 1);
    PBH_REQUIRE(e[0] < e[b], "%s: column %d: the range [%g, %g] is not increasing", what, c, e[0], e[b]);
    e += b + 1;
  }
  size_t all_cells = 0, lds = 0;
  for (int p = 0; p < npairs; ++p) {
    const int i = pairs_host[2 * p], j = pairs_host[2 * p + 1];
    PBH_REQUIRE(i >= 0 && i < k && j >= 0 && j < k, "%s: pair %d = (%d, %d) is outside [0, %d)", what, p, i, j, (int)k);
    PBH_REQUIRE(i != j, "%s: pair %d = (%d, %d) names one column twice", what, p, i, j);
    const size_t cells = (size_t)bins_host[i] * bins_host[j];
    PBH_REQUIRE(cells <= (size_t)kJointMaxCells, "%s: pair %d has %d x %d = %zu cells; at most %d", what, p,
                (int)bins_host[i], (int)bins_host[j], cells, kJointMaxCells);
    all_cells += cells;
    const size_t need_lds = ((size_t)bins_host[i] + bins_host[j] + 2) * sizeof(double) + cells * sizeof(uint32_t);
    lds = need_lds > lds ? need_lds : lds;
  }
  const size_t need = total * sizeof(double) + sizeof(JointTables);
  if (ws_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
    return PBH_ERR_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  double* edges_dev = (double*)ws;
  char* tb = (char*)ws + total * sizeof(double);
  PBH_CHECK_HIP(hipMemcpyAsync(edges_dev, edges_host, total * sizeof(double), hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(JointTables, cols), cols_host, (size_t)k * sizeof(double*),
                               hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(JointTables, bins), bins_host, (size_t)k * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(JointTables, pairs), pairs_host, (size_t)npairs * 2 * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemcpyAsync(tb + offsetof(JointTables, uniform), uniform_host, (size_t)k, hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemsetAsync(counts, 0, all_cells * sizeof(int64_t), s));
  if (lds > 65536)  // 64 KiB of counters and the edges: above the default dynamic LDS limit, below the CU's 160 KiB
    PBH_CHECK_HIP(hipFuncSetAttribute((const void*)k_histogram2d, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_histogram2d, dim3((unsigned)summary_blocks(n), (unsigned)npairs), dim3(kSumThreads), lds, s,
                     (const JointTables*)tb, n, (const double*)edges_dev, (unsigned long long*)counts);
  PBH_CHECK_LAUNCH();
  return PBH_OK;
}
