// Summaries of sample columns on the device (include/probabilit_hip.h, "summaries of samples"):
//
//   pbh_moments        np.isnan().sum / np.min / np.max / np.mean and the central moments of np.var
//                      (numpy _core/_methods.py _var: the mean first, then the centred sums) and of
//                      scipy.stats.skew / kurtosis (scipy stats/_stats_py.py _moment)
//   pbh_select_ranks   np.sort(x)[ranks], the partition behind np.quantile
//                      (numpy lib/_function_base_impl.py _quantile), as a multi-target radix select
//   pbh_histogram      np.histogram(x, bins, range) for uniform bins (numpy lib/_histograms_impl.py)
//
// All are HBM-bound sweeps over the column(s): 8 B per sample per read, 16 / 32 / 8 B per sample.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "pbh_error.h"
#include "pbh_summary.h"

namespace pbh {
namespace {

// ---------------------------------------------------------------- moments
// Fixed tree over the block's 256 threads: 6 levels inside each wave, 2 over the 4 waves.
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = v + __shfl_xor(v, o, kWave);  // both partners form the same sum
  return v;
}

__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
  v = wave_tree_sum(v);
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// NaN-free min / max of the block (NaNs are counted apart and decide the result at the end)
__device__ __forceinline__ double block_min(double v, double* sh) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const double w = __shfl_xor(v, o, kWave);
    v = w < v ? w : v;
  }
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
  for (int i = 1; i < kSumThreads / kWave; ++i) r = sh[i] < r ? sh[i] : r;
  return r;
}

__device__ __forceinline__ double block_max(double v, double* sh) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const double w = __shfl_xor(v, o, kWave);
    v = w > v ? w : v;
  }
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
  for (int i = 1; i < kSumThreads / kWave; ++i) r = sh[i] > r ? sh[i] : r;
  return r;
}

// slab layout: part[(c * B + b) * 4 + {0..3}]
// first sweep: sum, min, max, nan count; second: sums of d^2, d^3, d^4, d = x - mean
template <int SWEEP>
__global__ __launch_bounds__(kSumThreads) void k_moments(const double* __restrict__ X, int64_t n, int64_t ld,
                                                         const double* __restrict__ out, double* __restrict__ part) {
  __shared__ double sh[kSumThreads / kWave];
  const int c = blockIdx.y, t = threadIdx.x;
  const double* __restrict__ x = X + (int64_t)c * ld;
  const int64_t tiles = (n + kSumTile - 1) / kSumTile;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (SWEEP == 0) {
    a1 = INFINITY;
    a2 = -INFINITY;
  }
  const double mean = SWEEP == 1 ? out[c * PBH_MOMENTS_STRIDE + 3] : 0.0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kSumTile + t;
    double v[kSumItems];
#pragma unroll
    for (int j = 0; j < kSumItems; ++j) {
      const int64_t i = base + (int64_t)j * kSumThreads;
      v[j] = i < n ? x[i] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < kSumItems; ++j) {
      const int64_t i = base + (int64_t)j * kSumThreads;
      if (i < n) {
        if (SWEEP == 0) {
          a0 = a0 + v[j];
          a1 = v[j] < a1 ? v[j] : a1;
          a2 = v[j] > a2 ? v[j] : a2;
          a3 = a3 + (v[j] != v[j] ? 1.0 : 0.0);
        } else {
          const double d = v[j] - mean;
          const double d2 = d * d;
          a0 = a0 + d2;
          a1 = a1 + d2 * d;
          a2 = a2 + d2 * d2;
        }
      }
    }
  }
  double r0 = block_tree_sum(a0, sh), r1, r2, r3;
  if (SWEEP == 0) {
    r1 = block_min(a1, sh);
    r2 = block_max(a2, sh);
    r3 = block_tree_sum(a3, sh);
  } else {
    r1 = block_tree_sum(a1, sh);
    r2 = block_tree_sum(a2, sh);
    r3 = 0.0;
  }
  if (t == 0) {
    double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * 4;
    p[0] = r0;
    p[1] = r1;
    p[2] = r2;
    p[3] = r3;
  }
}

// one block per column over the B block partials, in a fixed order
template <int SWEEP>
__global__ __launch_bounds__(kSumThreads) void k_moments_finish(const double* __restrict__ part, int B, int64_t n,
                                                                double* __restrict__ out) {
  __shared__ double sh[kSumThreads / kWave];
  const int c = blockIdx.x, t = threadIdx.x;
  const double* p = part + (int64_t)c * B * 4;
  double a0 = 0.0, a1 = SWEEP == 0 ? INFINITY : 0.0, a2 = SWEEP == 0 ? -INFINITY : 0.0, a3 = 0.0;
  for (int b = t; b < B; b += kSumThreads) {
    const double q0 = p[b * 4], q1 = p[b * 4 + 1], q2 = p[b * 4 + 2], q3 = p[b * 4 + 3];
    a0 = a0 + q0;
    if (SWEEP == 0) {
      a1 = q1 < a1 ? q1 : a1;
      a2 = q2 > a2 ? q2 : a2;
      a3 = a3 + q3;
    } else {
      a1 = a1 + q1;
      a2 = a2 + q2;
    }
  }
  double* o = out + c * PBH_MOMENTS_STRIDE;
  const double dn = (double)n;
  if (SWEEP == 0) {
    const double s = block_tree_sum(a0, sh);
    const double mn = block_min(a1, sh), mx = block_max(a2, sh);
    const double nan = block_tree_sum(a3, sh);
    if (t == 0) {
      double mean = s / dn;
      if (nan == 0.0 && mn == mx) mean = mn;  // n equal values: their mean is that value
      o[0] = nan;
      o[1] = nan > 0.0 ? NAN : mn;
      o[2] = nan > 0.0 ? NAN : mx;
      o[3] = mean;
      o[7] = 0.0;
    }
  } else {
    const double s2 = block_tree_sum(a0, sh), s3 = block_tree_sum(a1, sh), s4 = block_tree_sum(a2, sh);
    if (t == 0) {
      o[4] = s2 / dn;
      o[5] = s3 / dn;
      o[6] = s4 / dn;
    }
  }
}

// ---------------------------------------------------------------- select
// np.sort's order: the key image of pbh_common.h, every NaN (either sign) on the one largest key.
// No other double maps to a key whose top 16 bits are all ones.
__device__ __forceinline__ uint64_t select_key(double x) { return x != x ? ~0ull : f64_to_key(x); }

struct SelPrefixes {
  uint64_t prefix[kSelMaxRanks];  // distinct, ascending
  int32_t count;
};

struct SelTargets {
  uint64_t rem[kSelMaxRanks];  // rank among the keys that share the target's prefix
  uint8_t slot[kSelMaxRanks];  // index of that prefix in SelPrefixes
  int32_t count;
};

struct SelNarrowed {
  uint64_t rem;
  uint32_t digit;
  uint32_t pad;
};

// First pass: every key counts its top 16 bits.  65536 16-bit counters, two per LDS word; a tile
// adds at most kSelTile < 65536 to a counter, and the counters are flushed (one global add per
// non-empty counter) and cleared after every tile, so none overflows.  When the whole wave holds
// one digit (one binade, one repeated value) its leader adds the wave's count: 64 adds to one LDS
// word would serialise (k_digit_hist of pbh_sort.hip).
__global__ __launch_bounds__(kSelThreads) void k_select_top(const double* __restrict__ x, int64_t n,
                                                            uint32_t* __restrict__ hist) {
  __shared__ uint32_t w[32768];
  const int t = threadIdx.x, lane = t & (kWave - 1);
  for (int i = t; i < 32768; i += kSelThreads) w[i] = 0;
  __syncthreads();
  const int64_t tiles = (n + kSelTile - 1) / kSelTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kSelTile + t;
#pragma unroll 4
    for (int j = 0; j < kSelItems; ++j) {
      const int64_t i = base + (int64_t)j * kSelThreads;
      const bool valid = i < n;
      const uint32_t d = valid ? (uint32_t)(select_key(x[i]) >> 48) : 0u;
      const uint64_t active = __ballot(valid);
      if (active == 0ull) continue;  // wave-uniform
      const int leader = __builtin_ctzll(active);
      const uint32_t d0 = (uint32_t)__shfl((int)d, leader, kWave);
      if (__ballot(valid && d == d0) == active) {
        if (lane == leader) atomicAdd(&w[d0 >> 1], (uint32_t)__popcll(active) << ((d0 & 1u) * 16u));
      } else if (valid) {
        atomicAdd(&w[d >> 1], 1u << ((d & 1u) * 16u));
      }
    }
    __syncthreads();
    for (int i = t; i < 32768; i += kSelThreads) {
      const uint32_t v = w[i];
      if (v) {
        if (v & 0xFFFFu) atomicAdd(&hist[2 * i], v & 0xFFFFu);
        if (v >> 16) atomicAdd(&hist[2 * i + 1], v >> 16);
        w[i] = 0;
      }
    }
    __syncthreads();
  }
}

// Passes 1..3: a key whose top `16 * pass` bits equal prefix s counts its next digit into
// hist[s * 65536 + digit].  Lanes of a wave that hold the same (prefix, digit) are counted by one
// add (up to 16 distinct pairs per wave instruction; what is left adds singly).
__global__ __launch_bounds__(256) void k_select_next(const double* __restrict__ x, int64_t n, int pass,
                                                     SelPrefixes pf, uint32_t* __restrict__ hist) {
  __shared__ uint64_t sp[kSelMaxRanks];
  const int t = threadIdx.x, lane = t & (kWave - 1);
  if (t < kSelMaxRanks) sp[t] = t < pf.count ? pf.prefix[t] : ~0ull;
  __syncthreads();
  const int np = pf.count;
  const int pshift = 64 - 16 * pass, dshift = 48 - 16 * pass;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t iters = (n + stride - 1) / stride;  // the same for every thread: ballots stay whole
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t i = it * stride + (int64_t)blockIdx.x * 256 + t;
    bool live = false;
    uint32_t code = 0;
    if (i < n) {
      const uint64_t key = select_key(x[i]);
      const uint64_t p = key >> pshift;
      int lo = 0, hi = np;  // first slot with sp[slot] >= p
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sp[mid] < p)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < np && sp[lo] == p) {
        live = true;
        code = ((uint32_t)lo << 16) | ((uint32_t)(key >> dshift) & 0xFFFFu);
      }
    }
    for (int round = 0; round < 16; ++round) {
      const uint64_t m = __ballot(live);
      if (m == 0ull) break;  // wave-uniform
      const int leader = __builtin_ctzll(m);
      const uint32_t c0 = (uint32_t)__shfl((int)code, leader, kWave);
      const bool same = live && code == c0;
      const uint64_t sm = __ballot(same);
      if (lane == leader) atomicAdd(&hist[c0], (uint32_t)__popcll(sm));
      live = live && !same;
    }
    if (live) atomicAdd(&hist[code], 1u);
  }
}

// One block per target: the digit d with cum[d] <= rem < cum[d + 1] in its prefix' 65536 counters.
__global__ __launch_bounds__(1024) void k_select_narrow(const uint32_t* __restrict__ hist, SelTargets tg,
                                                        SelNarrowed* __restrict__ res) {
  __shared__ uint64_t chunk[1024];
  const int t = threadIdx.x, q = blockIdx.x;
  const uint32_t* h = hist + (size_t)tg.slot[q] * 65536;
  uint64_t s = 0;
  for (int j = 0; j < 64; ++j) s += h[t * 64 + j];
  chunk[t] = s;
  __syncthreads();
  if (t < kWave) {
    uint64_t mine = 0;
    for (int j = 0; j < 16; ++j) mine += chunk[t * 16 + j];
    uint64_t incl = mine;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint64_t y = __shfl_up(incl, o, kWave);
      if (t >= o) incl += y;
    }
    uint64_t before = incl - mine;
    const uint64_t rem = tg.rem[q];
    const bool last = t == kWave - 1;  // (rem >= the total cannot happen; the last lane takes it)
    if (rem >= before && (rem < incl || last)) {
      int d = t * 1024, dend = d + 1024;
      for (int j = 0; j < 16; ++j) {
        const uint64_t cs = chunk[t * 16 + j];
        if (rem < before + cs || j == 15) break;
        before += cs;
        d += 64;
      }
      dend = d + 64;
      for (; d < dend - 1; ++d) {
        const uint64_t cnt = h[d];
        if (rem < before + cnt) break;
        before += cnt;
      }
      res[q].digit = (uint32_t)d;
      res[q].rem = rem - before;
      res[q].pad = 0;
    }
  }
}

// ---------------------------------------------------------------- histogram
__global__ __launch_bounds__(kSumThreads) void k_histogram(const double* __restrict__ X, int64_t n, int64_t ld,
                                                           const double* __restrict__ edges, int bins,
                                                           unsigned long long* __restrict__ counts) {
  extern __shared__ double dyn[];  // edges (bins + 1 doubles), then bins uint32 counters
  double* e = dyn;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(dyn + bins + 1);
  const int c = blockIdx.y, t = threadIdx.x, lane = t & (kWave - 1);
  for (int i = t; i <= bins; i += kSumThreads) e[i] = edges[i];
  for (int i = t; i < bins; i += kSumThreads) cnt[i] = 0;
  __syncthreads();
  const double lo = e[0], hi = e[bins];
  const double scale = (double)bins / (hi - lo);
  const double* __restrict__ x = X + (int64_t)c * ld;
  const int64_t tiles = (n + kSumTile - 1) / kSumTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kSumTile + t;
    double v[kSumItems];
#pragma unroll
    for (int j = 0; j < kSumItems; ++j) {
      const int64_t i = base + (int64_t)j * kSumThreads;
      v[j] = i < n ? x[i] : NAN;
    }
#pragma unroll
    for (int j = 0; j < kSumItems; ++j) {
      const double xv = v[j];
      const bool in = xv >= lo && xv <= hi;  // false for NaN
      int b = 0;
      if (in) {
        const double f = (xv - lo) * scale;
        // hi - lo subnormal or overflowing makes scale inf or 0 and f possibly NaN: only a guess
        // in [0, bins - 1) is converted
        b = !(f >= 0.0) ? 0 : f >= (double)(bins - 1) ? bins - 1 : (int)f;
        while (b > 0 && xv < e[b]) --b;
        while (b < bins - 1 && xv >= e[b + 1]) ++b;
      }
      const uint64_t active = __ballot(in);
      if (active == 0ull) continue;  // wave-uniform
      const int leader = __builtin_ctzll(active);
      const int b0 = __shfl(b, leader, kWave);
      if (__ballot(in && b == b0) == active) {
        if (lane == leader) atomicAdd(&cnt[b0], (uint32_t)__popcll(active));
      } else if (in) {
        atomicAdd(&cnt[b], 1u);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = counts + (int64_t)c * bins;
  for (int i = t; i < bins; i += kSumThreads)
    if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
}

int check_block(const char* what, const void* X, int64_t n, int32_t k, int64_t ld) {
  PBH_REQUIRE(X != nullptr, "%s: X is NULL", what);
  PBH_REQUIRE(((uintptr_t)X & 7) == 0, "%s: X must be 8-byte aligned", what);
  PBH_REQUIRE(n >= 1, "%s: n = %lld; a summary needs at least one sample", what, (long long)n);
  PBH_REQUIRE(k >= 1 && k <= 65535, "%s: k = %d is outside [1, 65535]", what, (int)k);
  PBH_REQUIRE(k == 1 || ld >= n, "%s: ld = %lld < n = %lld", what, (long long)ld, (long long)n);
  return PBH_OK;
}

constexpr size_t kSelHistBytes = 65536 * sizeof(uint32_t);

}  // namespace
}  // namespace pbh

using namespace pbh;

extern "C" int pbh_moments_workspace_size(int32_t k, size_t* bytes) {
  PBH_REQUIRE(bytes != nullptr && k >= 1, "pbh_moments_workspace_size: bad arguments");
  *bytes = (size_t)k * kSumMaxBlocks * 4 * sizeof(double);
  return PBH_OK;
}

extern "C" int pbh_moments(const double* X, int64_t n, int32_t k, int64_t ld, double* out, void* ws, size_t ws_bytes,
                           void* stream) {
  if (int st = check_block("pbh_moments", X, n, k, ld)) return st;
  PBH_REQUIRE(out != nullptr && ws != nullptr, "pbh_moments: out / ws is NULL");
  size_t need = 0;
  pbh_moments_workspace_size(k, &need);
  if (ws_bytes < need) {
    set_error("pbh_moments: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return PBH_ERR_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  const int B = (int)summary_blocks(n);
  double* part = (double*)ws;
  const dim3 grid((unsigned)B, (unsigned)k), block(kSumThreads);
  hipLaunchKernelGGL(k_moments<0>, grid, block, 0, s, X, n, ld, (const double*)out, part);
  hipLaunchKernelGGL(k_moments_finish<0>, dim3((unsigned)k), block, 0, s, (const double*)part, B, n, out);
  hipLaunchKernelGGL(k_moments<1>, grid, block, 0, s, X, n, ld, (const double*)out, part);
  hipLaunchKernelGGL(k_moments_finish<1>, dim3((unsigned)k), block, 0, s, (const double*)part, B, n, out);
  PBH_CHECK_LAUNCH();
  return PBH_OK;
}

extern "C" int pbh_select_workspace_size(int32_t m, size_t* bytes) {
  PBH_REQUIRE(bytes != nullptr && m >= 1 && m <= kSelMaxRanks, "pbh_select_workspace_size: m = %d is outside [1, %d]",
              (int)m, kSelMaxRanks);
  *bytes = (size_t)m * kSelHistBytes + (size_t)kSelMaxRanks * sizeof(SelNarrowed);
  return PBH_OK;
}

extern "C" int pbh_select_ranks(const double* x, int64_t n, const int64_t* ranks_host, int32_t m, double* out_host,
                                void* ws, size_t ws_bytes, void* stream) {
  if (int st = check_block("pbh_select_ranks", x, n, 1, n)) return st;
  PBH_REQUIRE(n < ((int64_t)1 << 32), "pbh_select_ranks: n = %lld; the counters are 32-bit", (long long)n);
  PBH_REQUIRE(ranks_host && out_host && ws, "pbh_select_ranks: ranks / out / ws is NULL");
  PBH_REQUIRE(m >= 1 && m <= kSelMaxRanks, "pbh_select_ranks: m = %d ranks is outside [1, %d]", (int)m, kSelMaxRanks);
  for (int q = 0; q < m; ++q)
    PBH_REQUIRE(ranks_host[q] >= 0 && ranks_host[q] < n, "pbh_select_ranks: rank[%d] = %lld is outside [0, %lld)", q,
                (long long)ranks_host[q], (long long)n);
  size_t need = 0;
  pbh_select_workspace_size(m, &need);
  if (ws_bytes < need) {
    set_error("pbh_select_ranks: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return PBH_ERR_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  uint32_t* hist = (uint32_t*)ws;
  SelNarrowed* res = (SelNarrowed*)((char*)ws + (size_t)m * kSelHistBytes);

  uint64_t prefix[kSelMaxRanks] = {};  // per target: its key's top 16 * pass bits
  SelTargets tg;
  memset(&tg, 0, sizeof tg);
  tg.count = m;
  for (int q = 0; q < m; ++q) tg.rem[q] = (uint64_t)ranks_host[q];
  SelPrefixes pf;
  memset(&pf, 0, sizeof pf);
  pf.count = 1;  // the empty prefix
  SelNarrowed got[kSelMaxRanks];
  for (int pass = 0; pass < 4; ++pass) {
    PBH_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)pf.count * kSelHistBytes, s));
    if (pass == 0) {
      const int64_t tiles = (n + kSelTile - 1) / kSelTile;
      const unsigned g = (unsigned)std::min<int64_t>(tiles, kSelMaxBlocks);
      hipLaunchKernelGGL(k_select_top, dim3(g), dim3(kSelThreads), 0, s, x, n, hist);
    } else {
      hipLaunchKernelGGL(k_select_next, dim3(grid_for(n, 256 * 8, 2048)), dim3(256), 0, s, x, n, pass, pf, hist);
    }
    hipLaunchKernelGGL(k_select_narrow, dim3((unsigned)m), dim3(1024), 0, s, (const uint32_t*)hist, tg, res);
    PBH_CHECK_LAUNCH();
    PBH_CHECK_HIP(hipMemcpyAsync(got, res, (size_t)m * sizeof(SelNarrowed), hipMemcpyDeviceToHost, s));
    PBH_CHECK_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < m; ++q) {
      prefix[q] = (prefix[q] << 16) | (uint64_t)(got[q].digit & 0xFFFFu);
      tg.rem[q] = got[q].rem;
    }
    // the next pass' prefixes: the distinct ones, ascending; every target's slot among them
    uint64_t sorted[kSelMaxRanks];
    std::copy(prefix, prefix + m, sorted);
    std::sort(sorted, sorted + m);
    const int np = (int)(std::unique(sorted, sorted + m) - sorted);
    pf.count = np;
    for (int j = 0; j < kSelMaxRanks; ++j) pf.prefix[j] = j < np ? sorted[j] : ~0ull;
    for (int q = 0; q < m; ++q) tg.slot[q] = (uint8_t)(std::lower_bound(sorted, sorted + np, prefix[q]) - sorted);
  }
  for (int q = 0; q < m; ++q) out_host[q] = prefix[q] == ~0ull ? (double)NAN : key_to_f64(prefix[q]);
  return PBH_OK;
}

extern "C" int pbh_histogram_workspace_size(int32_t bins, size_t* bytes) {
  PBH_REQUIRE(bytes != nullptr && bins >= 1 && bins <= PBH_HISTOGRAM_MAX_BINS,
              "pbh_histogram_workspace_size: bins = %d is outside [1, %d]", (int)bins, PBH_HISTOGRAM_MAX_BINS);
  *bytes = ((size_t)bins + 1) * sizeof(double);
  return PBH_OK;
}

extern "C" int pbh_histogram(const double* X, int64_t n, int32_t k, int64_t ld, const double* edges_host, int32_t bins,
                             int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (int st = check_block("pbh_histogram", X, n, k, ld)) return st;
  PBH_REQUIRE(bins >= 1 && bins <= PBH_HISTOGRAM_MAX_BINS, "pbh_histogram: bins = %d is outside [1, %d]", (int)bins,
              PBH_HISTOGRAM_MAX_BINS);
  PBH_REQUIRE(edges_host && counts && ws, "pbh_histogram: edges / counts / ws is NULL");
  PBH_REQUIRE(isfinite(edges_host[0]) && isfinite(edges_host[bins]) && edges_host[0] < edges_host[bins],
              "pbh_histogram: the range [%g, %g] is not finite and increasing", edges_host[0], edges_host[bins]);
  for (int i = 0; i < bins; ++i)
    PBH_REQUIRE(edges_host[i] <= edges_host[i + 1], "pbh_histogram: edges[%d] > edges[%d]", i, i + 1);
  size_t need = 0;
  pbh_histogram_workspace_size(bins, &need);
  if (ws_bytes < need) {
    set_error("pbh_histogram: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return PBH_ERR_WORKSPACE;
  }
  hipStream_t s = as_stream(stream);
  PBH_CHECK_HIP(hipMemcpyAsync(ws, edges_host, need, hipMemcpyHostToDevice, s));
  PBH_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)k * bins * sizeof(int64_t), s));
  const size_t lds = need + (size_t)bins * sizeof(uint32_t);
  hipLaunchKernelGGL(k_histogram, dim3((unsigned)summary_blocks(n), (unsigned)k), dim3(kSumThreads), lds, s, X, n, ld,
                     (const double*)ws, (int)bins, (unsigned long long*)counts);
  PBH_CHECK_LAUNCH();
  return PBH_OK;
}
