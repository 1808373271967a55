// Launch shapes of the summary kernels (pbh_summary.hip): what a user does with the samples once
// they exist -- np.mean / np.var / scipy.stats.skew / kurtosis, np.quantile, np.histogram --
// computed where the samples are.  All three read the samples and write O(k * bins) bytes.
#pragma once

#include "pbh_common.h"

namespace pbh {

// moments and histogram: 256 threads x 8 items per tile, tiles dealt round-robin to at most
// PBH_SUMMARY_MAX_BLOCKS blocks per column (include/probabilit_hip.h states the summation shape)
constexpr int kSumThreads = 256;
constexpr int kSumItems = PBH_SUMMARY_TILE / kSumThreads;
constexpr int kSumTile = PBH_SUMMARY_TILE;
constexpr int kSumMaxBlocks = PBH_SUMMARY_MAX_BLOCKS;
static_assert(kSumItems * kSumThreads == kSumTile, "tile");

// select: 1024 threads x 16 keys per tile; the first pass keeps 65536 16-bit counters in LDS, and a
// tile adds at most kSelTile < 65536 to any of them before they are flushed
constexpr int kSelThreads = 1024;
constexpr int kSelItems = PBH_SELECT_TILE / kSelThreads;
constexpr int kSelTile = PBH_SELECT_TILE;
constexpr int kSelMaxBlocks = PBH_SELECT_MAX_BLOCKS;
constexpr int kSelMaxRanks = PBH_SELECT_MAX_RANKS;
static_assert(kSelItems * kSelThreads == kSelTile && kSelTile < 65536, "tile");

inline int64_t summary_blocks(int64_t n) {
  const int64_t tiles = (n + kSumTile - 1) / kSumTile;
  return tiles < 1 ? 1 : (tiles < kSumMaxBlocks ? tiles : kSumMaxBlocks);
}

}  // namespace pbh
