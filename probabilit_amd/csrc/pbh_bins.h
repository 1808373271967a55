// The bin rule shared by the kernels that bin by an edge table in LDS (pbh_joint.hip,
// pbh_binned.hip): np.histogramdd's, per axis.
#pragma once

#include "pbh_common.h"

namespace pbh {

// The bin of v among the m + 1 non-decreasing edges e (lo = e[0] <= v <= hi = e[m] holds):
// searchsorted(e, v, side="right") - 1, v == hi moved into the last bin.
template <bool UNIFORM>
__device__ __forceinline__ int joint_bin(const double* e, int m, double lo, double scale, double v) {
  if (UNIFORM) {  // k_histogram's guess by one multiply, corrected against the edges
    const double f = (v - lo) * scale;
    int b = !(f >= 0.0) ? 0 : f >= (double)(m - 1) ? m - 1 : (int)f;
    while (b > 0 && v < e[b]) --b;
    while (b < m - 1 && v >= e[b + 1]) ++b;
    return b;
  }
  // the number of edges <= v: every step halves the span whatever v is, so a wave does not diverge
  int base = 0, len = m + 1;
  while (len > 1) {
    const int half = len >> 1;
    base = e[base + half] <= v ? base + half : base;
    len -= half;
  }
  const int b = base + (e[base] <= v ? 1 : 0) - 1;
  return b > m - 1 ? m - 1 : b;
}

}  // namespace pbh
