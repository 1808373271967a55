// Process-wide cache of inverse-CDF setup tables (pbh_table_cache.hip).
#pragma once

#include <stddef.h>

#include <functional>

#include "pbh_common.h"
#include "pbh_scope.h"

namespace pbh {

enum TableKind : int {
  kTabGammaGuide = 1,  // gammainc guide of shape a (gamma, chi, chi2, maxwell, nakagami)
  kTabPoisson = 2,     // pdtr CDF + scipy windows + guide of mean mu
  kTabBetaGuide = 3,   // betainc guide of (a, b)
  kTabDiscrete = 4,    // binom / bernoulli / nbinom CDF + complement (key: dist id, parameters)
};

using TableBuild = std::function<bool(double*, hipStream_t)>;

// The table of (kind, key[0 .. nkey)), held until the ref leaves: built once per process and
// device by `build` on stream s into a persistent allocation of `bytes`, then reused by every
// later call (s waits for the build's completion event); when the cache is full, a table of this
// call's own in a stream-ordered allocation.  Empty when the build or the allocation fails.
TableRef acquire_table(int kind, const double* key, int nkey, size_t bytes, hipStream_t s, const TableBuild& build);

}  // namespace pbh
