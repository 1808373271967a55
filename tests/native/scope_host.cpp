// Host-only check of pbh_scope.h's generic holder (pbh::Held) with a counting release: every
// case must release each live pointer exactly once, on the stream last set, and an empty holder
// never.  No HIP call is made; the streams are made-up handles.  Exit status 0 = every case held.
#include <stdio.h>

#include <utility>
#include <vector>

#include "pbh_scope.h"

namespace {

struct Call {
  int* p;
  hipStream_t s;
};
std::vector<Call> g_log;

struct Count {
  void operator()(int* p, hipStream_t s) const { g_log.push_back(Call{p, s}); }
};
using H = pbh::Held<int, Count>;

hipStream_t stream(int i) { return reinterpret_cast<hipStream_t>((uintptr_t)0x1000 + 16 * (uintptr_t)i); }

int g_failed = 0;
int obj[8];

// the log holds exactly `want` (in order)
void expect(const char* what, std::vector<Call> want) {
  bool ok = g_log.size() == want.size();
  for (size_t i = 0; ok && i < want.size(); ++i) ok = g_log[i].p == want[i].p && g_log[i].s == want[i].s;
  printf("%s: %s (%zu releases, %zu expected)\n", what, ok ? "ok" : "FAILED", g_log.size(), want.size());
  if (!ok) ++g_failed;
  g_log.clear();
}

int early_return(bool early) {
  H a(&obj[0], stream(0));
  H b(&obj[1], stream(1));
  if (early) return 1;
  b.set_stream(stream(2));
  return 0;
}

}  // namespace

int main() {
  {
    H a(&obj[0], stream(0));
    expect("alive: nothing yet", {});
  }
  expect("scope exit", {{&obj[0], stream(0)}});
  {
    H a(&obj[0], stream(0));
    a.set_stream(stream(3));
    a.set_stream(stream(4));
  }
  expect("scope exit on the stream last set", {{&obj[0], stream(4)}});
  {
    H a(&obj[0], stream(0));
    H b(std::move(a));
    if (a.get() || b.get() != &obj[0]) ++g_failed;
    expect("move construction: nothing yet", {});
  }
  expect("move construction", {{&obj[0], stream(0)}});
  {
    H a(&obj[0], stream(0));
    H b(&obj[1], stream(1));
    b = std::move(a);
    expect("move assignment over a live holder: the old one", {{&obj[1], stream(1)}});
    if (a.get() || b.get() != &obj[0]) ++g_failed;
    b.set_stream(stream(5));
  }
  expect("move assignment: the moved one, once, with its stream set after", {{&obj[0], stream(5)}});
  {
    H a(&obj[0], stream(0));
    a.reset();
    expect("explicit reset", {{&obj[0], stream(0)}});
    a.reset();
    if (a.get()) ++g_failed;
  }
  expect("after reset: nothing more", {});
  if (early_return(true) != 1) ++g_failed;
  expect("early return from a function holding two", {{&obj[1], stream(1)}, {&obj[0], stream(0)}});
  if (early_return(false) != 0) ++g_failed;
  expect("late return from the same function", {{&obj[1], stream(2)}, {&obj[0], stream(0)}});
  {
    std::vector<H> v;
    for (int i = 0; i < 5; ++i) v.emplace_back(&obj[i], stream(i));  // grows: holders are moved
    expect("vector growth moves, releases nothing", {});
    while (!v.empty()) v.pop_back();
  }
  expect("a vector of holders destroyed in reverse",
         {{&obj[4], stream(4)}, {&obj[3], stream(3)}, {&obj[2], stream(2)}, {&obj[1], stream(1)}, {&obj[0], stream(0)}});
  {
    H e;
    H f(nullptr, stream(1));
    H g(std::move(e));
    f = std::move(g);
    f.set_stream(stream(2));
    f.reset();
  }
  expect("empty holders release nothing", {});
  printf("%s\n", g_failed ? "FAILED" : "all ok");
  return g_failed ? 1 : 0;
}
