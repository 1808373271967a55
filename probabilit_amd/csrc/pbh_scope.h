// What a call borrows from the device, owned by scope (host only): a return between acquiring
// and releasing cannot skip the release, because no release is written by hand.
#pragma once

#include <stddef.h>

#include <memory>
#include <vector>

#include "pbh_error.h"

namespace pbh {

// A pointer, the stream its release is ordered on, and the release: Release{}(p, stream) runs
// once, when a non-null pointer leaves (scope exit, reset, or assignment over it).  Move-only.
template <class T, class Release>
class Held {
 public:
  Held() = default;
  Held(T* p, hipStream_t s) : p_(p), s_(s) {}
  Held(Held&& o) noexcept : p_(o.p_), s_(o.s_) { o.p_ = nullptr; }
  Held& operator=(Held&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      s_ = o.s_;
      o.p_ = nullptr;
    }
    return *this;
  }
  Held(const Held&) = delete;
  Held& operator=(const Held&) = delete;
  ~Held() { reset(); }
  void reset() {
    if (p_) Release{}(p_, s_);
    p_ = nullptr;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  void set_stream(hipStream_t s) { s_ = s; }  // the release is ordered on s from now on

 private:
  T* p_ = nullptr;
  hipStream_t s_ = nullptr;
};

// A stream-ordered scratch buffer: hipMallocAsync by get, hipFreeAsync on the same stream when it
// leaves (after the kernels queued on that stream so far).
struct FreeAsync {
  void operator()(void* p, hipStream_t s) const { (void)hipFreeAsync(p, s); }
};
template <class T>
struct Scratch : Held<T, FreeAsync> {
  using Held<T, FreeAsync>::get;
  hipError_t get(size_t bytes, hipStream_t s) {  // replaces (and frees) what it held
    void* p = nullptr;
    const hipError_t e = hipMallocAsync(&p, bytes, s);
    if (e == hipSuccess) static_cast<Held<T, FreeAsync>&>(*this) = Held<T, FreeAsync>((T*)p, s);
    return e;
  }
};

// A held inverse-CDF setup table (acquire_table, pbh_table_cache.h): a cached one is given back
// to the cache, a private one is freed, either way ordered on the stream.  Empty: no table.
struct TableRelease {
  void operator()(double* t, hipStream_t s) const;  // pbh_table_cache.hip
};
using TableRef = Held<double, TableRelease>;

// An owned generated column (gen_create, pbh_step4.h); its table and run values leave on the
// deleter's stream, which the owner may set (get_deleter().s) before it lets go.
struct GenColumn;
struct GenDelete {
  hipStream_t s = nullptr;
  void operator()(GenColumn* g) const;  // pbh_ppf.hip
};
using GenHandle = std::unique_ptr<GenColumn, GenDelete>;

// Stream ordering with events it owns: order(from, to) lets `to` continue after `from`'s work so
// far; the events are destroyed with it.
class StreamOrder {
 public:
  StreamOrder() = default;
  StreamOrder(const StreamOrder&) = delete;
  StreamOrder& operator=(const StreamOrder&) = delete;
  ~StreamOrder() {
    for (hipEvent_t e : events_) (void)hipEventDestroy(e);
  }
  int order(hipStream_t from, hipStream_t to) {
    if (from == to) return PBH_OK;
    hipEvent_t e = nullptr;
    PBH_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    events_.push_back(e);
    PBH_CHECK_HIP(hipEventRecord(e, from));
    PBH_CHECK_HIP(hipStreamWaitEvent(to, e, 0));
    return PBH_OK;
  }

 private:
  std::vector<hipEvent_t> events_;
};

}  // namespace pbh
