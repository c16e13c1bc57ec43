// picp_host.h -- host-side internals shared by the runtime translation units (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <vector>

#include "picp_c.h"
#include "picp_internal.h"
#include "picp_pose.h"

#pragma GCC visibility push(hidden)

// records the thread's last error message (picp_last_error) and returns `code`
__attribute__((format(printf, 2, 3))) int picp_set_err(int code, const char* fmt, ...);

// the pose conversions the host calls (picp_pose.h)
using picp::pose_to_state;
using picp::state_to_pose;
// picp_runtime.cpp
void state_to_stats(const PicpState& s, picp_stats& st);

// checks that `device` exists (PICP_ERR_ARG, the message names the caller `what`) and makes it the
// thread's current one.  picp_runtime.cpp
int select_device(const char* what, int device);

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// Device buffer *ptr of *cap elements of `elem` bytes, discarded and allocated anew (at least 256
// elements) when `need` elements do not fit; the contents are not kept.  picp_runtime.cpp
int grow(void** ptr, int64_t* cap, int64_t need, size_t elem);

// A growable device buffer of T: the pointer and its capacity in elements.  It frees itself with
// its owner; kernels and launch wrappers receive the raw pointer.
template <class T>
struct DevBuf {
  T* p = nullptr;
  int64_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  // room for n elements (at least 256); the contents are not kept.  PICP_ERR_NOMEM on failure.
  int grow(int64_t n) {
    void* q = p;
    const int rc = ::grow(&q, &cap, n, sizeof(T));
    p = (T*)q;
    return rc;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  operator T*() const { return p; }
};

// hipEvents destroyed on every return path
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t create() {
    hipError_t e = hipEventCreate(&a);
    return e == hipSuccess ? hipEventCreate(&b) : e;
  }
  ~EventPair() {
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
  }
};

// n timed spans: the caller enqueues span i's work between begin(i) and end(i) and anything untimed
// (a restore) outside them.  sum_ms waits for the stream and adds up the spans' elapsed times.
struct TimedSpans {
  std::vector<EventPair> ev;
  explicit TimedSpans(int n) : ev((size_t)n) {}
  hipError_t create() {
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < ev.size() && e == hipSuccess; ++i) e = ev[i].create();
    return e;
  }
  hipError_t begin(int i, hipStream_t st) { return hipEventRecord(ev[(size_t)i].a, st); }
  hipError_t end(int i, hipStream_t st) { return hipEventRecord(ev[(size_t)i].b, st); }
  hipError_t sum_ms(hipStream_t st, double* total) {
    hipError_t e = hipStreamSynchronize(st);
    *total = 0.0;
    for (size_t i = 0; i < ev.size() && e == hipSuccess; ++i) {
      float ms = 0.0f;
      e = hipEventElapsedTime(&ms, ev[i].a, ev[i].b);
      *total += ms;
    }
    return e;
  }
};

#pragma GCC visibility pop

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return picp_set_err(e_ == hipErrorOutOfMemory ? PICP_ERR_NOMEM : PICP_ERR_DEVICE,     \
                          "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                          __LINE__);                                                        \
  } while (0)

#define CHECK_ARG(cond, msg)                                                                \
  do {                                                                                      \
    if (!(cond)) return picp_set_err(PICP_ERR_ARG, "%s", msg);                              \
  } while (0)
