// cf_host.h — the host-side plumbing every translation unit with entry points shares: how an error is reported, how a thread
// gets onto a handle's device, how device memory is owned, and how a host-buffer entry point walks its rows through the device.
// Host code only: nothing here reaches a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/cosmofit.h"

// Sets the calling thread's cf_last_error text and returns `code` (cosmofit_api.hip).
int cf_set_error(int code, const std::string& msg);

// A failed HIP call ends the enclosing function with CF_ERR_HIP and "<the call>: <what HIP said>".
#define HIP_TRY(expr)                                                                                    \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return cf_set_error(CF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Behind hipLaunchKernelGGL: CF_OK, or CF_ERR_HIP with "<fn>: <what HIP said>" when the launch was refused.
inline int cf_launch_status(const char* fn) {
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? CF_OK : cf_set_error(CF_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(err));
}

// The calling thread's current device is the caller's business (a torch process has its own idea of it): every entry point switches
// to the handle's device for its own HIP calls and switches back on the way out.  One hipGetDevice per call when the two agree.
struct DeviceScope {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) cur = -1;
    if (cur != dev) {
      err = hipSetDevice(dev);
      if (err == hipSuccess) prev = cur;
    }
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int ensure(size_t need) {
    if (need <= bytes) return 0;
    if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
    HIP_TRY(hipMalloc(&p, need));
    bytes = need;
    return 0;
  }
  template <class T> T* as() const { return (T*)p; }
};

// The rows of a host-buffer entry point, `piece` at a time through device buffers on one stream.  Name the row-indexed arguments
// with in() / out() (a null host pointer is an argument the caller left out: no buffer, null device pointer), then run(): per
// piece the inputs go up, body(s0, m) launches the device path on rows s0 .. s0 + m of the device buffers, the outputs come down
// behind the rows of the earlier pieces, and the stream is synchronised.  What does not advance with the rows (query points, a
// mock set, accumulators) is the caller's to copy before run().
class RowStage {
 public:
  RowStage(hipStream_t stream, int64_t piece) : st_(stream), piece_(piece) {}
  void* in(const void* host, size_t row_bytes) { return add(const_cast<void*>(host), row_bytes, false); }
  void* out(void* host, size_t row_bytes) { return add(host, row_bytes, true); }
  template <class T> T* in(const T* host, size_t row_bytes) { return (T*)in((const void*)host, row_bytes); }
  template <class T> T* out(T* host, size_t row_bytes) { return (T*)out((void*)host, row_bytes); }
  template <class F> int run(int64_t S, F body) {
    if (failed_) return failed_;
    for (int64_t s0 = 0; s0 < S; s0 += piece_) {
      const int64_t m = std::min(piece_, S - s0);
      for (int k = 0; k < n_; ++k)
        if (!col_[k].down)
          HIP_TRY(hipMemcpyAsync(col_[k].dev.p, col_[k].host + s0 * col_[k].row, (size_t)m * col_[k].row, hipMemcpyHostToDevice, st_));
      if (int rc = body(s0, m)) return rc;
      for (int k = 0; k < n_; ++k)
        if (col_[k].down)
          HIP_TRY(hipMemcpyAsync(col_[k].host + s0 * col_[k].row, col_[k].dev.p, (size_t)m * col_[k].row, hipMemcpyDeviceToHost, st_));
      HIP_TRY(hipStreamSynchronize(st_));
    }
    return CF_OK;
  }

 private:
  enum { MAX_COLS = 16 };
  struct Col {
    DevBuf dev;
    char* host;
    size_t row;
    bool down;
  };
  void* add(void* host, size_t row_bytes, bool down) {
    if (!host || failed_) return nullptr;
    if (n_ == MAX_COLS) {
      failed_ = cf_set_error(CF_ERR_INVALID, "RowStage: more than 16 row arguments");
      return nullptr;
    }
    Col& c = col_[n_];
    if ((failed_ = c.dev.ensure((size_t)piece_ * row_bytes))) return nullptr;
    c.host = (char*)host;
    c.row = row_bytes;
    c.down = down;
    ++n_;
    return c.dev.p;
  }
  hipStream_t st_;
  int64_t piece_;
  Col col_[MAX_COLS];
  int n_ = 0;
  int failed_ = 0;  // the first failed allocation's return code: run() reports it
};
