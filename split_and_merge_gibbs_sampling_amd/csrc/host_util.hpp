// host_util.hpp -- host plumbing shared by the host translation units (engine.cpp,
// summary_host.cpp): HIP errors as exceptions, growing device and pinned buffers, and a
// simple fork-join loop over the host's threads.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

namespace hdpm {

struct HipError {
  hipError_t e;
  const char* what;
};
#define HIPCHK(x)                                      \
  do {                                                 \
    hipError_t _e = (x);                               \
    if (_e != hipSuccess) throw HipError{_e, #x};     \
  } while (0)

inline std::atomic<int64_t> g_dev_allocs{0};   // device allocations made (diagnostics)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  // Grow to at least `count` elements; keep_old copies the previous contents.
  void ensure(size_t count, bool keep_old = false, hipStream_t s = nullptr) {
    if (count <= n && p) return;
    T* np = nullptr;
    g_dev_allocs.fetch_add(1, std::memory_order_relaxed);
    HIPCHK(hipMalloc(&np, std::max<size_t>(count, 1) * sizeof(T)));
    if (keep_old && p && n) {
      HIPCHK(hipMemcpyAsync(np, p, n * sizeof(T), hipMemcpyDeviceToDevice, s));
      HIPCHK(hipStreamSynchronize(s));
    }
    release();
    p = np;
    n = count;
  }
};

template <class T>
struct PinBuf {
  T* p = nullptr;
  size_t n = 0;
  ~PinBuf() {
    if (p) (void)hipHostFree(p);
  }
  // non-coherent (coarse-grained) by default: CPU-cached, so the host reads these buffers
  // at cache speed; every device write to them is followed by a stream or event wait
  // before use.  Buffers kernels read or write in place (no copy) are coherent.
  void ensure(size_t count, unsigned flags = hipHostMallocNonCoherent) {
    if (count <= n && p) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    HIPCHK(hipHostMalloc(&p, std::max<size_t>(count, 1) * sizeof(T), flags));
    n = count;
  }
};

inline int host_threads() {
  unsigned h = std::thread::hardware_concurrency();
  if (h == 0) h = 4;
  return (int)std::min<unsigned>(h, 16);
}

template <class F>
void parallel_for(int64_t n, F f) {
  const int T = host_threads();
  if (n < 4096 || T <= 1) {
    f(0, n);
    return;
  }
  std::vector<std::thread> th;
  const int64_t chunk = (n + T - 1) / T;
  for (int t = 0; t < T; ++t) {
    int64_t a = t * chunk, b = std::min(n, a + chunk);
    if (a >= b) break;
    th.emplace_back([=] { f(a, b); });
  }
  for (auto& x : th) x.join();
}

}  // namespace hdpm
