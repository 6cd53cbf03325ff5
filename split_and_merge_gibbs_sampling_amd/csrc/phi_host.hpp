// The outcome of one device update_phi (phi.hip) as the host sees it: where the outputs lie, how
// they are read, which hand-back bit a status sets, which kernels run the update again, and how
// the log-likelihood pairs are summed.  Plain C++, no HIP (tests/cpp/phi_host_test.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

// The statuses the host decides on (engine.cpp asserts them against kernels.hpp's PhiStatus)
// and the kernels of an update (enqueue_phi's mode).
namespace phi_host {
constexpr int kOk = 0, kWindow = 4, kShort = 5, kNonDet = 9;
constexpr int kWalks = 0, kTree = 1, kFast = 2, kNoRerun = -1;
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
}  // namespace phi_host

// Outputs of a device update of T clusters of d attributes: status (int) at 0 and consumption
// (int64) at 8, then picks (a byte per item), sigmas, log-likelihood pairs; `bytes` ends them.
// The fast path's copy of the stream state after the update (624 words + a flag) is at o_state.
struct PhiOutLayout {
  size_t o_pick, o_sig, o_ll, bytes, o_state;
};
inline PhiOutLayout phi_out_layout(int T, int d) {
  const size_t items = (size_t)T * d, o_sig = phi_host::align16(16 + items), o_ll = o_sig + items * 8,
               bytes = o_ll + (size_t)2 * T * 8;
  return {16, o_sig, o_ll, bytes, phi_host::align16(bytes)};
}

// A completed update's output buffer, read-only.
class PhiOutView {
  const uint8_t* p_;
  PhiOutLayout L_;

 public:
  PhiOutView(const uint8_t* out, const PhiOutLayout& L) : p_(out), L_(L) {}
  int status() const { return ((const int*)p_)[0]; }
  int64_t cons() const {
    int64_t c;
    std::memcpy(&c, p_ + 8, 8);
    return c;
  }
  const uint8_t* pick() const { return p_ + L_.o_pick; }
  const double* sig() const { return (const double*)(p_ + L_.o_sig); }
  const double* ll() const { return (const double*)(p_ + L_.o_ll); }
  const uint32_t* state_words() const { return (const uint32_t*)(p_ + L_.o_state); }
};

// The bit of hdpm_stats.phi_fallback_status_mask a handed-back update sets: its status (0..14),
// or 15 for an update that completed (kOk) but whose result the host cannot adopt.
inline int64_t phi_handback_bit(int status) {
  return (int64_t)1 << (status != phi_host::kOk ? std::min(std::max(status, 0), 14) : 15);
}

// The re-run ladder: the kernels that run the same update again (same inputs, nothing committed
// yet) after `mode_ran` ended with `status`, or kNoRerun.  A pick that depended on the uniform
// (kNonDet) goes to the walks; any other case the fast path leaves open goes to the general
// kernels, except a drift outside its window (kWindow, kShort), which is the caller's to widen.
inline int phi_rerun_mode(int mode_ran, int status, bool tree) {
  using namespace phi_host;
  if (mode_ran == kWalks || status == kOk) return kNoRerun;
  if (status == kNonDet) return kWalks;
  if (mode_ran == kFast && status != kWindow && status != kShort) return tree ? kTree : kWalks;
  return kNoRerun;
}

// Centers (pick + 1) and sigmas of the update's T clusters into rows labels[t] (null: row t)
// of cen / sig ([.][d]).
inline void phi_copy_params(const PhiOutView& v, int T, int d, const int* labels, uint8_t* cen, double* sig) {
  for (int t = 0; t < T; ++t) {
    const size_t k = (size_t)(labels ? labels[t] : t);
    for (int j = 0; j < d; ++j) cen[k * d + j] = (uint8_t)(v.pick()[(size_t)t * d + j] + 1);
    std::memcpy(sig + k * d, v.sig() + (size_t)t * d, (size_t)d * 8);
  }
}

// compute_loglikelihood from the 2 T per-cluster terms in cluster order, as a compensated
// (two-sum) total.  Compared bit for bit: the order and form of every operation are fixed.
inline double phi_ll_fold(const double* ll, int T) {
  double hi = 0.0, lo = 0.0;
  for (int q = 0; q < 2 * T; ++q) {
    const double x = ll[q], s = hi + x;
    lo += std::fabs(hi) >= std::fabs(x) ? (hi - s) + x : (x - s) + hi;
    hi = s;
  }
  return hi + lo;
}
