// trace_loss.hpp -- the host arithmetic of the posterior summaries, each rule once.
//
// The hdpm_trace_* calls (summary_host.cpp) turn the device's integer sums into losses; the
// tests compare those bit for bit, so every call goes through the same expressions here:
// a candidate's cluster sizes to log2 sizes, sum_a n_a log2 n_a and sum_a C2(n_a); the VI
// against the trace and against one draw; the term of VI.lb; the candidates per block; the
// label range; and the 63-bit bound of the integer sums.
//
// Plain C++, no HIP: summary_host.cpp includes it, and tests/cpp/trace_loss_test.cpp checks
// it on the host against straight-line restatements.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace hdpm {

constexpr size_t kTraceMaxBlock = 64;   // candidates per block at most (their N x 8-byte sums)

struct TlSizes {
  double hc;    // sum_a n_a log2 n_a, summed in ascending a
  uint64_t A;   // sum_a C2(n_a)
};
// lsz[a] = log2 n_a (0 for an empty cluster), with hc and A of the Ka sizes
inline TlSizes tl_sizes(const uint64_t* sz, int Ka, double* lsz) {
  TlSizes r{0.0, 0};
  for (int a = 0; a < Ka; ++a) {
    lsz[a] = sz[a] > 0 ? std::log2((double)sz[a]) : 0.0;
    r.hc = r.hc + (double)sz[a] * lsz[a];
    const uint64_t m = sz[a] > 0 ? sz[a] - 1 : 0;   // the even factor halved first: exact for any n_a
    r.A += (sz[a] & 1) ? sz[a] * (m / 2) : (sz[a] / 2) * m;
  }
  return r;
}

// mcclust.ext VI(cls, cls.draw): (sum_a n_a log2 n_a + (S - 2 sum_m sum_ab T log2 T) / M) / N
inline double tl_vi(double hc, double S, double l, double M, int N) { return (hc + (S - 2 * l) / M) / N; }

// VI to one draw (its S_m and sum_ab T log2 T); rounding can undershoot 0 when the candidate
// is the draw
inline double tl_vi_draw(double hc, double Sm, double l1, int N) {
  const double d = (hc + Sm - 2 * l1) / N;
  return d < 0.0 ? 0.0 : d;
}

// mcclust.ext VI.lb, the term of point i:
// (log2 n_{c_i} + log2 sum_j psm_ij - 2 log2 sum_{j in c_i} psm_ij) / N
inline double tl_vi_lb_term(double lsz, double lall, double lsame, int N) { return (lsz + lall - 2 * lsame) / N; }

// candidates per block: budget / (cells x 4 bytes) tables, at least 1, at most kTraceMaxBlock
// and the count itself
inline size_t tl_block(size_t budget, size_t cells, size_t count) {
  const size_t cb = std::max<size_t>(1, budget / (cells * 4));
  return std::min(std::min(cb, kTraceMaxBlock), count);
}

// the largest of n labels, or -1 if one lies outside 0..254
inline int tl_label_max(const int32_t* lab, int64_t n) {
  int mx = 0;
  for (int64_t q = 0; q < n; ++q) {
    if (lab[q] < 0 || lab[q] > 254) return -1;
    mx = std::max(mx, lab[q]);
  }
  return mx;
}

// N^2 M < 2^63: the integer sums over pairs of points and draws cannot overflow
inline bool tl_fits63(uint64_t N, uint64_t M) {
  return !((unsigned __int128)N * (unsigned __int128)N * (unsigned __int128)M >> 63);
}

}  // namespace hdpm
