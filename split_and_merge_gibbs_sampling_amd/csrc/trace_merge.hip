// trace_merge.hip -- what merging two classes of a partition c would change in the expected
// VI or in Binder's loss, for all pairs at once and from the contingency tables alone
// (hdpm_trace_merge_gains, hdpm_trace_merge_path, hdpm_trace_refine_merge).
//
// With T^m[a][z] the table of c against draw z_m, n_a the class sizes and
//   f(s, t) = (s + t) log2(s + t) - s log2 s - t log2 t   (0 if s = 0 or t = 0)
//           = (s log1p(t / s) + t log1p(s / t)) / ln 2     as evaluated,
// merging the non-empty classes a < b changes
//
//   VI:     mgain[a][b] = (M f(n_a, n_b) - 2 sum_m sum_z f(T^m[a][z], T^m[b][z])) / (M N)
//   Binder: mgain[a][b] = M n_a n_b - 2 cross[a][b]      (the change of M A + P - 2 Q)
//
// and a pair with an empty class, like the diagonal, has gain exactly 0.
//
//   k_mg_pairs  VI, over the transposed tables of k_tr_transpose: one thread per pair and
//               slice of the draws (k_tr_cross's slices, m = y, y + S, ..).  The lanes of a
//               wave share one class u and take consecutive classes v: per cell one
//               broadcast load and one coalesced load.  The thread runs through its draws in
//               order and through z ascending with one double accumulator, skipping cells
//               where either count is 0 (their term is exactly +0.0), and stores its partial
//               at part[slice][min(u, v)][max(u, v)].  All pairs u < v, or (after a fold)
//               only the pairs of one class: f(s, t) and f(t, s) are the same bits, so the
//               stored value does not depend on which way round the pair was taken.
//   k_mg_gain   one thread per entry of the Ka x Ka matrix: the slices of its pair summed in
//               slice order (VI) or cross read (Binder, k_tr_cross's integers), the gain
//               formed with the class sizes; both triangles from the same words.
//   k_mg_fold   row b of every draw's table added into row a and zeroed, in both layouts
//               (tab: M x Ka x Kz, tabT: M x Kz x Ka): the merged partition's tables, from
//               which k_tr_reduce gives its Q and sum T log2 T.
//
// No atomics on doubles, and the slice count depends on M alone: no gain depends on the
// grid, on the table budget or on Ka.
//
// Bound: k_mg_pairs is two log1p per cell pair with both counts non-zero, at most
// M x Kz x Ka (Ka - 1) / 2 of them, on tables that sit in L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/hdpm.h"
#include "summary_launch.hpp"

namespace hdpm {

constexpr int kMgThreads = 256;
constexpr int kMgWave = 64;           // pairs of a workgroup of k_mg_pairs: one wave, one class u
constexpr int kMgSlices = 64;         // slices of the draws, as in k_tr_cross

// trace_merge.hpp mg_f, on the device; s, t > 0
__device__ __forceinline__ double mg_fd(double s, double t) {
  return (s * log1p(t / s) + t * log1p(s / t)) / 0.6931471805599453;
}

// blockIdx.x = (class u, chunk of 64 classes v), blockIdx.y = slice.  only < 0: all pairs,
// u = 0 .. Ka - 2 and v = u + 1 + 64 chunk + lane; otherwise u = only and v = 64 chunk +
// lane, v != u.  part is slices x Ka x Ka; entries on or below the diagonal are never written.
__global__ __launch_bounds__(kMgWave) void k_mg_pairs(const uint32_t* __restrict__ tabT, int M, int Ka, int Kz,
                                                     int nchunk, int only, double* __restrict__ part) {
  const int chunk = (int)blockIdx.x % nchunk;
  const int u = only < 0 ? (int)blockIdx.x / nchunk : only;
  const int v = (only < 0 ? u + 1 : 0) + chunk * kMgWave + (int)threadIdx.x;
  if (v >= Ka || v == u) return;
  double acc = 0.0;
  for (int m = blockIdx.y; m < M; m += gridDim.y) {
    const uint32_t* T = tabT + (int64_t)m * Ka * Kz;
    for (int z = 0; z < Kz; ++z) {
      const uint32_t s = T[z * Ka + u], t = T[z * Ka + v];
      if (s != 0u && t != 0u) acc = acc + mg_fd((double)s, (double)t);
    }
  }
  const int lo = min(u, v), hi = max(u, v);
  part[((int64_t)blockIdx.y * Ka + lo) * Ka + hi] = acc;
}

// n: the Ka class sizes as doubles.  VI reads part (slices x Ka x Ka), Binder cross (Ka x Ka).
template <int LOSS>
__global__ __launch_bounds__(kMgThreads) void k_mg_gain(const double* __restrict__ part, int slices,
                                                       const unsigned long long* __restrict__ cross,
                                                       const double* __restrict__ n, int Ka, double dM, double dMN,
                                                       double* __restrict__ gain) {
  const int q = blockIdx.x * kMgThreads + threadIdx.x;
  if (q >= Ka * Ka) return;
  const int a = q / Ka, b = q % Ka;
  const int lo = min(a, b), hi = max(a, b);
  const double nl = n[lo], nh = n[hi];
  double g = 0.0;
  if (a != b && nl > 0.0 && nh > 0.0) {
    if (LOSS == HDPM_LOSS_VI) {
      double sum = 0.0;
      for (int y = 0; y < slices; ++y) sum = sum + part[((int64_t)y * Ka + lo) * Ka + hi];
      g = (dM * mg_fd(nl, nh) - 2.0 * sum) / dMN;
    } else {
      g = (double)((long long)dM * (long long)nl * (long long)nh - 2ll * (long long)cross[lo * Ka + hi]);
    }
  }
  gain[q] = g;
}

// one thread per (draw, z); either layout may be null
__global__ __launch_bounds__(kMgThreads) void k_mg_fold(uint32_t* __restrict__ tab, uint32_t* __restrict__ tabT, int M,
                                                       int Ka, int Kz, int a, int b) {
  const int64_t t = (int64_t)blockIdx.x * kMgThreads + threadIdx.x;
  if (t >= (int64_t)M * Kz) return;
  const int64_t m = t / Kz;
  const int z = (int)(t % Kz);
  if (tab) {
    uint32_t* T = tab + m * Ka * Kz;
    T[a * Kz + z] += T[b * Kz + z];
    T[b * Kz + z] = 0u;
  }
  if (tabT) {
    uint32_t* T = tabT + (m * Kz + z) * Ka;
    T[a] += T[b];
    T[b] = 0u;
  }
}

// ------------------------------------------------------------------------------ launchers

int mg_slices(int M) { return std::min(M, kMgSlices); }

// part holds mg_slices(M) x Ka x Ka doubles; only < 0 for all the pairs
hipError_t launch_mg_pairs(const uint32_t* tabT, int M, int Ka, int Kz, int only, double* part, hipStream_t s) {
  if (Ka < 2) return hipSuccess;
  const int span = only < 0 ? Ka - 1 : Ka;
  const int nchunk = (span + kMgWave - 1) / kMgWave;
  const int rows = only < 0 ? Ka - 1 : 1;
  hipLaunchKernelGGL(k_mg_pairs, dim3((unsigned)(rows * nchunk), (unsigned)mg_slices(M)), dim3(kMgWave), 0, s, tabT, M,
                     Ka, Kz, nchunk, only, part);
  return hipGetLastError();
}

// gain (Ka x Ka doubles) from part (HDPM_LOSS_VI) or cross (HDPM_LOSS_BINDER) and the sizes n
hipError_t launch_mg_gain(int loss, const double* part, const uint64_t* cross, const double* n, int M, int Ka, int N,
                          double* gain, hipStream_t s) {
  const dim3 grid((unsigned)((Ka * Ka + kMgThreads - 1) / kMgThreads));
  const double dM = (double)M, dMN = (double)M * (double)N;
  if (loss == HDPM_LOSS_VI)
    hipLaunchKernelGGL(k_mg_gain<HDPM_LOSS_VI>, grid, dim3(kMgThreads), 0, s, part, mg_slices(M),
                       (const unsigned long long*)cross, n, Ka, dM, dMN, gain);
  else
    hipLaunchKernelGGL(k_mg_gain<HDPM_LOSS_BINDER>, grid, dim3(kMgThreads), 0, s, part, mg_slices(M),
                       (const unsigned long long*)cross, n, Ka, dM, dMN, gain);
  return hipGetLastError();
}

hipError_t launch_mg_fold(uint32_t* tab, uint32_t* tabT, int M, int Ka, int Kz, int a, int b, hipStream_t s) {
  const int64_t tot = (int64_t)M * Kz;
  hipLaunchKernelGGL(k_mg_fold, dim3((unsigned)((tot + kMgThreads - 1) / kMgThreads)), dim3(kMgThreads), 0, s, tab,
                     tabT, M, Ka, Kz, a, b);
  return hipGetLastError();
}

}  // namespace hdpm
