// trace_refine.hip -- what every single-point move would change in the expected VI or in
// Binder's loss of a partition c, from the saved labels and the contingency tables of
// trace_summary.hip, with no N x N matrix (hdpm_trace_move_gains, hdpm_trace_refine).
//
// With T^m[a][z] the table of c against draw z_m, n_a the class sizes and
// h(t) = (t + 1) log2(t + 1) - t log2 t (h(0) = 0), moving point i alone from a = c_i to
// class b != a (b = Ka: a new class, n_b = 0 and T[b][.] = 0) changes
//
//   VI:     gain[i][b] = (M (h(n_b) - h(n_a - 1)) - 2 (s[i][b] - s[i][a])) / (M N)
//           s[i][b] = sum_m h(T^m[b][z_m(i)]) for b != a, s[i][a] = sum_m h(T^m[a][z_m(i)] - 1)
//   Binder: gain[i][b] = M (n_b - n_a - 1) - 2 (aff[i][b] - aff[i][a])
//           aff[i][b] = sum_m T^m[b][z_m(i)]          (the change of M A + P - 2 Q)
//
// and gain[i][a] = 0.
//
//   k_rf_htable   the tables of c transposed as k_tr_transpose lays them out, each cell as
//                 the pair (h(T), h(T - 1)): the lanes of k_rf_sums do one load per draw and
//                 no log.  Binder reads the counts of k_tr_transpose itself.
//   k_rf_sums     k_tr_affinity's shape: one lane per (point, class) of a block of points,
//                 Ka + 1 lanes per point, consecutive lanes consecutive classes, so a wave is
//                 full for any Ka.  The lane owns s[i][b] (a double, added in draw order) or
//                 aff[i][b] (64-bit), keeps it in a register over the M draws with several
//                 draws' loads in flight, and stores it once to the block's staging array.
//                 The new-class lane reads nothing and stores 0.
//   k_rf_best     one thread per point of the block: the Ka + 1 gains from the staged sums in
//                 ascending class order, written over the sums when the full matrix is
//                 wanted, and their argmin.  The own class (gain 0) wins a tie, then the
//                 lowest class; at Ka = 255 the new class holds +inf and never wins.
//
// No sum crosses lanes and there are no atomics: every output is the same from run to run
// and does not depend on the grid or on how the points are cut into blocks.
//
// Bound: k_rf_sums issues M x N x Ka eight-byte (VI) or four-byte (Binder) reads into tables
// of M x Ka x Kz cells that sit in L2 or the Infinity Cache at ordinary sizes, and one label
// byte per read, shared by the lanes of a point through the vector cache.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/hdpm.h"
#include "summary_launch.hpp"

namespace hdpm {

constexpr int kRfThreads = 256;
constexpr int kRfUnroll = 4;          // draws whose label and table reads are in flight together

// trace_refine.hpp rf_h, on the device
__device__ __forceinline__ double rf_hd(double t) {
  return t > 0.0 ? log2(t + 1.0) + t * log1p(1.0 / t) / 0.6931471805599453 : 0.0;
}

// tab is M x Ka x Kz (k_tr_tables, one candidate); tabH is M x Kz x Ka pairs
__global__ __launch_bounds__(kRfThreads) void k_rf_htable(const uint32_t* __restrict__ tab, int M, int Ka, int Kz,
                                                         double2* __restrict__ tabH) {
  const int64_t t = (int64_t)blockIdx.x * kRfThreads + threadIdx.x;
  const int cells = Ka * Kz;
  if (t >= (int64_t)M * cells) return;
  const int m = (int)(t / cells), r = (int)(t % cells);
  const int b = r / Ka, a = r % Ka;
  const uint32_t c = tab[(int64_t)m * cells + a * Kz + b];
  tabH[t] = make_double2(rf_hd((double)c), c > 0u ? rf_hd((double)(c - 1u)) : 0.0);
}

template <int LOSS>
struct RfCell;
template <>
struct RfCell<HDPM_LOSS_VI> {
  using sum_t = double;
  // the pair of a cell: h(T) for a class the point would join, h(T - 1) for its own
  static __device__ __forceinline__ const double* at(const void* tabT, int a, int own) {
    return (const double*)tabT + 2 * a + own;
  }
  static __device__ __forceinline__ sum_t staged(double g) { return g; }
  static constexpr int kStride = 2;
};
template <>
struct RfCell<HDPM_LOSS_BINDER> {
  using sum_t = unsigned long long;
  static __device__ __forceinline__ const uint32_t* at(const void* tabT, int a, int) {
    return (const uint32_t*)tabT + a;
  }
  static __device__ __forceinline__ sum_t staged(double g) { return (sum_t)__double_as_longlong(g); }
  static constexpr int kStride = 1;
};

// Points i0 .. i0 + words / (Ka + 1) - 1 (all below N); out[(i - i0) * (Ka + 1) + b], eight
// bytes each.  A label byte >= Kz adds nothing, as in k_tr_affinity.
template <int LOSS>
__global__ __launch_bounds__(kRfThreads) void k_rf_sums(const uint8_t* __restrict__ lab,
                                                       const uint8_t* __restrict__ cls, int Np, int M, int Ka, int Kz,
                                                       const void* __restrict__ tabT, int i0, int64_t words,
                                                       typename RfCell<LOSS>::sum_t* __restrict__ out) {
  using sum_t = typename RfCell<LOSS>::sum_t;
  const int64_t q = (int64_t)blockIdx.x * kRfThreads + threadIdx.x;
  if (q >= words) return;
  const int L = Ka + 1;
  const int p = (int)(q / L), b = (int)(q - (int64_t)p * L);
  sum_t acc = 0;
  if (b < Ka) {
    const uint8_t* z = lab + i0 + p;
    const auto* T = RfCell<LOSS>::at(tabT, b, (int)cls[i0 + p] == b ? 1 : 0);
    const int64_t tsz = (int64_t)Ka * Kz * RfCell<LOSS>::kStride;
    const int zs = Ka * RfCell<LOSS>::kStride;
    int m = 0;
    for (; m + kRfUnroll <= M; m += kRfUnroll) {
      int zb[kRfUnroll];
      sum_t v[kRfUnroll];
#pragma unroll
      for (int k = 0; k < kRfUnroll; ++k) zb[k] = (int)z[(int64_t)(m + k) * Np];
#pragma unroll
      for (int k = 0; k < kRfUnroll; ++k) v[k] = zb[k] < Kz ? (sum_t)T[(m + k) * tsz + zb[k] * zs] : (sum_t)0;
#pragma unroll
      for (int k = 0; k < kRfUnroll; ++k) acc = acc + v[k];
    }
    for (; m < M; ++m) {
      const int zb = (int)z[(int64_t)m * Np];
      if (zb < Kz) acc = acc + (sum_t)T[m * tsz + zb * zs];
    }
  }
  out[q] = acc;
}

// ct: VI h(n_b) for b = 0..Ka (h(n_Ka) = h(0) = 0) then h(n_a - 1) for a = 0..Ka-1; Binder
// n_b for b = 0..Ka (n_Ka = 0), as doubles.  stage is read as the sums and, with `full`,
// written as the gains (the doubles' bits) in place.
template <int LOSS>
__global__ __launch_bounds__(kRfThreads) void k_rf_best(typename RfCell<LOSS>::sum_t* stage,
                                                       const uint8_t* __restrict__ cls, int Ka, int i0, int npts,
                                                       const double* __restrict__ ct, double dM, double dMN, int full,
                                                       int32_t* __restrict__ best, double* __restrict__ gain) {
  const int p = blockIdx.x * kRfThreads + threadIdx.x;
  if (p >= npts) return;
  const int L = Ka + 1;
  auto* row = stage + (int64_t)p * L;
  const int a = (int)cls[i0 + p];
  const auto own = row[a];
  const long long iM = (long long)dM;
  int bb = a;
  double bg = 0.0;
  for (int b = 0; b < L; ++b) {
    double g;
    if (b == a) g = 0.0;
    else if (b == 255) g = INFINITY;
    else if (LOSS == HDPM_LOSS_VI) g = (dM * (ct[b] - ct[L + a]) - 2.0 * ((double)row[b] - (double)own)) / dMN;
    else
      g = (double)(iM * ((long long)ct[b] - (long long)ct[a] - 1ll) -
                   2ll * ((long long)row[b] - (long long)own));
    if (full) row[b] = RfCell<LOSS>::staged(g);
    if (g < bg) {
      bg = g;
      bb = b;
    }
  }
  best[p] = bb;
  gain[p] = bg;
}

// ------------------------------------------------------------------------------ launchers

hipError_t launch_rf_htable(const uint32_t* tab, int M, int Ka, int Kz, double* tabH, hipStream_t s) {
  const int64_t tot = (int64_t)M * Ka * Kz;
  hipLaunchKernelGGL(k_rf_htable, dim3((unsigned)((tot + kRfThreads - 1) / kRfThreads)), dim3(kRfThreads), 0, s, tab,
                     M, Ka, Kz, (double2*)tabH);
  return hipGetLastError();
}

template <int LOSS>
static hipError_t rf_gains(const uint8_t* lab, const uint8_t* cls, int Np, int M, int Ka, int Kz, const void* tabT,
                           int i0, int npts, const double* ct, int N, int full, uint64_t* stage, int32_t* best,
                           double* gain, hipStream_t s) {
  using sum_t = typename RfCell<LOSS>::sum_t;
  const int64_t words = (int64_t)npts * (Ka + 1);
  hipLaunchKernelGGL(k_rf_sums<LOSS>, dim3((unsigned)((words + kRfThreads - 1) / kRfThreads)), dim3(kRfThreads), 0, s,
                     lab, cls, Np, M, Ka, Kz, tabT, i0, words, (sum_t*)stage);
  hipLaunchKernelGGL(k_rf_best<LOSS>, dim3((unsigned)((npts + kRfThreads - 1) / kRfThreads)), dim3(kRfThreads), 0, s,
                     (sum_t*)stage, cls, Ka, i0, npts, ct, (double)M, (double)M * (double)N, full, best, gain);
  return hipGetLastError();
}

// npts points from i0 (i0 + npts <= N): stage holds npts x (Ka + 1) eight-byte words (the
// gains as doubles afterwards, if full), best / gain npts each.  tabT is launch_rf_htable's
// array for HDPM_LOSS_VI and launch_tr_transpose's for HDPM_LOSS_BINDER.
hipError_t launch_rf_gains(int loss, const uint8_t* lab, const uint8_t* cls, int Np, int M, int Ka, int Kz,
                           const void* tabT, int i0, int npts, const double* ct, int N, int full, uint64_t* stage,
                           int32_t* best, double* gain, hipStream_t s) {
  return loss == HDPM_LOSS_VI
             ? rf_gains<HDPM_LOSS_VI>(lab, cls, Np, M, Ka, Kz, tabT, i0, npts, ct, N, full, stage, best, gain, s)
             : rf_gains<HDPM_LOSS_BINDER>(lab, cls, Np, M, Ka, Kz, tabT, i0, npts, ct, N, full, stage, best, gain, s);
}

}  // namespace hdpm
