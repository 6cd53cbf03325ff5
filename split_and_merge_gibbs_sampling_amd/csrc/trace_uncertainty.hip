// trace_uncertainty.hip -- how far a point estimate can be trusted, from the saved labels and
// the contingency tables of trace_summary.hip, with no N x N matrix.
//
// With T^m[a][b] = #{j: c_j = a, z_m(j) = b} the table of the estimate c against draw z_m:
//
//   aff[i][a]   = sum_m T^m[a][z_m(i)]               = M sum_{j: c_j = a} psm_ij
//   cross[a][b] = sum_m sum_z T^m[a][z] T^m[b][z]    = M sum_{i in a, j in b} psm_ij
//               = sum_{i: c_i = a} aff[i][b]
//
//   k_tr_transpose  the tables of one candidate as tabT[m][b][a]: the Ka counts that one
//                   (point, draw) adds are contiguous
//   k_tr_affinity   one thread per (point, cluster) of a block of points: the thread owns
//                   aff[i][a], keeps its 64-bit sum in a register over the M draws and
//                   stores it once.  Consecutive lanes are consecutive clusters of one point,
//                   then the next point, so a wave is full for any Ka, reads consecutive
//                   words of a column of tabT and writes consecutive words of aff
//   k_tr_cross      one thread per pair a <= b and slice of the draws: the products of two
//                   columns of tabT summed over z and its draws in 64 bits, then one integer
//                   atomic add per side of the diagonal
//
// Counts of points are uint32 and every sum over draws or pairs is 64-bit; the only atomics
// are the integer adds of k_tr_cross, so every output is the same from run to run and does
// not depend on how the points are cut into blocks.
//
// Bound: k_tr_affinity issues M x N x Ka four-byte reads into tables of M x Ka x Kz x 4
// bytes, which sit in L2 or the Infinity Cache at ordinary sizes, and one label byte per
// read: the M label bytes of a point are fetched once per block pass and shared by the Ka
// lanes of the point through the vector cache.  k_tr_cross is M x Kz x Ka (Ka + 1) / 2
// multiply-adds on the same tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "summary_launch.hpp"

namespace hdpm {

constexpr int kTuThreads = 256;
constexpr int kTuUnroll = 4;          // draws whose label and table reads are in flight together
constexpr int kTuCrossSlices = 64;    // slices of the draws in k_tr_cross: atomics per output word at most

// tab is M x Ka x Kz (k_tr_tables, one candidate); tabT is M x Kz x Ka
__global__ __launch_bounds__(kTuThreads) void k_tr_transpose(const uint32_t* __restrict__ tab, int M, int Ka, int Kz,
                                                            uint32_t* __restrict__ tabT) {
  const int64_t t = (int64_t)blockIdx.x * kTuThreads + threadIdx.x;
  const int cells = Ka * Kz;
  if (t >= (int64_t)M * cells) return;
  const int m = (int)(t / cells), r = (int)(t % cells);
  const int b = r / Ka, a = r % Ka;
  tabT[t] = tab[(int64_t)m * cells + a * Kz + b];
}

// Points i0 .. i0 + words / Ka - 1 (all below N); out[(i - i0) * Ka + a].  A label byte that
// is padding (0xFF) or >= Kz adds nothing, as in k_tr_gather.
__global__ __launch_bounds__(kTuThreads) void k_tr_affinity(const uint8_t* __restrict__ lab, int Np, int M, int Ka,
                                                           int Kz, const uint32_t* __restrict__ tabT, int i0,
                                                           int64_t words, unsigned long long* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * kTuThreads + threadIdx.x;
  if (q >= words) return;
  const int p = (int)(q / Ka), a = (int)(q - (int64_t)p * Ka);
  const uint8_t* z = lab + i0 + p;
  const uint32_t* T = tabT + a;
  const int64_t tsz = (int64_t)Ka * Kz;
  unsigned long long acc = 0ull;
  int m = 0;
  for (; m + kTuUnroll <= M; m += kTuUnroll) {
    int zb[kTuUnroll];
    uint32_t v[kTuUnroll];
#pragma unroll
    for (int k = 0; k < kTuUnroll; ++k) zb[k] = (int)z[(int64_t)(m + k) * Np];
#pragma unroll
    for (int k = 0; k < kTuUnroll; ++k) v[k] = zb[k] < Kz ? T[(m + k) * tsz + zb[k] * Ka] : 0u;
#pragma unroll
    for (int k = 0; k < kTuUnroll; ++k) acc += (unsigned long long)v[k];
  }
  for (; m < M; ++m) {
    const int zb = (int)z[(int64_t)m * Np];
    if (zb < Kz) acc += (unsigned long long)T[m * tsz + zb * Ka];
  }
  out[q] = acc;
}

// cross (Ka x Ka) must be zero.  blockIdx.y = slice of the draws (m = y, y + gridDim.y, ..).
// A count is below 2^31 and sum_z T[a][z] T[b][z] <= n_a n_b, so the sums stay below N^2 M.
__global__ __launch_bounds__(kTuThreads) void k_tr_cross(const uint32_t* __restrict__ tabT, int M, int Ka, int Kz,
                                                        unsigned long long* cross) {
  const int q = blockIdx.x * kTuThreads + threadIdx.x;
  if (q >= Ka * Ka) return;
  const int a = q / Ka, b = q % Ka;
  if (b < a) return;
  unsigned long long acc = 0ull;
  for (int m = blockIdx.y; m < M; m += gridDim.y) {
    const uint32_t* T = tabT + (int64_t)m * Ka * Kz;
    for (int zb = 0; zb < Kz; ++zb) acc += (unsigned long long)T[zb * Ka + a] * (unsigned long long)T[zb * Ka + b];
  }
  if (acc) {
    atomicAdd(&cross[a * Ka + b], acc);
    if (a != b) atomicAdd(&cross[b * Ka + a], acc);
  }
}

// ------------------------------------------------------------------------------ launchers

hipError_t launch_tr_transpose(const uint32_t* tab, int M, int Ka, int Kz, uint32_t* tabT, hipStream_t s) {
  const int64_t tot = (int64_t)M * Ka * Kz;
  hipLaunchKernelGGL(k_tr_transpose, dim3((unsigned)((tot + kTuThreads - 1) / kTuThreads)), dim3(kTuThreads), 0, s, tab,
                     M, Ka, Kz, tabT);
  return hipGetLastError();
}

// npts points from i0 (i0 + npts <= N); out holds npts x Ka words
hipError_t launch_tr_affinity(const uint8_t* lab, int Np, int M, int Ka, int Kz, const uint32_t* tabT, int i0, int npts,
                              uint64_t* out, hipStream_t s) {
  const int64_t words = (int64_t)npts * Ka;
  hipLaunchKernelGGL(k_tr_affinity, dim3((unsigned)((words + kTuThreads - 1) / kTuThreads)), dim3(kTuThreads), 0, s, lab,
                     Np, M, Ka, Kz, tabT, i0, words, (unsigned long long*)out);
  return hipGetLastError();
}

// cross (Ka x Ka) must be zero
hipError_t launch_tr_cross(const uint32_t* tabT, int M, int Ka, int Kz, uint64_t* cross, hipStream_t s) {
  hipLaunchKernelGGL(k_tr_cross, dim3((unsigned)((Ka * Ka + kTuThreads - 1) / kTuThreads), std::min(M, kTuCrossSlices)),
                     dim3(kTuThreads), 0, s, tabT, M, Ka, Kz, (unsigned long long*)cross);
  return hipGetLastError();
}

}  // namespace hdpm
