// trace_summary.hip -- posterior point estimates from the saved labels, with no N x N matrix.
//
// posterior.hip builds comp.psm(C) as N x N counts; that is 19.6 GB at C4 (N = 70k) and 4 TB
// at C5 (N = 1M).  Every quantity the reference's analysis needs (zoo_simulator.R:193-236,
// 339-344: minVI, and Binder's loss beside it) follows from the contingency tables of a
// candidate partition c against every saved draw z_m, T^m[a][b] = #{j: c_j = a, z_m(j) = b},
// and the draws' cluster sizes n^m_b:
//
//   sum_j psm_ij                = (1/M) sum_m n^m[z_m(i)]
//   sum_{j: c_j = c_i} psm_ij   = (1/M) sum_m T^m[c_i][z_m(i)]
//   E[VI(c, z)]                 = (1/N) [sum_a n_a log2 n_a
//                                        + (1/M) sum_m (sum_b n^m_b log2 n^m_b - 2 sum_ab T^m log2 T^m)]
//   Binder                      = sum_a C2(n_a) + (sum_m sum_b C2(n^m_b) - 2 sum_m sum_ab C2(T^m)) / M
//
//   k_tr_pack     a block of draws (int32) to one byte per label, draw-major, points fastest,
//                 rows padded to a multiple of 16 points with 0xFF
//   k_tr_sizes    n^m_b of every draw (M x 256 uint32)
//   k_tr_tables   T^m of a block of candidates against every draw: LDS histograms over a
//                 chunk of points, flushed with integer atomics to a compact global array
//   k_tr_gather   per point: sum_m n^m[z_m(i)] and, per candidate, sum_m T^m[c_i][z_m(i)]
//   k_tr_reduce / k_tr_reduce_draws   per candidate: sum C2(T) (uint64) and sum T log2 T
//                 (double), ordered partial sums and fixed-order trees
//
// Counts of points are uint32, every sum over draws or pairs is 64-bit, and the only
// atomics are integer adds, so every output is the same from run to run and does not
// depend on how the candidates are split into blocks.
//
// Bound: k_tr_tables issues one LDS add per (point, draw, candidate); k_tr_gather one
// 4-byte gather per (point, draw, candidate) into tables that stay in L2.  Both stream the
// label bytes (M x N per candidate group) from HBM / L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace hdpm {

constexpr int kTrThreads = 256;
constexpr int kTrChunk = 65536;       // points of one draw per workgroup of the histogram kernels
constexpr int kTrLdsWords = 12288;    // 48 KB of histogram per workgroup: three workgroups on a CU
constexpr int kTrGroup = 4;           // candidates that share one read of z_m

// 4 labels per thread: trace is nm x N (a block of draws), lab points at the first of them
__global__ void k_tr_pack(const int32_t* __restrict__ trace, int nm, int N, int Np, uint8_t* __restrict__ lab) {
  const int W = Np >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nm * W) return;
  const int m = (int)(t / W), i0 = (int)(t % W) * 4;
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    const uint32_t b = i < N ? (uint32_t)(uint8_t)trace[(int64_t)m * N + i] : 0xFFu;
    v |= b << (8 * k);
  }
  *(uint32_t*)(lab + (int64_t)m * Np + i0) = v;
}

__device__ __forceinline__ uint32_t byte_of(const uint4& v, int k) {
  const uint32_t w = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
  return (w >> (8 * (k & 3))) & 0xFFu;
}

// Workgroup (draw m, chunk of points, candidate group, band of candidate labels): counts
// (c_j - a0, z_m(j)) for the points of its chunk whose candidate label lies in the band
// [a0, a0 + B), for up to G candidates that share each 16-byte piece of z_m.
//
// The histogram is held `ncopies` times in LDS (a power of two, as many as fit), thread t
// adding to copy t mod ncopies: the lanes that hit one hot cell spread over the copies, and
// the odd stride between copies puts them on different banks.  A table too large for LDS
// (B < Ka) is covered by several bands, each streaming the chunk again.
//
// cls == nullptr counts the draw alone (every point in candidate cluster 0): k_tr_sizes.
__device__ __forceinline__ void tr_hist(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ cls, int Np, int M,
                                        int nchunks, int ncand, int Ka, int Kz, int B, int G, int ncopies,
                                        int cstride, int ldz, uint32_t* __restrict__ tab, uint32_t* h) {
  const int tid = threadIdx.x;
  const int m = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const int g0 = blockIdx.y * G, ng = min(G, ncand - g0);
  const int a0 = blockIdx.z * B;
  const int words = ncopies * cstride;
  for (int q = tid; q < words; q += kTrThreads) h[q] = 0u;
  __syncthreads();
  uint32_t* mine = h + (tid & (ncopies - 1)) * cstride;
  const int p0 = chunk * kTrChunk, p1 = min(p0 + kTrChunk, Np);
  const uint8_t* zr = lab + (int64_t)m * Np;
  for (int p = p0 + tid * 16; p < p1; p += kTrThreads * 16) {
    const uint4 zv = *(const uint4*)(zr + p);
    for (int g = 0; g < ng; ++g) {
      uint4 cv = make_uint4(0u, 0u, 0u, 0u);
      if (cls) cv = *(const uint4*)(cls + (int64_t)(g0 + g) * Np + p);
      uint32_t* hg = mine + g * B * Kz;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int zb = (int)byte_of(zv, k), ca = (int)byte_of(cv, k);
        const int a = ca - a0;
        if (zb < Kz && ca < Ka && a >= 0 && a < B) atomicAdd(&hg[a * Kz + zb], 1u);
      }
    }
  }
  __syncthreads();
  const int cells = G * B * Kz;
  for (int q = tid; q < cells; q += kTrThreads) {
    uint32_t s = 0;
    for (int cp = 0; cp < ncopies; ++cp) s += h[cp * cstride + q];
    const int g = q / (B * Kz), r = q % (B * Kz);
    const int a = a0 + r / Kz, b = r % Kz;
    if (s && g < ng && a < Ka) atomicAdd(&tab[(((int64_t)(g0 + g) * M + m) * Ka + a) * ldz + b], s);
  }
}

__global__ __launch_bounds__(kTrThreads) void k_tr_sizes(const uint8_t* __restrict__ lab, int Np, int M, int nchunks,
                                                        int ncopies, int cstride, uint32_t* __restrict__ sizes) {
  extern __shared__ __align__(16) uint32_t tr_lds[];
  // labels are 0..254: 255 cells, so the 0xFF padding is not counted; rows of 256 in the output
  tr_hist(lab, nullptr, Np, M, nchunks, 1, 1, 255, 1, 1, ncopies, cstride, 256, sizes, tr_lds);
}

__global__ __launch_bounds__(kTrThreads) void k_tr_tables(const uint8_t* __restrict__ lab,
                                                         const uint8_t* __restrict__ cls, int Np, int M, int nchunks,
                                                         int ncand, int Ka, int Kz, int B, int G, int ncopies,
                                                         int cstride, uint32_t* __restrict__ tab) {
  extern __shared__ __align__(16) uint32_t tr_lds[];
  tr_hist(lab, cls, Np, M, nchunks, ncand, Ka, Kz, B, G, ncopies, cstride, Kz, tab, tr_lds);
}

// 4 points per thread, blockIdx.y = candidate of the block; blockIdx.y == ncand (launched
// only when `all` is wanted) sums the draws' cluster sizes instead.
__global__ __launch_bounds__(kTrThreads) void k_tr_gather(const uint8_t* __restrict__ lab,
                                                         const uint8_t* __restrict__ cls, int N, int Np, int M,
                                                         int ncand, int Ka, int Kz, const uint32_t* __restrict__ tab,
                                                         const uint32_t* __restrict__ sizes,
                                                         unsigned long long* __restrict__ all,
                                                         unsigned long long* __restrict__ same) {
  const int p = (blockIdx.x * kTrThreads + threadIdx.x) * 4;
  if (p >= Np) return;
  const int c = blockIdx.y;
  unsigned long long acc[4] = {0ull, 0ull, 0ull, 0ull};
  if (c == ncand) {
    for (int m = 0; m < M; ++m) {
      const uint32_t zw = *(const uint32_t*)(lab + (int64_t)m * Np + p);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t zb = (zw >> (8 * k)) & 0xFFu;
        if (zb != 0xFFu) acc[k] += sizes[(int64_t)m * 256 + zb];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (p + k < N) all[p + k] = acc[k];
    return;
  }
  const uint32_t cw = *(const uint32_t*)(cls + (int64_t)c * Np + p);
  int row[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ca = (int)((cw >> (8 * k)) & 0xFFu);
    row[k] = ca < Ka ? ca * Kz : -1;
  }
  const uint32_t* T = tab + (int64_t)c * M * Ka * Kz;
  const int tsz = Ka * Kz;
  for (int m = 0; m < M; ++m) {
    const uint32_t zw = *(const uint32_t*)(lab + (int64_t)m * Np + p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int zb = (int)((zw >> (8 * k)) & 0xFFu);
      if (row[k] >= 0 && zb < Kz) acc[k] += T[(int64_t)m * tsz + row[k] + zb];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (p + k < N) same[(int64_t)c * N + p + k] = acc[k];
}

// fixed-order tree over the workgroup's partial sums (the rule k_vi_terms follows)
__device__ __forceinline__ void tr_tree(unsigned long long sq, double sl, unsigned long long* q, double* l) {
  __shared__ unsigned long long rq[kTrThreads];
  __shared__ double rl[kTrThreads];
  rq[threadIdx.x] = sq;
  rl[threadIdx.x] = sl;
  __syncthreads();
  for (int o = kTrThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      rq[threadIdx.x] += rq[threadIdx.x + o];
      rl[threadIdx.x] += rl[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *q = rq[0];
    *l = rl[0];
  }
}

// One workgroup per table (`cells` contiguous counts): sum of C2(t) and of t log2 t.  Thread
// t sums cells t, t + 256, ... in order; rows of zeros beyond a candidate's own labels add
// +0.0, so the result does not depend on the row count of the compact array.
__global__ __launch_bounds__(kTrThreads) void k_tr_reduce(const uint32_t* __restrict__ tab, int cells,
                                                         unsigned long long* __restrict__ q,
                                                         double* __restrict__ l) {
  const uint32_t* T = tab + (int64_t)blockIdx.x * cells;
  unsigned long long sq = 0ull;
  double sl = 0.0;
  for (int idx = threadIdx.x; idx < cells; idx += kTrThreads) {
    const unsigned long long t = T[idx];
    if (t > 1ull) {
      sq += t * (t - 1ull) / 2ull;
      sl += (double)t * log2((double)t);
    }
  }
  tr_tree(sq, sl, q + blockIdx.x, l + blockIdx.x);
}

// One workgroup per candidate: the M per-draw partial sums, thread t taking draws t, t + 256, ...
__global__ __launch_bounds__(kTrThreads) void k_tr_reduce_draws(const unsigned long long* __restrict__ q1,
                                                               const double* __restrict__ l1, int M,
                                                               unsigned long long* __restrict__ q,
                                                               double* __restrict__ l) {
  const unsigned long long* Q = q1 + (int64_t)blockIdx.x * M;
  const double* L = l1 + (int64_t)blockIdx.x * M;
  unsigned long long sq = 0ull;
  double sl = 0.0;
  for (int m = threadIdx.x; m < M; m += kTrThreads) {
    sq += Q[m];
    sl += L[m];
  }
  tr_tree(sq, sl, q + blockIdx.x, l + blockIdx.x);
}

// ------------------------------------------------------------------------------ launchers

hipError_t launch_tr_pack(const int32_t* trace, int nm, int N, int Np, uint8_t* lab, hipStream_t s) {
  const int64_t tot = (int64_t)nm * (Np >> 2);
  hipLaunchKernelGGL(k_tr_pack, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, trace, nm, N, Np, lab);
  return hipGetLastError();
}

static int tr_copies(int cstride) {
  int nc = 1;
  while (nc < kTrThreads && nc * 2 * cstride <= kTrLdsWords) nc *= 2;
  return nc;
}

// sizes (M x 256) must be zero
hipError_t launch_tr_sizes(const uint8_t* lab, int Np, int M, uint32_t* sizes, hipStream_t s) {
  const int nchunks = (Np + kTrChunk - 1) / kTrChunk;
  const int cstride = 255, nc = tr_copies(cstride);
  hipLaunchKernelGGL(k_tr_sizes, dim3((unsigned)((int64_t)M * nchunks)), dim3(kTrThreads),
                     (size_t)nc * cstride * 4, s, lab, Np, M, nchunks, nc, cstride, sizes);
  return hipGetLastError();
}

// tab (ncand x M x Ka x Kz) must be zero
hipError_t launch_tr_tables(const uint8_t* lab, const uint8_t* cls, int Np, int M, int ncand, int Ka, int Kz,
                            uint32_t* tab, hipStream_t s) {
  // candidates per workgroup and rows per band: what fits the LDS budget
  int G = kTrGroup, B = Ka;
  while (G > 1 && G * Ka * Kz + 1 > kTrLdsWords) G >>= 1;
  if (Ka * Kz + 1 > kTrLdsWords) {
    G = 1;
    B = (kTrLdsWords - 1) / Kz;   // Kz <= 255: at least 48 rows
  }
  G = std::min(G, ncand);
  const int nbands = (Ka + B - 1) / B;
  const int cstride = (G * B * Kz) | 1, nc = tr_copies(cstride);
  const int nchunks = (Np + kTrChunk - 1) / kTrChunk;
  hipLaunchKernelGGL(k_tr_tables, dim3((unsigned)((int64_t)M * nchunks), (unsigned)((ncand + G - 1) / G), nbands),
                     dim3(kTrThreads), (size_t)nc * cstride * 4, s, lab, cls, Np, M, nchunks, ncand, Ka, Kz, B, G,
                     nc, cstride, tab);
  return hipGetLastError();
}

hipError_t launch_tr_gather(const uint8_t* lab, const uint8_t* cls, int N, int Np, int M, int ncand, int Ka, int Kz,
                            const uint32_t* tab, const uint32_t* sizes, uint64_t* all, uint64_t* same,
                            hipStream_t s) {
  const int ny = ncand + (all ? 1 : 0);
  if (ny == 0) return hipSuccess;
  const int nb = ((Np >> 2) + kTrThreads - 1) / kTrThreads;
  hipLaunchKernelGGL(k_tr_gather, dim3(nb, ny), dim3(kTrThreads), 0, s, lab, cls, N, Np, M, ncand, Ka, Kz, tab, sizes,
                     (unsigned long long*)all, (unsigned long long*)same);
  return hipGetLastError();
}

// ntab tables of `cells` counts, M per candidate: q1 / l1 (ntab) per table, q / l (ntab / M) per candidate
hipError_t launch_tr_reduce(const uint32_t* tab, int ncand, int M, int cells, uint64_t* q1, double* l1, uint64_t* q,
                            double* l, hipStream_t s) {
  hipLaunchKernelGGL(k_tr_reduce, dim3((unsigned)((int64_t)ncand * M)), dim3(kTrThreads), 0, s, tab, cells,
                     (unsigned long long*)q1, l1);
  hipLaunchKernelGGL(k_tr_reduce_draws, dim3(ncand), dim3(kTrThreads), 0, s, (const unsigned long long*)q1, l1, M,
                     (unsigned long long*)q, l);
  return hipGetLastError();
}

}  // namespace hdpm
