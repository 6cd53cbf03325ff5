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

#include "summary_launch.hpp"

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

// ------------------------------------------------- groups of equal label columns (k_tg_*)
//
// minVI(method = "avg") / minbinder(method = "avgl") without the matrix: points whose labels
// agree in every draw have psm = 1 and merge first under average linkage, so the tree is
// built on the U distinct label columns, each weighted by its member count (trace_tree.hpp).
//
//   k_tg_insert   hash of every point's M-byte column (4 points per thread, points fastest),
//                 then an open-addressing insert: a point joins a slot only after its whole
//                 column equals the slot's representative byte for byte, else it probes on
//   k_tg_assign   group_of[i] and the member counts, once the host has numbered the slots
//                 by ascending smallest member
//   k_tg_sig      sig[U][Mp] (group-major, for the counts) and sigT[M][Up] (draw-major, a
//                 trace of U weighted points for the tables) from the smallest members
//   k_tg_counts   S[u][v] = #{m: sig_u[m] == sig_v[m]}: 64 x 64 outputs per workgroup, M in
//                 slabs of 64 bytes through LDS, 4 x 4 outputs per thread, four bytes per
//                 xor + zero-byte count
//   k_tg_tables   T^m[a][b] = sum_u w_u [cut(u) = a][sig_u[m] = b] in the layout of k_tr_tables
//   k_tg_gather   per group: sum_m n^m[sig_u[m]] and, per cut, sum_m T^m[cut(u)][sig_u[m]]
//   k_tg_expand   a cut of the groups to labels per point
//
// The slot a column lands in depends on the insertion order; nothing else does: a column is
// claimed by exactly one slot (its probe sequence is fixed and slots never empty), the
// smallest member is an atomicMin, and the groups are numbered by that.

constexpr uint32_t kTgEmpty = 0xFFFFFFFFu;
constexpr int kTgTile = 64;      // outputs of k_tg_counts per workgroup, each way
constexpr int kTgSlab = 64;      // bytes of M per LDS slab: Mp is a multiple
constexpr int kTgLd = 17;        // words per LDS row (16 + 1: rows on different banks)

__device__ __forceinline__ uint32_t tg_mix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// rep / first: tmask + 1 slots, both 0xFF.. before the launch.  ctl[0] counts the slots
// claimed; ctl[1] is set when more than max_groups are (or the table is full) and stops
// every thread at its next point.
__global__ __launch_bounds__(kTrThreads) void k_tg_insert(const uint8_t* __restrict__ lab, int N, int Np, int M,
                                                         uint32_t hmask, uint32_t tmask, uint32_t max_groups,
                                                         uint32_t* rep, uint32_t* first, uint32_t* __restrict__ pslot,
                                                         uint32_t* ctl) {
  const int p = (blockIdx.x * kTrThreads + threadIdx.x) * 4;
  if (p >= N) return;
  uint32_t h[4] = {2166136261u, 2166136261u, 2166136261u, 2166136261u};
  for (int m = 0; m < M; ++m) {
    const uint32_t zw = *(const uint32_t*)(lab + (int64_t)m * Np + p);
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = (h[k] ^ ((zw >> (8 * k)) & 0xFFu)) * 16777619u;
  }
  for (int k = 0; k < 4; ++k) {
    const uint32_t i = (uint32_t)(p + k);
    if (i >= (uint32_t)N) return;
    if (__atomic_load_n(&ctl[1], __ATOMIC_RELAXED)) return;
    uint32_t slot = tg_mix(h[k]) & hmask & tmask;
    bool placed = false;
    for (uint32_t probe = 0; probe <= tmask; ++probe, slot = (slot + 1u) & tmask) {
      uint32_t r = __atomic_load_n(&rep[slot], __ATOMIC_RELAXED);
      if (r == kTgEmpty) {
        r = atomicCAS(&rep[slot], kTgEmpty, i);
        if (r == kTgEmpty) {
          if (atomicAdd(&ctl[0], 1u) >= max_groups) {
            atomicExch(&ctl[1], 1u);
            return;
          }
          r = i;
        }
      }
      bool eq = true;
      if (r != i)
        for (int m = 0; m < M; ++m)
          if (lab[(int64_t)m * Np + i] != lab[(int64_t)m * Np + r]) {
            eq = false;
            break;
          }
      if (eq) {
        if (i < __atomic_load_n(&first[slot], __ATOMIC_RELAXED)) atomicMin(&first[slot], i);
        pslot[i] = slot;
        placed = true;
        break;
      }
    }
    if (!placed) {
      atomicExch(&ctl[1], 1u);
      return;
    }
  }
}

// weight (U) must be zero
__global__ __launch_bounds__(kTrThreads) void k_tg_assign(const uint32_t* __restrict__ pslot,
                                                         const uint32_t* __restrict__ slot_gid, int N,
                                                         uint32_t* __restrict__ group_of, uint32_t* weight) {
  const int i = blockIdx.x * kTrThreads + threadIdx.x;
  if (i >= N) return;
  const uint32_t g = slot_gid[pslot[i]];
  group_of[i] = g;
  atomicAdd(&weight[g], 1u);
}

// one thread per (group, draw) of the padded arrays: bytes beyond U or M are 0
__global__ __launch_bounds__(kTrThreads) void k_tg_sig(const uint8_t* __restrict__ lab, int Np, int M, int U, int Mp,
                                                      int Up, const uint32_t* __restrict__ first,
                                                      uint8_t* __restrict__ sig, uint8_t* __restrict__ sigT) {
  const int64_t t = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
  if (t >= (int64_t)Up * Mp) return;
  const int u = (int)(t % Up), m = (int)(t / Up);
  const uint8_t b = (u < U && m < M) ? lab[(int64_t)m * Np + first[u]] : (uint8_t)0;
  if (u < U) sig[(int64_t)u * Mp + m] = b;
  if (m < M) sigT[(int64_t)m * Up + u] = b;
}

// zero bytes of x, four at a time
__device__ __forceinline__ uint32_t tg_zero_bytes(uint32_t x) {
  uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  t = ~(t | x | 0x7F7F7F7Fu);
  return (uint32_t)__popc(t);
}

// `pad` = Mp - M: the padding bytes are 0 in every row and count as matches
__global__ __launch_bounds__(kTrThreads) void k_tg_counts(const uint8_t* __restrict__ sig, int U, int Mp, uint32_t pad,
                                                         uint32_t* __restrict__ S) {
  __shared__ uint32_t A[kTgTile * kTgLd], B[kTgTile * kTgLd];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int u0 = blockIdx.y * kTgTile, v0 = blockIdx.x * kTgTile;
  const int lr = tid >> 2, lq = (tid & 3) * 4;     // the row and first word this thread loads
  uint32_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0u;
  for (int s = 0; s < Mp; s += kTgSlab) {
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (u0 + lr < U) a = *(const uint4*)(sig + (int64_t)(u0 + lr) * Mp + s + lq * 4);
    if (v0 + lr < U) b = *(const uint4*)(sig + (int64_t)(v0 + lr) * Mp + s + lq * 4);
    uint32_t* ar = A + lr * kTgLd + lq;
    uint32_t* br = B + lr * kTgLd + lq;
    ar[0] = a.x; ar[1] = a.y; ar[2] = a.z; ar[3] = a.w;
    br[0] = b.x; br[1] = b.y; br[2] = b.z; br[3] = b.w;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTgSlab / 4; ++k) {
      uint32_t av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[i] = A[(ty + 16 * i) * kTgLd + k];
        bv[i] = B[(tx + 16 * i) * kTgLd + k];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += tg_zero_bytes(av[i] ^ bv[j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int u = u0 + ty + 16 * i, v = v0 + tx + 16 * j;
      if (u < U && v < U) S[(int64_t)u * U + v] = acc[i][j] - pad;
    }
}

// One workgroup per (draw, cut): the table in LDS when Ka x Kz words fit (lds != 0), else
// added straight to the global table.  tab must be zero.
__global__ __launch_bounds__(kTrThreads) void k_tg_tables(const uint8_t* __restrict__ sigT,
                                                         const uint8_t* __restrict__ cut,
                                                         const uint32_t* __restrict__ w, int U, int Up, int M, int Ka,
                                                         int Kz, int lds, uint32_t* tab) {
  extern __shared__ __align__(16) uint32_t tr_lds[];
  const int m = blockIdx.x, c = blockIdx.y, cells = Ka * Kz;
  uint32_t* T = tab + ((int64_t)c * M + m) * cells;
  if (lds) {
    for (int q = threadIdx.x; q < cells; q += kTrThreads) tr_lds[q] = 0u;
    __syncthreads();
  }
  uint32_t* dst = lds ? tr_lds : T;
  for (int u = threadIdx.x; u < U; u += kTrThreads) {
    const int a = cut[(int64_t)c * Up + u], b = sigT[(int64_t)m * Up + u];
    if (a < Ka && b < Kz) atomicAdd(&dst[a * Kz + b], w[u]);
  }
  if (lds) {
    __syncthreads();
    for (int q = threadIdx.x; q < cells; q += kTrThreads)
      if (tr_lds[q]) T[q] = tr_lds[q];
  }
}

// blockIdx.y = cut of the block; blockIdx.y == ncut (launched only when `all` is wanted)
// sums the draws' cluster sizes instead
__global__ __launch_bounds__(kTrThreads) void k_tg_gather(const uint8_t* __restrict__ sigT,
                                                         const uint8_t* __restrict__ cut, int U, int Up, int M,
                                                         int ncut, int Ka, int Kz, const uint32_t* __restrict__ tab,
                                                         const uint32_t* __restrict__ sizes,
                                                         unsigned long long* __restrict__ all,
                                                         unsigned long long* __restrict__ same) {
  const int u = blockIdx.x * kTrThreads + threadIdx.x;
  if (u >= U) return;
  const int c = blockIdx.y;
  unsigned long long acc = 0ull;
  if (c == ncut) {
    for (int m = 0; m < M; ++m) {
      const uint32_t b = sigT[(int64_t)m * Up + u];
      if (b != 0xFFu) acc += sizes[(int64_t)m * 256 + b];
    }
    all[u] = acc;
    return;
  }
  const int a = cut[(int64_t)c * Up + u];
  const uint32_t* T = tab + (int64_t)c * M * Ka * Kz;
  if (a < Ka)
    for (int m = 0; m < M; ++m) {
      const int b = sigT[(int64_t)m * Up + u];
      if (b < Kz) acc += T[((int64_t)m * Ka + a) * Kz + b];
    }
  same[(int64_t)c * U + u] = acc;
}

__global__ __launch_bounds__(kTrThreads) void k_tg_expand(const uint32_t* __restrict__ group_of,
                                                         const int32_t* __restrict__ cut, int N,
                                                         int32_t* __restrict__ cl) {
  const int i = blockIdx.x * kTrThreads + threadIdx.x;
  if (i < N) cl[i] = cut[group_of[i]];
}

// rep / first (tslots each) must be 0xFF.., ctl (2 words) zero; tslots a power of two
hipError_t launch_tg_insert(const uint8_t* lab, int N, int Np, int M, int hash_bits, uint32_t tslots,
                            uint32_t max_groups, uint32_t* rep, uint32_t* first, uint32_t* pslot, uint32_t* ctl,
                            hipStream_t s) {
  const uint32_t hmask = hash_bits <= 0 || hash_bits >= 32 ? 0xFFFFFFFFu : (1u << hash_bits) - 1u;
  const int nb = (((N + 3) >> 2) + kTrThreads - 1) / kTrThreads;
  hipLaunchKernelGGL(k_tg_insert, dim3(nb), dim3(kTrThreads), 0, s, lab, N, Np, M, hmask, tslots - 1u, max_groups, rep,
                     first, pslot, ctl);
  return hipGetLastError();
}

// weight (U) must be zero; sig is U x Mp, sigT is M x Up
hipError_t launch_tg_finish(const uint8_t* lab, int N, int Np, int M, int U, int Mp, int Up, const uint32_t* pslot,
                            const uint32_t* slot_gid, const uint32_t* first, uint32_t* group_of, uint32_t* weight,
                            uint8_t* sig, uint8_t* sigT, hipStream_t s) {
  hipLaunchKernelGGL(k_tg_assign, dim3((N + kTrThreads - 1) / kTrThreads), dim3(kTrThreads), 0, s, pslot, slot_gid, N,
                     group_of, weight);
  const int64_t tot = (int64_t)Up * Mp;
  hipLaunchKernelGGL(k_tg_sig, dim3((unsigned)((tot + kTrThreads - 1) / kTrThreads)), dim3(kTrThreads), 0, s, lab, Np,
                     M, U, Mp, Up, first, sig, sigT);
  return hipGetLastError();
}

hipError_t launch_tg_counts(const uint8_t* sig, int U, int M, int Mp, uint32_t* S, hipStream_t s) {
  const int nt = (U + kTgTile - 1) / kTgTile;
  hipLaunchKernelGGL(k_tg_counts, dim3(nt, nt), dim3(kTrThreads), 0, s, sig, U, Mp, (uint32_t)(Mp - M), S);
  return hipGetLastError();
}

// tab (ncut x M x Ka x Kz) must be zero; cut is ncut x Up bytes
hipError_t launch_tg_tables(const uint8_t* sigT, const uint8_t* cut, const uint32_t* w, int U, int Up, int M, int ncut,
                            int Ka, int Kz, uint32_t* tab, hipStream_t s) {
  const int lds = Ka * Kz <= kTrLdsWords ? 1 : 0;
  hipLaunchKernelGGL(k_tg_tables, dim3(M, ncut), dim3(kTrThreads), lds ? (size_t)Ka * Kz * 4 : 0, s, sigT, cut, w, U,
                     Up, M, Ka, Kz, lds, tab);
  return hipGetLastError();
}

hipError_t launch_tg_gather(const uint8_t* sigT, const uint8_t* cut, int U, int Up, int M, int ncut, int Ka, int Kz,
                            const uint32_t* tab, const uint32_t* sizes, uint64_t* all, uint64_t* same, hipStream_t s) {
  const int ny = ncut + (all ? 1 : 0);
  if (ny == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tg_gather, dim3((U + kTrThreads - 1) / kTrThreads, ny), dim3(kTrThreads), 0, s, sigT, cut, U, Up,
                     M, ncut, Ka, Kz, tab, sizes, (unsigned long long*)all, (unsigned long long*)same);
  return hipGetLastError();
}

hipError_t launch_tg_expand(const uint32_t* group_of, const int32_t* cut, int N, int32_t* cl, hipStream_t s) {
  hipLaunchKernelGGL(k_tg_expand, dim3((N + kTrThreads - 1) / kTrThreads), dim3(kTrThreads), 0, s, group_of, cut, N,
                     cl);
  return hipGetLastError();
}

}  // namespace hdpm
