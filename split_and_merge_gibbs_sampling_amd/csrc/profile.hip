// profile.hip -- what each class of a point estimate is: the centers and sigmas of its members
// across the recorded draws (hdpm_predict_profile, include/hdpm.h).
//
// For a point i of class a, draw s says "your center is c^s_{z_s(i)}, your sigma is
// sg^s_{z_s(i)}".  Summed over the members of a, the draw's clusters enter with the counts of
// the contingency table T^s[a][k] (k_tr_tables), so no label of one draw is matched with a label
// of another.  With the parameter tables of predict.hip (a center byte, the raw sigma and the
// (exp(match), exp(mismatch)) pair per (s, k, j)):
//
//   k_pf_sigma    u_s[a][j] = (sum_k (double)T^s[a][k] * sg^s_kj) / n_a, a workgroup per (draw,
//                 class), its lanes over the attributes: the count is wave-uniform (a scalar
//                 load, zero counts skipped: they add +0.0) and the sigmas are read coalesced
//                 over j.  k in cluster order, plain multiply and add.  The draws come in chunks
//                 whose u_s (Ka x d doubles per draw) obey the table budget.
//   k_pf_welford  a lane per (class, attribute) folds a chunk's u_s into (mean, m2) in draw
//                 order, carried between chunks in st, double for double.
//   k_pf_levels   a lane per (class, attribute), a wave over consecutive attributes of one
//                 class.  The lane walks the draws and the clusters with non-zero count and
//                 owns the ld slots of its level rows, kept in LDS during the walk, so its
//                 read-modify-writes need no atomics and no barrier: cnt[c - 1] += T, and for
//                 the code law base += T ei and law[c - 1] += T (em - ei), one update per (s, k)
//                 whatever ld is; at the end slot l becomes (base + law[l]) / (M n_a) and the
//                 rows go to the staging.  64 KB of LDS hold 64 lanes' rows up to ld = 64 with
//                 both outputs; above that fewer lanes of the wave work (16 at ld = 255): the
//                 walk is bound by latency, not by lanes.  The parameters of four clusters are
//                 fetched together, so one memory latency covers four updates.  The attributes
//                 come in blocks whose level rows obey the table budget.
//
// Every sum of a (class, attribute) runs in one lane, over s in draw order and then k in cluster
// order, so no result depends on the block of attributes, the chunk of draws or the grid.
//
// Bound.  k_pf_sigma reads per draw Ka x Kz counts (4 B) and, per non-zero count, d sigmas
// (8 B): at most M min(Ka K, N) d 8 bytes, each draw's K x d sigmas re-read per class from L2
// (160 KB at K = 20, d = 128), and writes M Ka d 8 bytes: a streaming kernel, M Ka workgroups.
// k_pf_levels reads per block of attributes the same counts and, per non-zero count and lane,
// a center byte and a 16-byte pair (coalesced over j): at most M min(Ka K, N) d 17 bytes, the
// draw's tables re-read per class from L2 as above; its two 8-byte read-modify-writes per lane
// and non-zero (s, k) stay in LDS (~64 cycles each, a dependent read, add and write), and the
// level rows leave once, Ka x d x ld x 16 bytes.  With Ka x d lanes in all (2,560 at Ka = 20,
// d = 128: 40 waves on 256 CUs) the walk is bound by its depth, not by bytes: per lane M K / 4
// global round trips and M K dependent LDS updates.  Measured at M = 64, K = 20: 0.2 us per
// (draw, cluster) step, 0.21 - 0.29 ms a launch, where the bytes (82 MB at most) would take tens
// of microseconds (profiles/profile/).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "summary_launch.hpp"

namespace hdpm {

__global__ __launch_bounds__(kPfThreads) void k_pf_sigma(PfSigArgs p) {
  const int a = blockIdx.x % p.Ka, s = p.s0 + blockIdx.x / p.Ka;
  const int64_t base = p.off[s];
  const int K = (int)(p.off[s + 1] - base), d = p.d;
  const uint32_t* __restrict__ T = p.tab + ((int64_t)s * p.Ka + a) * p.Kz;
  const double* __restrict__ sg = p.sig + base * d;
  const double na = p.na[a];
  double* __restrict__ out = p.u + ((int64_t)(s - p.s0) * p.Ka + a) * d;
  for (int j = threadIdx.x; j < d; j += blockDim.x) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const uint32_t n = T[k];
      if (n) acc = acc + (double)n * sg[(int64_t)k * d + j];
    }
    out[j] = na > 0.0 ? acc / na : 0.0;
  }
}

__global__ __launch_bounds__(256) void k_pf_welford(PfWelArgs p) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.n) return;
  double mean = 0.0, m2 = 0.0;
  if (p.s0 > 0) {
    mean = p.st[q];
    m2 = p.st[p.n + q];
  }
  for (int s = p.s0; s < p.s1; ++s) {
    const double u = p.u[(int64_t)(s - p.s0) * p.n + q];
    const double delta = u - mean;
    mean = mean + delta / (double)(s + 1);
    m2 = m2 + delta * (u - mean);
  }
  if (p.s1 < p.M) {
    p.st[q] = mean;
    p.st[p.n + q] = m2;
    return;
  }
  if (p.mean) p.mean[q] = mean;
  if (p.var) p.var[q] = p.M > 1 ? m2 / ((double)p.M - 1.0) : 0.0;
}

__global__ __launch_bounds__(64) void k_pf_levels(PfLevArgs p) {
  extern __shared__ double s_lev[];                   // [level][lane]: the laws, then the counts
  const int L = p.lanes, lane = threadIdx.x, a = blockIdx.y, jj = blockIdx.x * L + lane;
  if (lane >= L || jj >= p.jb) return;                // no barrier below: a lane's slots are its own
  const int j = p.j0 + jj, d = p.d, d4 = (d + 3) & ~3, ld = p.ld;
  const bool want_cnt = p.cnt != nullptr, want_law = p.law != nullptr;
  double* s_law = s_lev + lane;
  uint64_t* s_cnt = (uint64_t*)(s_lev + (want_law ? ld * L : 0)) + lane;
  for (int l = 0; l < ld; ++l) {
    if (want_law) s_law[l * L] = 0.0;
    if (want_cnt) s_cnt[l * L] = 0;
  }
  const uint8_t* __restrict__ cen = p.cen;
  const double2* __restrict__ emm = (const double2*)p.emm;
  double base = 0.0;
  for (int s = 0; s < p.M; ++s) {
    const int64_t r0 = p.off[s];
    const int K = (int)(p.off[s + 1] - r0);
    const uint32_t* __restrict__ T = p.tab + ((int64_t)s * p.Ka + a) * p.Kz;
    for (int k0 = 0; k0 < K; k0 += kPfGroup) {
      // the counts of kPfGroup clusters (wave-uniform); a cluster past the last counts 0
      uint32_t n[kPfGroup], any = 0;
#pragma unroll
      for (int g = 0; g < kPfGroup; ++g) {
        n[g] = k0 + g < K ? T[k0 + g] : 0u;
        any |= n[g];
      }
      if (!any) continue;
      // their parameters fetched together, then the updates in cluster order
      int c[kPfGroup];
      double2 v[kPfGroup];
#pragma unroll
      for (int g = 0; g < kPfGroup; ++g) {
        const int64_t r = r0 + min(k0 + g, K - 1);
        c[g] = cen[r * d4 + j];                       // 1..m_j <= ld (checked at the build and by the call)
        v[g] = want_law ? emm[r * d + j] : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int g = 0; g < kPfGroup; ++g) {
        if (!n[g]) continue;                          // wave-uniform
        const int q = (c[g] - 1) * L;
        if (want_cnt) s_cnt[q] += n[g];
        if (want_law) {
          const double t = (double)n[g];
          base = base + t * v[g].y;
          s_law[q] = s_law[q] + t * (v[g].x - v[g].y);
        }
      }
    }
  }
  const int64_t slot = ((int64_t)a * p.jb + jj) * ld;
  if (want_cnt)
    for (int l = 0; l < ld; ++l) p.cnt[slot + l] = s_cnt[l * L];
  if (want_law) {
    const int m = p.att[j];
    const double na = p.na[a], den = (double)p.M * na;
    for (int l = 0; l < ld; ++l) p.law[slot + l] = (na > 0.0 && l < m) ? (base + s_law[l * L]) / den : 0.0;
  }
}

// ------------------------------------------------------------------------------ launchers

hipError_t launch_pf_sigma(const PfSigArgs& a, hipStream_t s) {
  if (a.s1 <= a.s0 || a.Ka <= 0 || a.d <= 0) return hipSuccess;
  const int threads = a.d >= kPfThreads ? kPfThreads : (a.d + 63) & ~63;
  hipLaunchKernelGGL(k_pf_sigma, dim3((unsigned)((a.s1 - a.s0) * a.Ka)), dim3(threads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pf_welford(const PfWelArgs& a, hipStream_t s) {
  if (a.s1 <= a.s0 || a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pf_welford, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// The lanes of a wave that work: as many level rows (ld slots of 8 bytes for each of the counts
// and the laws asked for) as kPfLdsBytes hold, at most 64; 16 at ld = 255 with both.
hipError_t launch_pf_levels(const PfLevArgs& a, hipStream_t s) {
  if (a.jb <= 0 || a.Ka <= 0 || a.M <= 0 || (!a.cnt && !a.law)) return hipSuccess;
  if (a.ld < 1 || a.ld > 255) return hipErrorInvalidValue;
  const int row = a.ld * 8 * ((a.cnt ? 1 : 0) + (a.law ? 1 : 0));
  PfLevArgs b = a;
  b.lanes = std::min(64, kPfLdsBytes / row);
  hipLaunchKernelGGL(k_pf_levels, dim3((unsigned)((a.jb + b.lanes - 1) / b.lanes), (unsigned)a.Ka), dim3(64),
                     (size_t)b.lanes * row, s, b);
  return hipGetLastError();
}

}  // namespace hdpm
