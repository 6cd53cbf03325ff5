// predict.hip -- the posterior predictive of rows against the recorded draws, and the pointwise
// log-likelihood of the training rows (hdpm_predict_*, include/hdpm.h).
//
// Draw s has K_s clusters with centers c_kj and dhamming's (match, mismatch) pair per (k, j),
// kept as tables built once (predict_host.hpp): a byte and two doubles per (s, k, j).
//
//   ll_k(y) = sum_j (y_j == c_kj ? match_kj : mismatch_kj), added in attribute order: the bits
//             of k_lmatrix on that state
//   w_k     = log n_k + ll_k (k = 1..K_s), w_0 = log gamma + ll_0;  lse = log sum_k exp(w_k);
//             r_k = exp(w_k - lse)
//
//   k_pr_new   a workgroup keeps a tile of rows (kPrThreads, fewer when the rows are few), one
//              per lane, and walks the draws.
//              Per draw it stages the tables of kPrG clusters x kPrDC attributes in LDS and
//              every lane adds into kPrG accumulators (independent FP64 add chains); all lanes
//              read the same table entry, an LDS broadcast.  Wide rows walk attribute chunks
//              with the accumulators kept, so the attribute order is unchanged.  A lane's row
//              comes as words of four codes, word-major, so a wave's read is contiguous; the
//              words are re-read per draw and cluster group from L1 / L2.  The w_k of a row go
//              to a scratch column of the lane; then the maximum, the exps in cluster order,
//              lse and r_k, and the fold sum_k r_k T^s[a][k] with the contingency tables of
//              k_tr_tables (zero counts skipped: they add +0.0).
//   k_pr_own   one lane per training row: its own cluster's ll in every draw, four draws in
//              flight (four add chains), the tables gathered from L2; the three running sums
//              per row in draw order.
//   k_pr_part  k_pr_new for rows with missing attributes (code 0: the attribute adds +0.0 to
//              every ll_k, and w_0 comes per row); a complete row gets k_pr_new's bytes.  For
//              k_pr_impute it leaves lse and the r_k of every (row, draw) of a chunk of draws,
//              the row's running sums carried from chunk to chunk.
//   k_pr_impute  the law of each missing code given its row's observed ones: a wave per missing
//              entry, a lane per level, the draws in order.
//
// A row's sums over draws run in draw order in one lane and its sums over clusters in cluster
// order, so no result depends on the grid, the tile or the block of rows.  Every exp and log
// is glibc's (glibc_math.hpp); sums of exps over draws keep a running maximum.
//
// Bound: k_pr_new issues per (row, draw, cluster, attribute) a compare, two selects and one
// FP64 add, and per (wave, cluster, attribute) one ds_read_b128 (4 LDS cycles), a quarter of
// a CU's LDS rate per SIMD at one wave each: the VALU and the LDS are loaded about equally.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "glibc_math.hpp"
#include "summary_launch.hpp"

namespace hdpm {

namespace prtab {
#define HDPM_GLIBC_TABLE static __constant__
#include "glibc_tables.inc"
#undef HDPM_GLIBC_TABLE
}  // namespace prtab

__device__ __forceinline__ double pr_exp(double x) { return glibc::exp_r(x, prtab::kGlibcExpTab); }
__device__ __forceinline__ double pr_log(double x) { return glibc::log_r(x, prtab::kGlibcLogTab); }

// log of a sum of exps whose terms arrive one by one: mx the largest so far, acc = sum exp(x - mx)
struct PrLse {
  double mx, acc;
  __device__ __forceinline__ void init(double x) {
    mx = x;
    acc = 1.0;
  }
  __device__ __forceinline__ void add(double x) {
    if (x > mx) {
      acc = acc * pr_exp(mx - x) + 1.0;
      mx = x;
    } else {
      acc = acc + pr_exp(x - mx);
    }
  }
  // log(sum / M)
  __device__ __forceinline__ double mean_log(double M) const { return mx + pr_log(acc / M); }
};

// kPrG clusters x nattr attributes of the staged tables into the lane's accumulators; xw is the
// lane's first word of the chunk, the next one `stride` words on.  MASK: a code 0 is a missing
// attribute and adds +0.0 whatever the tables say (k_pr_part)
template <int G, bool MASK = false>
__device__ __forceinline__ void pr_acc(const uint32_t* __restrict__ xw, int64_t stride, int nattr,
                                       const double2 (*s_mm)[kPrDC], const uint32_t (*s_cen)[kPrDC / 4],
                                       double (&acc)[kPrG]) {
  const int nfull = nattr >> 2;
  for (int w = 0; w < nfull; ++w) {
    const uint32_t x = xw[(int64_t)w * stride];
    uint32_t cw[G];
#pragma unroll
    for (int g = 0; g < G; ++g) cw[g] = s_cen[g][w];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t xb = (x >> (8 * b)) & 0xFFu;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const double2 v = s_mm[g][4 * w + b];
        const double t = xb == ((cw[g] >> (8 * b)) & 0xFFu) ? v.x : v.y;
        acc[g] = acc[g] + (MASK && xb == 0u ? 0.0 : t);
      }
    }
  }
  const int rest = nattr & 3;
  if (rest) {
    const uint32_t x = xw[(int64_t)nfull * stride];
    for (int b = 0; b < rest; ++b) {
      const uint32_t xb = (x >> (8 * b)) & 0xFFu;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const double2 v = s_mm[g][4 * nfull + b];
        const double t = xb == ((s_cen[g][nfull] >> (8 * b)) & 0xFFu) ? v.x : v.y;
        acc[g] = acc[g] + (MASK && xb == 0u ? 0.0 : t);
      }
    }
  }
}

__global__ __launch_bounds__(kPrThreads) void k_pr_new(PrNewArgs a) {
  __shared__ double2 s_mm[kPrG][kPrDC];
  __shared__ uint32_t s_cen[kPrG][kPrDC / 4];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t row = (int64_t)blockIdx.x * nt + tid;
  const bool valid = row < a.nrows;
  const int64_t lrow = valid ? row : a.nrows - 1;   // a lane past the end walks the last row and stores nothing
  const int d = a.d, nw = (d + 3) >> 2;
  const double2* mm = (const double2*)a.mm;
  const uint32_t* cenw = (const uint32_t*)a.cen;
  double* wcol = a.w + lrow;                        // w_k at wcol[k * nbp], k = 0 the new cluster
  PrLse lpd;
  double pn = 0.0;
  lpd.init(0.0);
  for (int s = a.s0; s < a.s1; ++s) {
    const int64_t base = a.off[s];
    const int K = (int)(a.off[s + 1] - base);
    for (int k0 = 0; k0 < K; k0 += kPrG) {
      const int G = min(kPrG, K - k0);
      double acc[kPrG];
#pragma unroll
      for (int g = 0; g < kPrG; ++g) acc[g] = 0.0;
      for (int j0 = 0; j0 < d; j0 += kPrDC) {
        const int nattr = min(kPrDC, d - j0), cw = (nattr + 3) >> 2;
        __syncthreads();                            // the previous chunk has been read
        for (int q = tid; q < G * nattr; q += nt) {
          const int g = q / nattr, jj = q - g * nattr;
          s_mm[g][jj] = mm[(base + k0 + g) * d + j0 + jj];
        }
        for (int q = tid; q < G * cw; q += nt) {
          const int g = q / cw, w = q - g * cw;
          s_cen[g][w] = cenw[(base + k0 + g) * nw + (j0 >> 2) + w];
        }
        __syncthreads();
        const uint32_t* xw = a.cw + (int64_t)(j0 >> 2) * a.nbp + lrow;
        switch (G) {
          case 1: pr_acc<1>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 2: pr_acc<2>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 3: pr_acc<3>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 4: pr_acc<4>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 5: pr_acc<5>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 6: pr_acc<6>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 7: pr_acc<7>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          default: pr_acc<8>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
        }
      }
      if (valid) {
#pragma unroll
        for (int g = 0; g < kPrG; ++g)
          if (g < G) {
            const int k = k0 + g;
            if (a.ll_out) a.ll_out[(int64_t)k * a.nbp + row] = acc[g];
            wcol[(int64_t)(k + 1) * a.nbp] = a.lognk[base + k] + acc[g];
          }
      }
    }
    if (!valid) continue;                           // no barrier below
    // the maximum, then the exps in cluster order
    double mx = a.w0;
    for (int k = 1; k <= K; ++k) mx = fmax(mx, wcol[(int64_t)k * a.nbp]);
    double sum = pr_exp(a.w0 - mx);
    for (int k = 1; k <= K; ++k) sum = sum + pr_exp(wcol[(int64_t)k * a.nbp] - mx);
    const double lse = mx + pr_log(sum);
    const double r0 = pr_exp(a.w0 - lse);
    pn = pn + r0;
    if (s == a.s0) lpd.init(lse);
    else lpd.add(lse);
    if (a.resp_out) a.resp_out[row] = r0;
    if (a.resp_out || a.tab) {
      for (int k = 1; k <= K; ++k) {
        const double r = pr_exp(wcol[(int64_t)k * a.nbp] - lse);
        if (a.resp_out) a.resp_out[(int64_t)k * a.nbp + row] = r;
        wcol[(int64_t)k * a.nbp] = r;
      }
    }
    if (a.tab) {
      const uint32_t* T = a.tab + (int64_t)s * a.Ka * a.Kz;
      for (int c = 0; c < a.Ka; ++c) {
        double t = 0.0;
        for (int k = 0; k < K; ++k) {
          const uint32_t n = T[c * a.Kz + k];
          if (n) t = t + wcol[(int64_t)(k + 1) * a.nbp] * (double)n;
        }
        double* cc = a.cc + (int64_t)c * a.nbp + row;
        *cc = s == a.s0 ? t : *cc + t;
      }
    }
  }
  if (!valid) return;
  const double nd = (double)(a.s1 - a.s0);
  if (a.lpd) a.lpd[row] = lpd.mean_log(nd) - a.log_ng;
  if (a.p_new) a.p_new[row] = pn / nd;
  if (a.tab)
    for (int c = 0; c < a.Ka; ++c) {
      double* cc = a.cc + (int64_t)c * a.nbp + row;
      *cc = a.na[c] > 0.0 ? *cc / (nd * a.na[c]) : 0.0;
    }
}

__global__ __launch_bounds__(kPrThreads) void k_pr_own(PrOwnArgs a) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.nrows) return;
  const int d = a.d, nw = (d + 3) >> 2, nfull = d >> 2, rest = d & 3;
  const double2* mm = (const double2*)a.mm;
  const uint32_t* cenw = (const uint32_t*)a.cen;
  const uint8_t* z = a.lab + a.row0 + row;
  const uint32_t* xw = a.cw + row;
  PrLse up, down;
  double mean = 0.0, m2 = 0.0;
  up.init(0.0);
  down.init(0.0);
  for (int s0 = 0; s0 < a.M; s0 += kPrOwnDraws) {
    const int U = min(kPrOwnDraws, a.M - s0);
    int64_t r[kPrOwnDraws];
    double acc[kPrOwnDraws];
#pragma unroll
    for (int u = 0; u < kPrOwnDraws; ++u) {
      const int s = s0 + min(u, U - 1);             // past the last draw: the last one again, unused
      r[u] = a.off[s] + (int64_t)z[(int64_t)s * a.Np];
      acc[u] = 0.0;
    }
    for (int w = 0; w < nfull; ++w) {
      const uint32_t x = xw[(int64_t)w * a.nbp];
      uint32_t cw[kPrOwnDraws];
#pragma unroll
      for (int u = 0; u < kPrOwnDraws; ++u) cw[u] = cenw[r[u] * nw + w];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t xb = (x >> (8 * b)) & 0xFFu;
#pragma unroll
        for (int u = 0; u < kPrOwnDraws; ++u) {
          const double2 v = mm[r[u] * d + 4 * w + b];
          acc[u] = acc[u] + (xb == ((cw[u] >> (8 * b)) & 0xFFu) ? v.x : v.y);
        }
      }
    }
    if (rest) {
      const uint32_t x = xw[(int64_t)nfull * a.nbp];
      for (int b = 0; b < rest; ++b) {
        const uint32_t xb = (x >> (8 * b)) & 0xFFu;
#pragma unroll
        for (int u = 0; u < kPrOwnDraws; ++u) {
          const double2 v = mm[r[u] * d + 4 * nfull + b];
          acc[u] = acc[u] + (xb == ((cenw[r[u] * nw + nfull] >> (8 * b)) & 0xFFu) ? v.x : v.y);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kPrOwnDraws; ++u)
      if (u < U) {
        const double l = acc[u];
        const int s = s0 + u;
        if (s == 0) {
          up.init(l);
          down.init(-l);
        } else {
          up.add(l);
          down.add(-l);
        }
        // Welford's update: the mean and the sum of squared deviations of l_0 .. l_s
        const double delta = l - mean;
        mean = mean + delta / (double)(s + 1);
        m2 = m2 + delta * (l - mean);
      }
  }
  const double M = (double)a.M;
  if (a.lppd) a.lppd[row] = up.mean_log(M);
  if (a.logcpo) a.logcpo[row] = -down.mean_log(M);
  if (a.var) a.var[row] = a.M > 1 ? m2 / (M - 1.0) : 0.0;
}

// ---- rows with missing attributes (code 0)

// k_pr_new's walk with the third select of pr_acc<G, true>, the row's own w_0, and for
// k_pr_impute the lse and r_k of every (draw, row) left in global scratch.  A complete row
// meets the same operations in the same order as in k_pr_new.
__global__ __launch_bounds__(kPrThreads) void k_pr_part(PrPartArgs p) {
  __shared__ double2 s_mm[kPrG][kPrDC];
  __shared__ uint32_t s_cen[kPrG][kPrDC / 4];
  const PrNewArgs& a = p.n;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t row = (int64_t)blockIdx.x * nt + tid;
  const bool valid = row < a.nrows;
  const int64_t lrow = valid ? row : a.nrows - 1;
  const int d = a.d, nw = (d + 3) >> 2;
  const double2* mm = (const double2*)a.mm;
  const uint32_t* cenw = (const uint32_t*)a.cen;
  double* wcol = a.w + lrow;
  const double w0 = p.w0[lrow];
  const bool keep = p.r != nullptr;
  PrLse lpd;
  double pn = 0.0;
  lpd.init(0.0);
  if (!p.first && valid) {                          // the row's sums over the draws before s0
    lpd.mx = p.carry[row];
    lpd.acc = p.carry[a.nbp + row];
    pn = p.carry[2 * a.nbp + row];
  }
  for (int s = a.s0; s < a.s1; ++s) {
    const int64_t base = a.off[s];
    const int K = (int)(a.off[s + 1] - base);
    for (int k0 = 0; k0 < K; k0 += kPrG) {
      const int G = min(kPrG, K - k0);
      double acc[kPrG];
#pragma unroll
      for (int g = 0; g < kPrG; ++g) acc[g] = 0.0;
      for (int j0 = 0; j0 < d; j0 += kPrDC) {
        const int nattr = min(kPrDC, d - j0), cw = (nattr + 3) >> 2;
        __syncthreads();
        for (int q = tid; q < G * nattr; q += nt) {
          const int g = q / nattr, jj = q - g * nattr;
          s_mm[g][jj] = mm[(base + k0 + g) * d + j0 + jj];
        }
        for (int q = tid; q < G * cw; q += nt) {
          const int g = q / cw, w = q - g * cw;
          s_cen[g][w] = cenw[(base + k0 + g) * nw + (j0 >> 2) + w];
        }
        __syncthreads();
        const uint32_t* xw = a.cw + (int64_t)(j0 >> 2) * a.nbp + lrow;
        switch (G) {
          case 1: pr_acc<1, true>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 2: pr_acc<2, true>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 3: pr_acc<3, true>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 4: pr_acc<4, true>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 5: pr_acc<5, true>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 6: pr_acc<6, true>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          case 7: pr_acc<7, true>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
          default: pr_acc<8, true>(xw, a.nbp, nattr, s_mm, s_cen, acc); break;
        }
      }
      if (valid) {
#pragma unroll
        for (int g = 0; g < kPrG; ++g)
          if (g < G) wcol[(int64_t)(k0 + g + 1) * a.nbp] = a.lognk[base + k0 + g] + acc[g];
      }
    }
    if (!valid) continue;                           // no barrier below
    double mx = w0;
    for (int k = 1; k <= K; ++k) mx = fmax(mx, wcol[(int64_t)k * a.nbp]);
    double sum = pr_exp(w0 - mx);
    for (int k = 1; k <= K; ++k) sum = sum + pr_exp(wcol[(int64_t)k * a.nbp] - mx);
    const double lse = mx + pr_log(sum);
    const double r0 = pr_exp(w0 - lse);
    pn = pn + r0;
    if (p.first && s == a.s0) lpd.init(lse);
    else lpd.add(lse);
    double* rec = nullptr;                          // the row's record of this draw: lse, r_0, r_1 .. r_K
    if (keep) {
      rec = p.r + row * p.rstride + (base - a.off[a.s0]) + 2 * (s - a.s0);
      rec[0] = lse;
      rec[1] = r0;
    }
    if (keep || a.tab) {
      for (int k = 1; k <= K; ++k) {
        const double r = pr_exp(wcol[(int64_t)k * a.nbp] - lse);
        if (keep) rec[1 + k] = r;
        wcol[(int64_t)k * a.nbp] = r;
      }
    }
    if (a.tab) {
      const uint32_t* T = a.tab + (int64_t)s * a.Ka * a.Kz;
      for (int c = 0; c < a.Ka; ++c) {
        double t = 0.0;
        for (int k = 0; k < K; ++k) {
          const uint32_t n = T[c * a.Kz + k];
          if (n) t = t + wcol[(int64_t)(k + 1) * a.nbp] * (double)n;
        }
        double* cc = a.cc + (int64_t)c * a.nbp + row;
        *cc = (p.first && s == a.s0) ? t : *cc + t;
      }
    }
  }
  if (!valid) return;
  if (!p.last) {
    p.carry[row] = lpd.mx;
    p.carry[a.nbp + row] = lpd.acc;
    p.carry[2 * a.nbp + row] = pn;
    return;
  }
  const double nd = (double)p.M;
  if (a.lpd) a.lpd[row] = lpd.mean_log(nd) - a.log_ng;
  if (a.p_new) a.p_new[row] = pn / nd;
  if (a.tab)
    for (int c = 0; c < a.Ka; ++c) {
      double* cc = a.cc + (int64_t)c * a.nbp + row;
      *cc = a.na[c] > 0.0 ? *cc / (nd * a.na[c]) : 0.0;
    }
}

// out[i] = exp(x[i]): the (exp(match), exp(mismatch)) pairs of k_pr_impute
__global__ __launch_bounds__(256) void k_pr_exp(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = pr_exp(x[i]);
}

// lane t's value in every lane (t the same in all of them)
__device__ __forceinline__ double pr_bcast(double x, int t) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), t),
                          __builtin_amdgcn_readlane(__double2loint(x), t));
}

// The law of one missing code given the row's observed ones.  A wave per entry (row, j); lane t
// holds the levels t + 1, t + 65, .. (P of them; a pass past m_j is skipped).  The wave walks
// the draws in order: q_l = r_0 / m_j, then + r_k * (l == c_kj ? exp(match) : exp(mismatch))
// in cluster order; A_l and the row's PrLse (mx, acc) stay in registers over a chunk of draws
// (between chunks in the entry's pmf row and in st, double for double).  Per draw, lane t
// fetches cluster t's r_k (contiguous in the row's record), center byte and pair, 64 clusters
// at a time, and the cluster loop hands them round by readlane: one memory latency per draw,
// not one per cluster.
template <int P>
__global__ __launch_bounds__(64 * kPrImpWaves) void k_pr_impute(PrImpArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kPrImpWaves + (threadIdx.x >> 6)));
  if (e >= a.nent) return;
  const int64_t row = a.ent[2 * (int64_t)e];
  const int j = (int)a.ent[2 * (int64_t)e + 1];
  const int m = a.att[j];
  const int d = a.d, d4 = (d + 3) & ~3;
  const double dm = (double)m;
  const double2* __restrict__ emm = (const double2*)a.emm;
  const uint8_t* __restrict__ cen = a.cen;
  const double* __restrict__ rec = a.r + row * a.rstride;
  double* out = a.pmf + (int64_t)e * a.ld;
  double A[P];
#pragma unroll
  for (int p = 0; p < P; ++p) A[p] = 0.0;
  double mx = 0.0, acc = 1.0;
  if (!a.first) {                                   // the sums over the draws before s0
    mx = a.st[e];
    acc = a.st[(int64_t)a.nent + e];
#pragma unroll
    for (int p = 0; p < P; ++p)
      if (lane + 64 * p < a.ld) A[p] = out[lane + 64 * p];
  }
  const int64_t base0 = a.off[a.s0];
  for (int s = a.s0; s < a.s1; ++s) {
    const int64_t base = a.off[s];
    const int K = (int)(a.off[s + 1] - base);
    const double* rs = rec + (base - base0) + 2 * (s - a.s0);
    const double lse = rs[0];
    const double q0 = rs[1] / dm;
    double q[P];
#pragma unroll
    for (int p = 0; p < P; ++p) q[p] = q0;
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int n = min(64, K - k0);
      const int kk = k0 + min(lane, n - 1);         // a lane past the last cluster: the last one again, unused
      const double rv = rs[2 + kk];
      const int cv = cen[(base + kk) * d4 + j];
      const double2 vv = emm[(base + kk) * d + j];
      for (int t = 0; t < n; ++t) {
        const double rk = pr_bcast(rv, t), ma = pr_bcast(vv.x, t), mi = pr_bcast(vv.y, t);
        const int c = __builtin_amdgcn_readlane(cv, t);
#pragma unroll
        for (int p = 0; p < P; ++p)
          if (64 * p < m) q[p] = q[p] + rk * (lane + 64 * p + 1 == c ? ma : mi);
      }
    }
    if (a.first && s == a.s0) {
      mx = lse;
#pragma unroll
      for (int p = 0; p < P; ++p) A[p] = q[p];
    } else if (lse > mx) {
      const double f = pr_exp(mx - lse);
      acc = acc * f + 1.0;
      mx = lse;
#pragma unroll
      for (int p = 0; p < P; ++p) A[p] = A[p] * f + q[p];
    } else {
      const double f = pr_exp(lse - mx);
      acc = acc + f;
#pragma unroll
      for (int p = 0; p < P; ++p) A[p] = A[p] + q[p] * f;
    }
  }
  if (!a.last) {
    if (lane == 0) {
      a.st[e] = mx;
      a.st[(int64_t)a.nent + e] = acc;
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
      if (lane + 64 * p < a.ld) out[lane + 64 * p] = A[p];
    return;
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int slot = lane + 64 * p;
    if (slot < a.ld) out[slot] = slot < m ? A[p] / acc : 0.0;
  }
}

// ------------------------------------------------------------------------------ launchers

// The rows of a tile: kPrThreads where that still gives every CU a workgroup, else half or a
// quarter of it (a wave), so that few rows spread over more CUs.  No result depends on it.
static int pr_tile(int64_t nrows) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus <= 0)
    cus = 256;
  int tile = kPrThreads;
  while (tile > 64 && (nrows + tile - 1) / tile < cus) tile >>= 1;
  return tile;
}

hipError_t launch_pr_new(const PrNewArgs& a, hipStream_t s) {
  if (a.nrows <= 0 || a.s1 <= a.s0) return hipSuccess;
  const int tile = pr_tile(a.nrows);
  hipLaunchKernelGGL(k_pr_new, dim3((unsigned)((a.nrows + tile - 1) / tile)), dim3(tile), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pr_part(const PrPartArgs& a, hipStream_t s) {
  if (a.n.nrows <= 0 || a.n.s1 <= a.n.s0) return hipSuccess;
  const int tile = pr_tile(a.n.nrows);
  hipLaunchKernelGGL(k_pr_part, dim3((unsigned)((a.n.nrows + tile - 1) / tile)), dim3(tile), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pr_exp(const double* x, int64_t n, double* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pr_exp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, out);
  return hipGetLastError();
}

hipError_t launch_pr_impute(const PrImpArgs& a, hipStream_t s) {
  if (a.nent <= 0 || a.s1 <= a.s0) return hipSuccess;
  if (a.ld < 1 || a.ld > 255) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.nent + kPrImpWaves - 1) / kPrImpWaves)), block(64 * kPrImpWaves);
  switch ((a.ld + 63) / 64) {
    case 1: hipLaunchKernelGGL(k_pr_impute<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_pr_impute<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(k_pr_impute<3>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(k_pr_impute<4>, grid, block, 0, s, a); break;
  }
  return hipGetLastError();
}

hipError_t launch_pr_own(const PrOwnArgs& a, hipStream_t s) {
  if (a.nrows <= 0 || a.M <= 0) return hipSuccess;
  const int tile = pr_tile(a.nrows);
  hipLaunchKernelGGL(k_pr_own, dim3((unsigned)((a.nrows + tile - 1) / tile)), dim3(tile), 0, s, a);
  return hipGetLastError();
}

}  // namespace hdpm
