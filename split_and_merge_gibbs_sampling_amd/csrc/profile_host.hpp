// profile_host.hpp -- the host arithmetic of the cluster profiles (hdpm_predict_profile,
// include/hdpm.h): the check of ld (the partition's is predict_host.hpp's), the cuts of the attributes into blocks and of the draws
// into chunks that keep the device staging within the table budget, and a scalar fold of the
// same definitions that profile.hip's kernels evaluate.
//
// Plain C++, no HIP: summary_host.cpp includes it and tests/cpp/profile_host_test.cpp checks it
// on the host.  A check returns an empty string, or the message of the HDPM_E_ARG refusal.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace hdpm {

// ld, the slots of a level row: at most 255 and at least every m_j (the first attribute above it
// is named)
inline std::string pf_check_ld(int d, const int32_t* att, int ld) {
  if (ld < 1 || ld > 255) return "profile: ld must be in 1..255";
  for (int j = 0; j < d; ++j)
    if (att[j] > ld)
      return "profile: ld is " + std::to_string(ld) + ", below attrisize " + std::to_string(att[j]) + " of attribute " +
             std::to_string(j);
  return "";
}

// n items cut into pieces of budget / bytes_per_item items, at least one item per piece, in
// order: piece p is items cut[p] .. cut[p + 1] - 1, every item in exactly one piece
inline size_t pf_piece(size_t budget, long double bytes_per_item, size_t n) {
  const long double fit = (long double)budget / std::max<long double>(bytes_per_item, 1.0L);
  const size_t per = fit >= (long double)n ? n : (size_t)fit;
  return std::min(std::max<size_t>(per, 1), std::max<size_t>(n, 1));
}
inline std::vector<int> pf_cuts(size_t budget, long double bytes_per_item, int n) {
  std::vector<int> cut;
  const int per = (int)pf_piece(budget, bytes_per_item, (size_t)std::max(n, 0));
  for (int i = 0; i < n; i += per) cut.push_back(i);
  cut.push_back(std::max(n, 0));
  return cut;
}
// the attributes of a block: its level rows, Ka x ld slots of slot_bytes each per attribute (8
// for the counts, 8 for the code law: what the call asked for)
inline std::vector<int> pf_attr_blocks(size_t budget, int Ka, int ld, int slot_bytes, int d) {
  return pf_cuts(budget, (long double)Ka * ld * slot_bytes, d);
}
// the draws of a chunk: Ka x d doubles of u_s per draw
inline std::vector<int> pf_draw_chunks(size_t budget, int Ka, int d, int M) {
  return pf_cuts(budget, (long double)Ka * d * 8, M);
}

// What the fold reads.  Parameter row off[s] + k is cluster k of draw s: cen its centers as
// bytes (rows of cstride), sig its sigmas and emm its (exp(match), exp(mismatch)) pairs (rows of
// d).  tab is T^s[a][k] at tab[(s * Ka + a) * Kz + k], na the class sizes.
struct PfIn {
  int M, Ka, Kz, d, ld;
  const int32_t* att;
  const int64_t* off;
  const uint32_t* tab;
  const uint64_t* na;
  const uint8_t* cen;
  int cstride;
  const double* sig;
  const double* emm;
};

// The definitions of include/hdpm.h, one (class, attribute) at a time, the sums over s in draw
// order and then over k in cluster order.  Any output may be null.
inline void pf_fold(const PfIn& p, uint64_t* center_cnt, double* code_pmf, double* sigma_mean, double* sigma_var,
                    double* sigma_trace) {
  const int M = p.M, Ka = p.Ka, d = p.d, ld = p.ld;
  std::vector<uint64_t> cnt((size_t)ld);
  std::vector<double> law((size_t)ld);
  for (int a = 0; a < Ka; ++a)
    for (int j = 0; j < d; ++j) {
      const size_t aj = (size_t)a * d + j;
      const double na = (double)p.na[a];
      const int m = p.att[j];
      std::fill(cnt.begin(), cnt.end(), 0);
      std::fill(law.begin(), law.end(), 0.0);
      double mean = 0.0, m2 = 0.0;
      for (int s = 0; s < M; ++s) {
        const int64_t base = p.off[s];
        const int K = (int)(p.off[s + 1] - base);
        const uint32_t* T = p.tab + ((size_t)s * Ka + a) * p.Kz;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) {
          const double t = (double)T[k];
          const size_t q = (size_t)(base + k) * d + j;
          const int c = p.cen[(size_t)(base + k) * p.cstride + j];
          cnt[c - 1] += T[k];
          acc = acc + t * p.sig[q];
          if (code_pmf)
            for (int l = 1; l <= m; ++l) law[l - 1] = law[l - 1] + t * (l == c ? p.emm[2 * q] : p.emm[2 * q + 1]);
        }
        const double u = p.na[a] ? acc / na : 0.0;
        if (sigma_trace) sigma_trace[((size_t)s * Ka + a) * d + j] = u;
        const double delta = u - mean;
        mean = mean + delta / (double)(s + 1);
        m2 = m2 + delta * (u - mean);
      }
      if (sigma_mean) sigma_mean[aj] = mean;
      if (sigma_var) sigma_var[aj] = M > 1 ? m2 / ((double)M - 1.0) : 0.0;
      for (int l = 0; l < ld; ++l) {
        if (center_cnt) center_cnt[aj * ld + l] = cnt[l];
        if (code_pmf) code_pmf[aj * ld + l] = (p.na[a] && l < m) ? law[l] / ((double)M * na) : 0.0;
      }
    }
}

}  // namespace hdpm
