// predict_host.hpp -- the host arithmetic of the posterior predictive (hdpm_predict_*), each
// rule once: the checks of the model and of the recorded parameters, the parameter tables the
// kernels of predict.hip read, the new-cluster weight, the rows per block and the packing of a
// block of rows.
//
// Plain C++, no HIP: summary_host.cpp includes it, and tests/cpp/predict_host_test.cpp checks
// it on the host.  A check returns an empty string, or the message of the HDPM_E_ARG refusal.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "rmath.hpp"

namespace hdpm {

constexpr size_t kPrRowQuantum = 64;   // rows of a block: a multiple, and at least one

// d and attrisize as hdpm_set_data accepts them, gamma > 0
inline std::string pr_check_model(int d, const int32_t* att, double gamma) {
  if (d <= 0 || !att) return "predict: d must be positive";
  for (int j = 0; j < d; ++j)
    if (att[j] < 1 || att[j] > 255)
      return "predict: attrisize must be in 1..255 (attribute " + std::to_string(j) + ")";
  if (!(gamma > 0.0) || !std::isfinite(gamma)) return "predict: gamma must be finite and > 0";
  return "";
}

// Draw s of the trace has labels exactly 0..K-1 (sizes: its 256 cluster sizes) and the caller
// gives K parameter rows for it
inline std::string pr_check_draw(int s, int32_t total_cls, const uint32_t* sizes) {
  int used = 0, top = -1;
  for (int b = 0; b < 256; ++b)
    if (sizes[b] != 0u) {
      ++used;
      top = b;
    }
  if (total_cls != used)
    return "predict: draw " + std::to_string(s) + ": total_cls is " + std::to_string(total_cls) +
           " but the trace has " + std::to_string(used) + " clusters";
  if (top != used - 1)
    return "predict: draw " + std::to_string(s) + ": the trace's labels must be exactly 0.." +
           std::to_string(used - 1) + " (label k names parameter row k)";
  return "";
}

// the K x d centers (integers in 1..m_j) and sigmas (finite, > 0) of draw s
inline std::string pr_check_params(int s, int K, int d, const int32_t* att, const double* cen, const double* sig) {
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < d; ++j) {
      const double c = cen[(size_t)k * d + j], g = sig[(size_t)k * d + j];
      const std::string at = "draw " + std::to_string(s) + ", cluster " + std::to_string(k) + ", attribute " +
                             std::to_string(j);
      if (!(c >= 1.0 && c <= (double)att[j]) || c != std::floor(c))
        return "predict: a center must be an integer in 1..attrisize (" + at + ")";
      if (!(g > 0.0) || !std::isfinite(g)) return "predict: a sigma must be finite and > 0 (" + at + ")";
    }
  return "";
}

// The tables of `rows` parameter rows: the center as a byte (rows x d4, d4 = d rounded up to
// a multiple of 4, the padding 0) and dhamming's (match, mismatch) pair per (row, attribute)
inline int pr_d4(int d) { return (d + 3) & ~3; }
inline void pr_build_tables(int64_t rows, int d, const int32_t* att, const double* cen, const double* sig,
                            uint8_t* cen_b, double* mm) {
  const int d4 = pr_d4(d);
  for (int64_t r = 0; r < rows; ++r) {
    for (int j = 0; j < d4; ++j) cen_b[r * d4 + j] = j < d ? (uint8_t)cen[r * d + j] : (uint8_t)0;
    for (int j = 0; j < d; ++j) dhamming_pair(sig[r * d + j], att[j], &mm[2 * (r * d + j)], &mm[2 * (r * d + j) + 1]);
  }
}

// ll_0 = -sum_j log(m_j), summed left to right: the log prior predictive of any row (the prior
// center is uniform and exp(match) + (m - 1) exp(mismatch) = 1 for every sigma)
inline double pr_ll0(int d, const int32_t* att) {
  double s = 0.0;
  for (int j = 0; j < d; ++j) s = s + std::log((double)att[j]);
  return -s;
}

// rows per block: budget / bytes_per_row in whole quanta, at least one quantum, at most the
// rows there are (rounded up to a quantum)
inline size_t pr_block(size_t budget, size_t bytes_per_row, size_t ny) {
  const size_t q = kPrRowQuantum;
  size_t nb = budget / std::max<size_t>(bytes_per_row, 1) / q * q;
  nb = std::max(nb, q);
  return std::min(nb, (ny + q - 1) / q * q);
}

// the first code outside 1..m_j among rows x d codes: its index, or -1
inline int64_t pr_bad_code(const uint8_t* codes, int64_t rows, int d, const int32_t* att) {
  for (int64_t i = 0; i < rows; ++i)
    for (int j = 0; j < d; ++j) {
      const uint8_t x = codes[i * d + j];
      if (x < 1 || x > att[j]) return i * d + j;
    }
  return -1;
}
inline std::string pr_code_message(int64_t at, int d) {
  return "predict: codes must lie in 1..attrisize[j] (row " + std::to_string(at / d) + ", attribute " +
         std::to_string(at % d) + ")";
}

// Rows r0 .. r1 - 1 of a block (row-major, d codes each) as words of four codes, word w of row
// r at cw[w * nbp + r]: consecutive lanes read consecutive words.  Padding codes are 0.
inline void pr_pack_rows(const uint8_t* codes, int64_t r0, int64_t r1, int d, size_t nbp, uint32_t* cw) {
  const int nw = pr_d4(d) / 4;
  for (int64_t r = r0; r < r1; ++r)
    for (int w = 0; w < nw; ++w) {
      uint32_t v = 0;
      for (int b = 0; b < 4 && 4 * w + b < d; ++b) v |= (uint32_t)codes[r * d + 4 * w + b] << (8 * b);
      cw[(size_t)w * nbp + r] = v;
    }
}

// partition labels 0..Ka-1, 1 <= Ka <= 255
inline std::string pr_check_classes(const int32_t* cl, int64_t N, int Ka) {
  if (Ka < 1 || Ka > 255) return "predict: Ka must be in 1..255";
  for (int64_t i = 0; i < N; ++i)
    if (cl[i] < 0 || cl[i] >= Ka)
      return "predict: the partition's labels must be in 0..Ka-1 (point " + std::to_string(i) + ")";
  return "";
}

}  // namespace hdpm
