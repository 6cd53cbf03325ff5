// predict_host.hpp -- the host arithmetic of the posterior predictive (hdpm_predict_*), each
// rule once: the checks of the model and of the recorded parameters, the parameter tables the
// kernels of predict.hip read, the new-cluster weight, the rows per block and the packing of a
// block of rows, and for rows with missing attributes the code check, the per-row ll_0, the
// entries, the ld check and imputation's cuts of the rows and of the draws.
//
// Plain C++, no HIP: summary_host.cpp includes it, and tests/cpp/predict_host_test.cpp and
// tests/cpp/impute_host_test.cpp check it on the host.  A check returns an empty string, or
// the message of the HDPM_E_ARG refusal.
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

// ---- rows with missing attributes (hdpm_predict_partial, hdpm_predict_impute): code 0 in a
// row says that the attribute was not observed

// the first code above m_j among rows x d codes (0 is allowed): its index, or -1
inline int64_t pr_bad_code_partial(const uint8_t* codes, int64_t rows, int d, const int32_t* att) {
  for (int64_t i = 0; i < rows; ++i)
    for (int j = 0; j < d; ++j)
      if (codes[i * d + j] > att[j]) return i * d + j;
  return -1;
}
inline std::string pr_code_message_partial(int64_t at, int d) {
  return "predict: codes must lie in 0..attrisize[j], 0 for a missing attribute (row " + std::to_string(at / d) +
         ", attribute " + std::to_string(at % d) + ")";
}

// ll_0 of one row: -sum log(m_j) over its observed attributes, left to right; a complete row
// gives the bits of pr_ll0
inline double pr_ll0_row(const uint8_t* y, int d, const int32_t* att) {
  double s = 0.0;
  for (int j = 0; j < d; ++j)
    if (y[j] != 0) s = s + std::log((double)att[j]);
  return -s;
}

// the missing entries (codes 0) of rows x d codes
inline int64_t pr_count_missing(const uint8_t* codes, int64_t rows, int d) {
  int64_t n = 0;
  for (int64_t q = 0; q < rows * d; ++q) n += codes[q] == 0;
  return n;
}

// Entries are numbered in row-major order.  off[b] = the entries of the rows before block b
// (nb rows each), b = 0 .. blocks, so off[blocks] is their count; returns blocks
inline size_t pr_missing_offsets(const uint8_t* codes, int64_t ny, int d, size_t nb, int64_t* off) {
  size_t b = 0;
  int64_t n = 0;
  for (int64_t i0 = 0; i0 < ny; i0 += (int64_t)nb, ++b) {
    off[b] = n;
    n += pr_count_missing(codes + (size_t)i0 * d, std::min<int64_t>((int64_t)nb, ny - i0), d);
  }
  off[b] = n;
  return b;
}

// the entries of rows r0 .. r1 - 1 in order, two words each: the row within the block
// (r - r0) and the attribute
inline void pr_missing_entries(const uint8_t* codes, int64_t r0, int64_t r1, int d, uint32_t* ent) {
  for (int64_t r = r0; r < r1; ++r)
    for (int j = 0; j < d; ++j)
      if (codes[r * d + j] == 0) {
        *ent++ = (uint32_t)(r - r0);
        *ent++ = (uint32_t)j;
      }
}

// Imputation cuts the rows into blocks of whole quanta and, within a block, the draws into
// chunks, so that a block's rows (row_bytes each, one draw's record included), its entries
// (entry_bytes each) and a chunk's records obey the budget.  qoff: pr_missing_offsets at
// kPrRowQuantum rows per block.  The quanta of the block that starts at quantum q0: as many
// as fit (and at most max_entries entries), at least one.
inline size_t pr_impute_quanta(const int64_t* qoff, size_t nq, size_t q0, size_t budget, size_t row_bytes,
                               size_t entry_bytes, int64_t max_entries) {
  size_t n = 1;
  while (q0 + n < nq) {
    const int64_t ent = qoff[q0 + n + 1] - qoff[q0];
    const long double need = (long double)(n + 1) * kPrRowQuantum * row_bytes + (long double)ent * entry_bytes;
    if (need > (long double)budget || ent > max_entries) break;
    ++n;
  }
  return n;
}
// The doubles per row that a block of `rows` rows (whole quanta) with `entries` entries has for
// the records of a chunk of draws: what the budget leaves after the rows' other staging
// (row_bytes less the one record of rec1 doubles that it counts) and the entries', spread
// over the block's own rows; at least rec1 (one draw always goes through), at most `whole`
// (all the draws).  The record buffer of the block is rows x this.
inline int64_t pr_impute_rstride(size_t budget, size_t rows, size_t row_bytes, int64_t entries, size_t entry_bytes,
                                 size_t rec1, int64_t whole) {
  const long double fixed = (long double)rows * (row_bytes - rec1 * 8) + (long double)entries * entry_bytes;
  const long double left = (long double)budget > fixed ? (long double)budget - fixed : 0.0L;
  const int64_t fit = (int64_t)std::min<long double>(left / ((long double)rows * 8), (long double)whole);
  return std::min<int64_t>(whole, std::max<int64_t>((int64_t)rec1, fit));
}
// the end s1 of the chunk of draws that starts at s0: the most draws whose records, off[s1] -
// off[s0] + 2 (s1 - s0) doubles per row, stay within cap; at least one draw
inline int pr_draw_chunk(const int64_t* off, int M, int s0, int64_t cap) {
  int s1 = s0 + 1;
  while (s1 < M && off[s1 + 1] - off[s0] + 2 * (int64_t)(s1 + 1 - s0) <= cap) ++s1;
  return s1;
}

// ld, the slots of a pmf row: at most 255 and at least the m_j of every missing attribute
inline std::string pr_check_ld(const uint8_t* codes, int64_t rows, int d, const int32_t* att, int ld) {
  if (ld < 0 || ld > 255) return "predict: ld must be in 0..255";
  for (int64_t i = 0; i < rows; ++i)
    for (int j = 0; j < d; ++j)
      if (codes[i * d + j] == 0 && att[j] > ld)
        return "predict: ld is " + std::to_string(ld) + ", below attrisize " + std::to_string(att[j]) +
               " of a missing attribute (row " + std::to_string(i) + ", attribute " + std::to_string(j) + ")";
  return "";
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
