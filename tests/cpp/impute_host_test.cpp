// csrc/predict_host.hpp, the helpers of rows with missing attributes (code 0): the code check,
// the per-row ll_0 (a complete row has pr_ll0's bits), the count of missing entries, their
// offsets per block of rows and their order, the ld check, and imputation's cuts: the quanta
// of a block, the share of the budget its records get, the chunks of draws; doubles compared
// by bytes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../split_and_merge_gibbs_sampling_amd/csrc/predict_host.hpp"

static int fails = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #x);           \
      ++fails;                                                     \
    }                                                              \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

int main() {
  using namespace hdpm;
  // ---- the code check: 0 passes, a code above m_j does not; the complete-row check still refuses 0
  {
    const int d = 3;
    const int32_t att[d] = {2, 3, 4};
    std::vector<uint8_t> y = {1, 0, 1, 0, 0, 0, 2, 3, 4};
    CHECK(pr_bad_code_partial(y.data(), 3, d, att) == -1);
    CHECK(pr_bad_code(y.data(), 3, d, att) == 1);
    y[5] = 5;
    CHECK(pr_bad_code_partial(y.data(), 3, d, att) == 5);
    CHECK(pr_bad_code_partial(y.data(), 1, d, att) == -1);
    CHECK(has(pr_code_message_partial(5, d), "row 1, attribute 2"));
    CHECK(has(pr_code_message_partial(5, d), "0..attrisize"));
    y[5] = 0; y[6] = 3;
    CHECK(pr_bad_code_partial(y.data(), 3, d, att) == 6);
  }
  // ---- ll_0 per row: a complete row has pr_ll0's bits; gaps drop their terms, left to right
  {
    const int d = 7;
    const int32_t att[d] = {2, 3, 6, 255, 17, 100, 5};
    std::vector<uint8_t> y = {1, 1, 1, 1, 1, 1, 1};
    CHECK(same_bits(pr_ll0_row(y.data(), d, att), pr_ll0(d, att)));
    for (int a = 1; a <= d; ++a) CHECK(same_bits(pr_ll0_row(y.data(), a, att), pr_ll0(a, att)));
    y[0] = 0; y[3] = 0; y[6] = 0;
    double s = 0.0;
    s = s + std::log(3.0);
    s = s + std::log(6.0);
    s = s + std::log(17.0);
    s = s + std::log(100.0);
    CHECK(same_bits(pr_ll0_row(y.data(), d, att), -s));
    std::vector<uint8_t> none(d, 0);
    CHECK(pr_ll0_row(none.data(), d, att) == 0.0);
    // log gamma + ll_0 of an all-missing row is log gamma itself
    CHECK(same_bits(std::log(0.68) + pr_ll0_row(none.data(), d, att), std::log(0.68)));
  }
  // ---- counts, offsets per block of rows and the entries' order
  {
    const int d = 5;
    const int64_t ny = 200;
    std::vector<uint8_t> y((size_t)ny * d, 1);
    // gaps on both sides of the 64-row edges, a row of all gaps, none in rows 128..190
    const int at[][2] = {{0, 0}, {0, 4}, {63, 2}, {64, 0}, {64, 1}, {65, 4}, {127, 3}, {191, 0}, {199, 4}};
    for (auto& a : at) y[(size_t)a[0] * d + a[1]] = 0;
    for (int j = 0; j < d; ++j) y[(size_t)100 * d + j] = 0;
    const int64_t total = 9 + 5;
    CHECK(pr_count_missing(y.data(), ny, d) == total);
    CHECK(pr_count_missing(y.data(), 64, d) == 3);
    CHECK(pr_count_missing(y.data() + 128 * d, 63, d) == 0);
    std::vector<int64_t> off(8, -1);
    CHECK(pr_missing_offsets(y.data(), ny, d, 64, off.data()) == 4);
    CHECK(off[0] == 0 && off[1] == 3 && off[2] == 12 && off[3] == 13 && off[4] == total && off[5] == -1);
    CHECK(pr_missing_offsets(y.data(), ny, d, 128, off.data()) == 2);
    CHECK(off[0] == 0 && off[1] == 12 && off[2] == total);
    CHECK(pr_missing_offsets(y.data(), ny, d, 256, off.data()) == 1);
    CHECK(off[0] == 0 && off[1] == total);
    // the entries of all rows at once, and block by block: the same list, rows rebased
    std::vector<uint32_t> all(2 * total, 0xDEADBEEFu), part(2 * total + 2, 0xDEADBEEFu);
    pr_missing_entries(y.data(), 0, ny, d, all.data());
    CHECK(all[0] == 0 && all[1] == 0 && all[2] == 0 && all[3] == 4 && all[4] == 63 && all[5] == 2);
    CHECK(all[6] == 64 && all[7] == 0 && all[8] == 64 && all[9] == 1 && all[10] == 65 && all[11] == 4);
    for (int j = 0; j < d; ++j) CHECK(all[2 * (6 + j)] == 100 && all[2 * (6 + j) + 1] == (uint32_t)j);
    CHECK(all[2 * 11] == 127 && all[2 * 11 + 1] == 3);
    CHECK(all[2 * 13] == 199 && all[2 * 13 + 1] == 4);
    pr_missing_offsets(y.data(), ny, d, 64, off.data());
    for (int b = 0; b < 4; ++b) {
      const int64_t r0 = 64 * b, r1 = std::min<int64_t>(ny, r0 + 64);
      pr_missing_entries(y.data(), r0, r1, d, part.data() + 2 * off[b]);
      for (int64_t e = off[b]; e < off[b + 1]; ++e) {
        CHECK(part[2 * e] + r0 == all[2 * e] && part[2 * e + 1] == all[2 * e + 1]);
        CHECK(y[(size_t)all[2 * e] * d + all[2 * e + 1]] == 0);
      }
    }
    CHECK(part[2 * total] == 0xDEADBEEFu);                   // nothing past the last entry
  }
  // ---- ld: at most 255, at least the m_j of every missing attribute (named); observed ones do not count
  {
    const int d = 3;
    const int32_t att[d] = {2, 255, 64};
    std::vector<uint8_t> y = {0, 7, 1, 1, 9, 0};
    CHECK(pr_check_ld(y.data(), 2, d, att, 64).empty());
    CHECK(pr_check_ld(y.data(), 2, d, att, 255).empty());
    CHECK(has(pr_check_ld(y.data(), 2, d, att, 256), "ld must be in 0..255"));
    CHECK(has(pr_check_ld(y.data(), 2, d, att, -1), "ld must be in 0..255"));
    const std::string m = pr_check_ld(y.data(), 2, d, att, 63);
    CHECK(has(m, "ld is 63") && has(m, "attrisize 64") && has(m, "row 1, attribute 2"));
    const std::string m1 = pr_check_ld(y.data(), 2, d, att, 1);
    CHECK(has(m1, "attrisize 2") && has(m1, "row 0, attribute 0"));
    CHECK(pr_check_ld(y.data(), 1, d, att, 2).empty());
    y[4] = 0;
    CHECK(has(pr_check_ld(y.data(), 2, d, att, 64), "attrisize 255"));
    std::vector<uint8_t> full = {1, 1, 1};
    CHECK(pr_check_ld(full.data(), 1, d, att, 0).empty());    // no gaps: any ld in range
  }
  // ---- imputation's cuts: the rows in whole quanta under the budget, then the draws
  {
    // 5 quanta; entries before each: 0, 10, 10, 500, 520, 521
    const int64_t qoff[6] = {0, 10, 10, 500, 520, 521};
    const size_t row = 100, ent = 50;                          // bytes per row and per entry
    // one quantum costs 6,400 + 50 x its entries
    CHECK(pr_impute_quanta(qoff, 5, 0, 1, row, ent, 1 << 28) == 1);                     // at least one
    CHECK(pr_impute_quanta(qoff, 5, 0, 2 * 6400 + 10 * 50 - 1, row, ent, 1 << 28) == 1);
    CHECK(pr_impute_quanta(qoff, 5, 0, 2 * 6400 + 10 * 50, row, ent, 1 << 28) == 2);
    CHECK(pr_impute_quanta(qoff, 5, 0, 3 * 6400 + 500 * 50 - 1, row, ent, 1 << 28) == 2);  // the third's 490 entries
    CHECK(pr_impute_quanta(qoff, 5, 0, (size_t)1 << 40, row, ent, 1 << 28) == 5);
    CHECK(pr_impute_quanta(qoff, 5, 0, (size_t)1 << 40, row, ent, 499) == 2);            // the cap on entries
    CHECK(pr_impute_quanta(qoff, 5, 2, (size_t)1 << 40, row, ent, 1 << 28) == 3);
    CHECK(pr_impute_quanta(qoff, 5, 2, 2 * 6400 + 510 * 50, row, ent, 1 << 28) == 2);
    CHECK(pr_impute_quanta(qoff, 5, 4, 1, row, ent, 1 << 28) == 1);
    // the records' share: rows x rstride x 8 plus the block's other staging stays within the
    // budget whenever more than the one draw that always goes through fits, for the block's own
    // rows -- also for a small block behind a large one.  M = 256, K = 20, d = 128, ld = 4:
    {
      const size_t rec1 = 22, rowb = 32 * 4 + 21 * 8 + 16 + 8 + 24 + rec1 * 8, entb = 4 * 8 + 24;
      const int64_t whole = 256 * 22;
      const size_t budget = (size_t)256 << 20;
      const size_t rows[] = {64, 128, 4096, 65536, 133952, 466240};
      for (size_t r : rows) {
        const int64_t ent = (int64_t)r;                        // one gap per row
        const int64_t rs = pr_impute_rstride(budget, r, rowb, ent, entb, rec1, whole);
        CHECK(rs >= (int64_t)rec1 && rs <= whole);
        const long double used = (long double)r * (rowb - rec1 * 8) + (long double)ent * entb + (long double)r * rs * 8;
        if (rs > (int64_t)rec1) CHECK(used <= (long double)budget);
        // and no smaller than it has to be: one more double per row would not fit, or it is all the draws
        if (rs < whole && rs > (int64_t)rec1) CHECK(used + (long double)r * 8 > (long double)budget);
      }
      CHECK(pr_impute_rstride(budget, 64, rowb, 64, entb, rec1, whole) == whole);          // a last block of one quantum
      CHECK(pr_impute_rstride(budget, 65536, rowb, 65536, entb, rec1, whole) < whole);
      CHECK(pr_impute_rstride(1, 64, rowb, 64, entb, rec1, whole) == (int64_t)rec1);       // nothing left: one draw
      CHECK(pr_impute_rstride(0, 64, rowb, 0, entb, rec1, whole) == (int64_t)rec1);
      // the blocks of 600,000 rows, one gap each, as impute_blocks cuts them: every block's buffer obeys the budget
      const size_t nq = (600000 + 63) / 64;
      std::vector<int64_t> qo(nq + 1);
      for (size_t b = 0; b <= nq; ++b) qo[b] = std::min<int64_t>((int64_t)b * 64, 600000);
      size_t blocks = 0;
      for (size_t q0 = 0; q0 < nq; ++blocks) {
        const size_t n = pr_impute_quanta(qo.data(), nq, q0, budget, rowb, entb, (int64_t)1 << 28);
        const int64_t ent = qo[q0 + n] - qo[q0];
        const int64_t rs = pr_impute_rstride(budget, n * 64, rowb, ent, entb, rec1, whole);
        const long double buf = (long double)(n * 64) * rs * 8;
        CHECK(buf + (long double)(n * 64) * (rowb - rec1 * 8) + (long double)ent * entb <= (long double)budget);
        q0 += n;
      }
      CHECK(blocks == 2);
    }
    // draws of 3, 1, 5, 2 clusters: records of 5, 3, 7, 4 doubles
    const int64_t off[5] = {0, 3, 4, 9, 11};
    CHECK(pr_draw_chunk(off, 4, 0, 1) == 1);                   // at least one draw
    CHECK(pr_draw_chunk(off, 4, 0, 7) == 1);
    CHECK(pr_draw_chunk(off, 4, 0, 8) == 2);
    CHECK(pr_draw_chunk(off, 4, 0, 14) == 2);
    CHECK(pr_draw_chunk(off, 4, 0, 15) == 3);
    CHECK(pr_draw_chunk(off, 4, 0, 19) == 4);
    CHECK(pr_draw_chunk(off, 4, 0, 1000) == 4);
    CHECK(pr_draw_chunk(off, 4, 2, 7) == 3 && pr_draw_chunk(off, 4, 2, 11) == 4 && pr_draw_chunk(off, 4, 3, 1) == 4);
    // the chunks of any cap tile the draws in order
    for (int64_t cap = 1; cap <= 20; ++cap) {
      int s = 0, steps = 0;
      while (s < 4) {
        const int e = pr_draw_chunk(off, 4, s, cap);
        CHECK(e > s && e <= 4);
        CHECK(e == s + 1 || off[e] - off[s] + 2 * (e - s) <= cap);
        s = e;
        ++steps;
      }
      CHECK(s == 4 && steps >= 1 && steps <= 4);
    }
  }
  if (fails) return 1;
  std::printf("impute host ok\n");
  return 0;
}
