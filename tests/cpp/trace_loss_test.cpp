// csrc/trace_loss.hpp alone: every helper against a straight-line restatement of the formula
// as the hdpm_trace_* calls wrote it out before they shared it; doubles compared by bytes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../split_and_merge_gibbs_sampling_amd/csrc/trace_loss.hpp"

static int fails = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #x);           \
      ++fails;                                                     \
    }                                                              \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// sizes -> lsz, hc, A as hdpm_trace_distances and hdpm_trace_cut_losses each spelled them
static void check_sizes(const std::vector<uint64_t>& sz, bool small = true) {
  const int Ka = (int)sz.size();
  std::vector<double> lsz(sz.size(), -1.0);
  const hdpm::TlSizes s = hdpm::tl_sizes(sz.data(), Ka, lsz.data());
  double hc = 0.0;
  uint64_t A1 = 0, A2 = 0;
  for (int a = 0; a < Ka; ++a) {
    const double want = sz[a] > 0 ? std::log2((double)sz[a]) : 0.0;
    CHECK(same_bits(lsz[a], want));
    hc = hc + (double)sz[a] * want;
    A1 += sz[a] * (uint64_t)(sz[a] > 0 ? sz[a] - 1 : 0) / 2;
    A2 += sz[a] * (sz[a] - (sz[a] > 0 ? 1 : 0)) / 2;
  }
  CHECK(same_bits(s.hc, hc));
  // (the two earlier spellings multiply first: exact below 2^32 only)
  if (small) CHECK(s.A == A1 && s.A == A2);
}

int main() {
  using namespace hdpm;
  // sizes: an empty cluster, size 1, everything in one cluster, Ka = 255, a size above 2^32
  check_sizes({5, 0, 3});
  check_sizes({1, 1, 1, 7});
  check_sizes({1000});
  {
    std::vector<uint64_t> sz(255);
    for (int a = 0; a < 255; ++a) sz[a] = (uint64_t)((a * 37) % 11) * (a + 1);   // zeros among them
    check_sizes(sz);
  }
  {
    const uint64_t big = ((uint64_t)1 << 32) + 3;
    check_sizes({big, 2, 0}, false);
    std::vector<uint64_t> sz{big, 2, 0};
    std::vector<double> lsz(3);
    // C2(2^32 + 3) = (2^32 + 3)(2^31 + 1) = 2^63 + 2^32 + 3 * 2^31 + 3, and C2(2) = 1: exact in uint64
    const uint64_t one = 1;
    CHECK(tl_sizes(sz.data(), 3, lsz.data()).A == (one << 63) + (one << 32) + 3 * (one << 31) + 3 + 1);
  }
  {
    uint64_t one = 1;
    double l = -1.0;
    const TlSizes s = tl_sizes(&one, 1, &l);
    CHECK(same_bits(l, 0.0) && same_bits(s.hc, 0.0) && s.A == 0);
  }

  // VI against the trace and against one draw, VI.lb's term: the expressions as written
  {
    const double hc = 1234.567, S = 98765.4321, l = 43210.9876, dM = 37.0, Sm = 2671.25, l1 = 1170.5;
    const int N = 1000;
    CHECK(same_bits(tl_vi(hc, S, l, dM, N), (hc + (S - 2 * l) / dM) / N));
    CHECK(same_bits(tl_vi_draw(hc, Sm, l1, N), (hc + Sm - 2 * l1) / N));
    CHECK(same_bits(tl_vi_draw(10.0, 10.0, 10.0 + 1e-12, N), 0.0));   // an undershoot clamps to +0
    CHECK(same_bits(tl_vi_draw(0.0, 0.0, 0.0, N), 0.0));
    const double lsz = std::log2(17.0), lall = std::log2(431.0 / dM), lsame = std::log2(29.0 / dM);
    CHECK(same_bits(tl_vi_lb_term(lsz, lall, lsame, N), (lsz + lall - 2 * lsame) / N));
  }

  // block rule
  CHECK(tl_block(1, 100, 50) == 1);                          // budget 1
  CHECK(tl_block((size_t)1 << 40, 100, 1000) == 64);         // large budget: kTraceMaxBlock
  CHECK(tl_block((size_t)1 << 40, 100, 7) == 7);             // ... or the count
  CHECK(tl_block(399, 100, 50) == 1);                        // cells x 4 above the budget
  CHECK(tl_block(400, 100, 50) == 1 && tl_block(1200, 100, 50) == 3 && tl_block(1200, 100, 2) == 2);
  CHECK(kTraceMaxBlock == 64);

  // label scan
  {
    std::vector<int32_t> lab{0, 3, 254, 7};
    CHECK(tl_label_max(lab.data(), 4) == 254);
    CHECK(tl_label_max(lab.data(), 2) == 3);
    lab[1] = -1;
    CHECK(tl_label_max(lab.data(), 4) == -1);
    lab[1] = 255;
    CHECK(tl_label_max(lab.data(), 4) == -1);
    CHECK(tl_label_max(lab.data(), 1) == 0);
  }

  // 63 bits: 2^63 - 1 = 7^2 x 188232082384791343 fits, 2^63 = (2^31)^2 x 2 does not
  {
    const uint64_t top = ((uint64_t)1 << 63) - 1;
    CHECK(top % 49 == 0);
    CHECK(tl_fits63(7, top / 49));
    CHECK(tl_fits63(1, top) && !tl_fits63(1, top + 1));
    CHECK(!tl_fits63((uint64_t)1 << 31, 2));
    CHECK(tl_fits63(1000000, 9223372) && !tl_fits63(1000000, 9223373));   // 10^12 M around 2^63
  }

  if (fails) return 1;
  std::printf("trace loss ok\n");
  return 0;
}
