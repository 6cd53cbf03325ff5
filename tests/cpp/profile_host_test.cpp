// csrc/profile_host.hpp: the cuts of the attributes and of the draws (every item in exactly one
// piece, in order, for budgets from 1 byte up), the argument refusals, and the scalar fold
// against the restatement of tests/profile_ref.py on a fixture that tests/test_profile_host.py
// writes (argv[1]); counts compared as integers, doubles by bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../split_and_merge_gibbs_sampling_amd/csrc/predict_host.hpp"
#include "../../split_and_merge_gibbs_sampling_amd/csrc/profile_host.hpp"

static int fails = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #x);           \
      ++fails;                                                     \
    }                                                              \
  } while (0)

static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

// every item 0 .. n - 1 once, in order, no empty piece
static bool tiles(const std::vector<int>& cut, int n) {
  if (cut.size() < 2 || cut.front() != 0 || cut.back() != n) return false;
  for (size_t c = 0; c + 1 < cut.size(); ++c)
    if (cut[c + 1] <= cut[c]) return false;
  return true;
}

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
    std::printf("FAILED: the fixture is short\n");
    ++fails;
  }
  return v;
}

int main(int argc, char** argv) {
  using namespace hdpm;
  // ---- the planner
  {
    const size_t budgets[] = {1, 7, 8, 4079, 4080, 4081, 8160, 100000, (size_t)1 << 20, (size_t)256 << 20, (size_t)1 << 40};
    const int shapes[][3] = {{1, 1, 1}, {3, 130, 255}, {255, 785, 255}, {10, 128, 16}, {255, 1, 2}};   // Ka, d, ld
    for (size_t b : budgets)
      for (auto& sh : shapes) {
        const int Ka = sh[0], d = sh[1], ld = sh[2];
        for (int slot : {8, 16}) {
          const std::vector<int> cut = pf_attr_blocks(b, Ka, ld, slot, d);
          CHECK(tiles(cut, d));
          for (size_t c = 0; c + 1 < cut.size(); ++c) {
            const long double bytes = (long double)(cut[c + 1] - cut[c]) * Ka * ld * slot;
            CHECK(cut[c + 1] - cut[c] == 1 || bytes <= (long double)b);          // within the budget, or one attribute
          }
          // and no smaller than it has to be: one attribute more per block would not fit
          if (cut.size() > 2) CHECK((long double)(cut[1] + 1) * Ka * ld * slot > (long double)b);
        }
        for (int M : {1, 2, 37, 1000}) {
          const std::vector<int> cut = pf_draw_chunks(b, Ka, d, M);
          CHECK(tiles(cut, M));
          for (size_t c = 0; c + 1 < cut.size(); ++c)
            CHECK(cut[c + 1] - cut[c] == 1 || (long double)(cut[c + 1] - cut[c]) * Ka * d * 8 <= (long double)b);
          if (cut.size() > 2) CHECK((long double)(cut[1] + 1) * Ka * d * 8 > (long double)b);
        }
      }
    // 1 byte: one attribute per block and one draw per chunk; a large budget: one piece
    CHECK(pf_attr_blocks(1, 3, 255, 16, 130).size() == 131);
    CHECK(pf_draw_chunks(1, 3, 130, 37).size() == 38);
    CHECK(pf_attr_blocks((size_t)256 << 20, 3, 255, 16, 130).size() == 2);
    CHECK(pf_draw_chunks((size_t)256 << 20, 3, 130, 37).size() == 2);
    // 255 x 785 x 255 x 16 bytes = 0.8 GB against 256 MiB: 1,040,400 bytes per attribute, 258 fit
    const std::vector<int> big = pf_attr_blocks((size_t)256 << 20, 255, 255, 16, 785);
    CHECK(big.size() == 5 && big[1] == 258 && big[4] == 785);
    // 3 x 130 x 8 = 3120 bytes per draw: 2 draws in 6240 bytes, not in 6239
    CHECK(pf_draw_chunks(6240, 3, 130, 5) == (std::vector<int>{0, 2, 4, 5}));
    CHECK(pf_draw_chunks(6239, 3, 130, 5) == (std::vector<int>{0, 1, 2, 3, 4, 5}));
  }
  // ---- the refusals
  {
    const int32_t att[4] = {2, 17, 255, 3};
    CHECK(pf_check_ld(4, att, 255).empty());
    CHECK(pf_check_ld(2, att, 17).empty());
    CHECK(has(pf_check_ld(4, att, 256), "ld must be in 1..255"));
    CHECK(has(pf_check_ld(4, att, 0), "ld must be in 1..255"));
    const std::string m = pf_check_ld(4, att, 254);
    CHECK(has(m, "ld is 254") && has(m, "attrisize 255") && has(m, "attribute 2"));
    const std::string m1 = pf_check_ld(4, att, 16);
    CHECK(has(m1, "attrisize 17") && has(m1, "attribute 1"));
    // the partition's check is hdpm_predict_new's (predict_host.hpp)
    const int32_t cl[5] = {0, 2, 1, 2, 0};
    CHECK(pr_check_classes(cl, 5, 3).empty());
    CHECK(pr_check_classes(cl, 5, 255).empty());               // empty classes are allowed
    CHECK(has(pr_check_classes(cl, 5, 2), "0..Ka-1") && has(pr_check_classes(cl, 5, 2), "point 1"));
    CHECK(has(pr_check_classes(cl, 5, 0), "Ka must be in 1..255"));
    CHECK(has(pr_check_classes(cl, 5, 256), "Ka must be in 1..255"));
    const int32_t neg[2] = {0, -1};
    CHECK(has(pr_check_classes(neg, 2, 3), "point 1"));
  }
  // ---- the fold on the fixture
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "rb");
    CHECK(f != nullptr);
    if (f) {
      const std::vector<int32_t> h = take<int32_t>(f, 6);
      const int M = h[0], Ka = h[1], Kz = h[2], d = h[3], ld = h[4], rows = h[5];
      const std::vector<int32_t> att = take<int32_t>(f, d), K = take<int32_t>(f, M);
      const std::vector<uint32_t> tab = take<uint32_t>(f, (size_t)M * Ka * Kz);
      const std::vector<uint64_t> na = take<uint64_t>(f, Ka);
      const std::vector<uint8_t> cen = take<uint8_t>(f, (size_t)rows * d);
      const std::vector<double> sig = take<double>(f, (size_t)rows * d), emm = take<double>(f, (size_t)rows * d * 2);
      const size_t nl = (size_t)Ka * d * ld, n = (size_t)Ka * d;
      const std::vector<uint64_t> cnt_w = take<uint64_t>(f, nl);
      const std::vector<double> pmf_w = take<double>(f, nl), mean_w = take<double>(f, n), var_w = take<double>(f, n),
                                tr_w = take<double>(f, (size_t)M * n);
      CHECK(std::fgetc(f) == EOF);
      std::fclose(f);
      std::vector<int64_t> off((size_t)M + 1, 0);
      for (int s = 0; s < M; ++s) off[s + 1] = off[s] + K[s];
      CHECK(off[M] == rows);
      const PfIn in{M, Ka, Kz, d, ld, att.data(), off.data(), tab.data(), na.data(), cen.data(), d, sig.data(), emm.data()};
      std::vector<uint64_t> cnt(nl, 99);
      std::vector<double> pmf(nl, -1.0), mean(n, -1.0), var(n, -1.0), tr((size_t)M * n, -1.0);
      pf_fold(in, cnt.data(), pmf.data(), mean.data(), var.data(), tr.data());
      CHECK(cnt == cnt_w);
      CHECK(std::memcmp(pmf.data(), pmf_w.data(), nl * 8) == 0);
      CHECK(std::memcmp(mean.data(), mean_w.data(), n * 8) == 0);
      CHECK(std::memcmp(var.data(), var_w.data(), n * 8) == 0);
      CHECK(std::memcmp(tr.data(), tr_w.data(), (size_t)M * n * 8) == 0);
      // any output may be null: the others keep their bytes
      std::vector<double> mean2(n, -1.0);
      pf_fold(in, nullptr, nullptr, mean2.data(), nullptr, nullptr);
      CHECK(std::memcmp(mean2.data(), mean_w.data(), n * 8) == 0);
      std::vector<uint64_t> cnt2(nl, 99);
      pf_fold(in, cnt2.data(), nullptr, nullptr, nullptr, nullptr);
      CHECK(cnt2 == cnt_w);
      std::printf("fold checked: M %d Ka %d d %d ld %d\n", M, Ka, d, ld);
    }
  }
  if (fails) return 1;
  std::printf("profile host ok\n");
  return 0;
}
