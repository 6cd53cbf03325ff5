// csrc/phi_host.hpp alone: the output layout at literal values, the view over a hand-filled
// buffer, the hand-back bit, every row of the re-run ladder's table, and the log-likelihood
// fold against the loop it replaced (bit for bit) and against a case a plain sum gets wrong.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../split_and_merge_gibbs_sampling_amd/csrc/phi_host.hpp"

static int fails = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #x);           \
      ++fails;                                                     \
    }                                                              \
  } while (0)

static bool layout_is(int T, int d, size_t pick, size_t sig, size_t ll, size_t bytes, size_t state) {
  const PhiOutLayout L = phi_out_layout(T, d);
  return L.o_pick == pick && L.o_sig == sig && L.o_ll == ll && L.bytes == bytes && L.o_state == state;
}

// the fold as device_update_phi and dspec_commit wrote it: per cluster, its two terms
static double fold_as_written(const double* ll, int T) {
  double hi = 0.0, lo = 0.0;
  for (int t = 0; t < T; ++t) {
    for (int q = 0; q < 2; ++q) {
      const double x = ll[2 * t + q], s = hi + x;
      lo += std::fabs(hi) >= std::fabs(x) ? (hi - s) + x : (x - s) + hi;
      hi = s;
    }
  }
  return hi + lo;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int main() {
  using namespace phi_host;
  // layout
  CHECK(layout_is(1, 1, 16, 32, 40, 56, 64));
  CHECK(layout_is(3, 5, 16, 32, 152, 200, 208));
  CHECK(layout_is(2, 16, 16, 48, 304, 336, 336));   // T d a multiple of 16: no padding before the sigmas

  // the view over a hand-filled buffer (T = 3, d = 5)
  {
    const int T = 3, d = 5;
    const PhiOutLayout L = phi_out_layout(T, d);
    std::vector<uint8_t> buf(L.o_state + 625 * 4, 0xEE);
    const int status = 4;
    const int64_t cons = ((int64_t)7 << 32) + 123;   // (above 2^32: all 8 bytes are read)
    std::memcpy(buf.data(), &status, 4);
    std::memcpy(buf.data() + 8, &cons, 8);
    for (int q = 0; q < T * d; ++q) {
      buf[L.o_pick + q] = (uint8_t)(q + 1);
      const double s = 0.5 + q;
      std::memcpy(buf.data() + L.o_sig + 8 * q, &s, 8);
    }
    for (int q = 0; q < 2 * T; ++q) {
      const double x = -1.0 - q;
      std::memcpy(buf.data() + L.o_ll + 8 * q, &x, 8);
    }
    for (uint32_t q = 0; q < 625; ++q) std::memcpy(buf.data() + L.o_state + 4 * q, &q, 4);
    const PhiOutView v(buf.data(), L);
    CHECK(v.status() == 4);
    CHECK(v.cons() == cons);
    for (int q = 0; q < T * d; ++q) CHECK(v.pick()[q] == q + 1 && v.sig()[q] == 0.5 + q);
    for (int q = 0; q < 2 * T; ++q) CHECK(v.ll()[q] == -1.0 - q);
    CHECK(v.state_words()[0] == 0 && v.state_words()[623] == 623 && v.state_words()[624] == 624);

    // the parameters into labelled rows, and into rows 0..T-1
    const int labs[3] = {4, 0, 2};
    std::vector<uint8_t> cen(5 * d, 0);
    std::vector<double> sig(5 * d, -1.0);
    phi_copy_params(v, T, d, labs, cen.data(), sig.data());
    for (int t = 0; t < T; ++t)
      for (int j = 0; j < d; ++j)
        CHECK(cen[labs[t] * d + j] == t * d + j + 2 && sig[labs[t] * d + j] == 0.5 + t * d + j);
    for (int j = 0; j < d; ++j) CHECK(cen[1 * d + j] == 0 && sig[3 * d + j] == -1.0);
    phi_copy_params(v, T, d, nullptr, cen.data(), sig.data());
    for (int q = 0; q < T * d; ++q) CHECK(cen[q] == q + 2 && sig[q] == 0.5 + q);
  }

  // hand-back bit
  CHECK(phi_handback_bit(-3) == 1);                   // negative: clamped to 0
  CHECK(phi_handback_bit(0) == (int64_t)1 << 15);     // Ok, but the host cannot adopt it
  CHECK(phi_handback_bit(9) == (int64_t)1 << 9);
  CHECK(phi_handback_bit(20) == (int64_t)1 << 14);

  // the ladder: mode ran x status x tree
  for (int status = -1; status <= 12; ++status)
    for (int tree = 0; tree < 2; ++tree) {
      const bool window = status == kWindow || status == kShort;
      // the walks are the last resort
      CHECK(phi_rerun_mode(kWalks, status, tree) == kNoRerun);
      // the trees go to the walks when a pick depended on the uniform, else hand back
      CHECK(phi_rerun_mode(kTree, status, tree) == (status == kNonDet ? kWalks : kNoRerun));
      // the fast path: done, or the walks (NonDet), or the caller's window to widen, or the
      // general kernels
      const int want = status == kOk ? kNoRerun : status == kNonDet ? kWalks : window ? kNoRerun : tree ? kTree : kWalks;
      CHECK(phi_rerun_mode(kFast, status, tree) == want);
    }
  CHECK(kOk == 0 && kWindow == 4 && kShort == 5 && kNonDet == 9 && kWalks == 0 && kTree == 1 && kFast == 2);

  // the fold
  {
    const double x[4] = {1e16, 1.0, -1e16, 0.0};
    CHECK(phi_ll_fold(x, 2) == 1.0);
    volatile double plain = 0.0;
    for (double v : x) plain = plain + v;
    CHECK(plain == 0.0);
    CHECK(phi_ll_fold(x, 0) == 0.0);
    std::mt19937_64 g(12345);
    std::uniform_real_distribution<double> mant(-1.0, 1.0);
    std::uniform_int_distribution<int> ex(-30, 60), len(1, 400);
    for (int rep = 0; rep < 300; ++rep) {
      const int T = len(g);
      std::vector<double> ll(2 * T);
      for (double& v : ll) v = std::ldexp(mant(g), ex(g));
      CHECK(same_bits(phi_ll_fold(ll.data(), T), fold_as_written(ll.data(), T)));
    }
  }

  if (fails) return 1;
  std::printf("phi host ok\n");
  return 0;
}
