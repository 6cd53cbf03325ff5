// trace_refine_test.cpp -- the descent rule of csrc/trace_refine.hpp on the host, driven by a
// CPU model of the gains and of the two losses on small traces: the selection, the new-class
// rule, the halving and the relabelling, each against a straight-line restatement; Binder's
// end state against brute force (move the point, recompute the integer); and that a rejected
// trial of one move ends the run.  tests/test_trace_refine_host.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../split_and_merge_gibbs_sampling_amd/csrc/trace_refine.hpp"

using namespace hdpm;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

struct Trace {
  int M, N, Kz;
  std::vector<int> z;   // M x N
};

// T^m[a][b] of c (labels 0..Ka-1) against draw m
static std::vector<int64_t> table(const Trace& t, const int32_t* c, int Ka, int m) {
  std::vector<int64_t> T((size_t)Ka * t.Kz, 0);
  for (int i = 0; i < t.N; ++i) T[(size_t)c[i] * t.Kz + t.z[(size_t)m * t.N + i]]++;
  return T;
}
static int64_t c2(int64_t x) { return x * (x - 1) / 2; }
static double xlog2x(int64_t x) { return x > 0 ? (double)x * std::log2((double)x) : 0.0; }

// M A + P - 2 Q
static uint64_t binder_loss(const Trace& t, const int32_t* c, int Ka) {
  std::vector<int64_t> n((size_t)Ka, 0);
  for (int i = 0; i < t.N; ++i) n[c[i]]++;
  int64_t A = 0, P = 0, Q = 0;
  for (int a = 0; a < Ka; ++a) A += c2(n[a]);
  for (int m = 0; m < t.M; ++m) {
    std::vector<int64_t> nz((size_t)t.Kz, 0);
    for (int i = 0; i < t.N; ++i) nz[t.z[(size_t)m * t.N + i]]++;
    for (int b = 0; b < t.Kz; ++b) P += c2(nz[b]);
    for (int64_t x : table(t, c, Ka, m)) Q += c2(x);
  }
  return (uint64_t)(t.M * A + P - 2 * Q);
}
static double vi_loss(const Trace& t, const int32_t* c, int Ka) {
  std::vector<int64_t> n((size_t)Ka, 0);
  for (int i = 0; i < t.N; ++i) n[c[i]]++;
  double hc = 0.0, s = 0.0;
  for (int a = 0; a < Ka; ++a) hc += xlog2x(n[a]);
  for (int m = 0; m < t.M; ++m) {
    std::vector<int64_t> nz((size_t)t.Kz, 0);
    for (int i = 0; i < t.N; ++i) nz[t.z[(size_t)m * t.N + i]]++;
    for (int b = 0; b < t.Kz; ++b) s += xlog2x(nz[b]);
    for (int64_t x : table(t, c, Ka, m)) s -= 2 * xlog2x(x);
  }
  return (hc + s / t.M) / t.N;
}

// the gains by the formulas of include/hdpm.h and their argmin by its tie rule
static void model_gains(const Trace& t, bool vi, const int32_t* c, int Ka, int32_t* best, double* gain) {
  const int L = Ka + 1;
  std::vector<int64_t> n((size_t)L, 0);
  for (int i = 0; i < t.N; ++i) n[c[i]]++;
  std::vector<std::vector<int64_t>> T;
  for (int m = 0; m < t.M; ++m) T.push_back(table(t, c, Ka, m));
  for (int i = 0; i < t.N; ++i) {
    const int a = c[i];
    std::vector<double> s((size_t)L, 0.0);
    std::vector<int64_t> aff((size_t)L, 0);
    for (int m = 0; m < t.M; ++m) {
      const int zb = t.z[(size_t)m * t.N + i];
      for (int b = 0; b < Ka; ++b) {
        const int64_t x = T[m][(size_t)b * t.Kz + zb];
        aff[b] += x;
        s[b] += b == a ? rf_h((double)(x - 1)) : rf_h((double)x);
      }
    }
    int bb = a;
    double bg = 0.0;
    for (int b = 0; b < L; ++b) {
      double g;
      if (b == a) g = 0.0;
      else if (b == 255) g = INFINITY;
      else if (vi)
        g = (t.M * (rf_h((double)n[b]) - rf_h((double)(n[a] - 1))) - 2.0 * (s[b] - s[a])) / ((double)t.M * t.N);
      else g = (double)(t.M * (n[b] - n[a] - 1) - 2 * (aff[b] - aff[a]));
      if (g < bg) { bg = g; bb = b; }
    }
    best[i] = bb;
    gain[i] = bg;
  }
}

static Trace random_trace(uint32_t seed, int M, int N, int K, std::vector<int32_t>* start, int Ks) {
  std::mt19937 rng(seed);
  Trace t{M, N, K, std::vector<int>((size_t)M * N)};
  std::vector<int> truth((size_t)N);
  for (int i = 0; i < N; ++i) truth[i] = (int)(rng() % (uint32_t)K);
  for (int m = 0; m < M; ++m)
    for (int i = 0; i < N; ++i) t.z[(size_t)m * N + i] = rng() % 5 == 0 ? (int)(rng() % (uint32_t)K) : truth[i];
  start->resize((size_t)N);
  for (int i = 0; i < N; ++i) (*start)[i] = (int32_t)(rng() % (uint32_t)Ks);
  return t;
}

static void test_helpers() {
  CHECK(rf_h(0.0) == 0.0 && rf_h(1.0) == 2.0);
  CHECK(std::fabs(rf_h(3.0) - (4 * 2.0 - 3 * std::log2(3.0))) < 1e-14);
  CHECK(rf_halve(1) == 1 && rf_halve(2) == 1 && rf_halve(3) == 2 && rf_halve(7) == 4 && rf_halve(8) == 4);
  int32_t c[7] = {5, 5, 2, 9, 2, 0, 9};
  CHECK(rf_relabel(c, 7) == 4);
  const int32_t want[7] = {0, 0, 1, 2, 1, 3, 2};
  CHECK(std::memcmp(c, want, sizeof c) == 0);
  // selection: of the new-class candidates (best == Ka = 3) only point 1 stays -- the
  // smallest gain, the lower index of the tie with point 4; gain 0 and above are no
  // candidates; the order is (gain, index)
  const int32_t best[7] = {3, 3, 1, 0, 3, 2, 1};
  const double gain[7] = {-1.0, -2.0, -2.0, 0.0, -2.0, -0.5, 1.0};
  std::vector<RfMove> mv;
  rf_select(best, gain, 7, 3, mv);
  CHECK(mv.size() == 3);
  CHECK(mv[0].i == 1 && mv[0].to == 3 && mv[0].gain == -2.0);
  CHECK(mv[1].i == 2 && mv[1].to == 1);
  CHECK(mv[2].i == 5 && mv[2].to == 2);
  // the first k moves applied at once, emptied classes dropped
  const int32_t cur[4] = {0, 1, 2, 2};
  const RfMove two[2] = {{1, 0, -1.0}, {0, 3, -0.5}};
  int32_t out[4];
  CHECK(rf_apply(cur, 4, two, 1, out) == 2 && out[0] == 0 && out[1] == 0 && out[2] == 1 && out[3] == 1);
  CHECK(rf_apply(cur, 4, two, 2, out) == 3 && out[0] == 0 && out[1] == 1 && out[2] == 2 && out[3] == 2);
  rf_select(best, gain, 0, 3, mv);
  CHECK(mv.empty());
}

template <class V>
static RfInfo run(const Trace& t, bool vi, const std::vector<int32_t>& start, int max_rounds,
                  std::vector<int32_t>* end, std::vector<double>* hist) {
  RfInfo info;
  end->assign(start.size(), -1);
  hist->assign((size_t)max_rounds + 1, -1.0);
  rf_run<V>(start.data(), t.N, max_rounds,
            [&](const int32_t* c, int K, int32_t* b, double* g) { model_gains(t, vi, c, K, b, g); },
            [&](const int32_t* c, int K) { return vi ? (V)vi_loss(t, c, K) : (V)binder_loss(t, c, K); },
            end->data(), &info, hist->data());
  return info;
}

static void test_descent(bool vi) {
  for (uint32_t seed = 1; seed <= 6; ++seed) {
    std::vector<int32_t> start, end;
    std::vector<double> hist;
    const Trace t = random_trace(seed, 7, 30 + (int)seed, 4, &start, 6);
    const RfInfo r = vi ? run<double>(t, vi, start, 100, &end, &hist) : run<uint64_t>(t, vi, start, 100, &end, &hist);
    CHECK(r.converged == 1 && r.rounds >= 1 && r.trials >= r.rounds && r.moved >= r.rounds);
    for (int q = 0; q < r.rounds; ++q) CHECK(hist[q + 1] < hist[q]);
    CHECK(hist[0] == r.start && hist[r.rounds] == r.value);
    // the end state is labelled by first appearance and carries the reported loss
    std::vector<int32_t> again(end);
    CHECK(rf_relabel(again.data(), t.N) == r.K && again == end);
    CHECK(r.value == (vi ? vi_loss(t, end.data(), r.K) : (double)binder_loss(t, end.data(), r.K)));
    if (vi) continue;
    // Binder: no single move lowers the integer, by brute force (the new class included)
    const uint64_t base = binder_loss(t, end.data(), r.K);
    for (int i = 0; i < t.N; ++i)
      for (int b = 0; b <= r.K; ++b) {
        std::vector<int32_t> d(end);
        d[i] = b;
        const int K = rf_relabel(d.data(), t.N);
        CHECK(binder_loss(t, d.data(), K) >= base);
      }
  }
}

// points 0 and 1 share a draw cluster of their own in every draw; the start has them in two
// singleton classes: each gains by joining the other, moving both gains nothing
static void test_halving(bool vi) {
  Trace t{5, 12, 2, std::vector<int>(60, 1)};
  for (int m = 0; m < 5; ++m) t.z[(size_t)m * 12] = t.z[(size_t)m * 12 + 1] = 0;
  std::vector<int32_t> start(12, 2), end;
  start[0] = 0;
  start[1] = 1;
  std::vector<double> hist;
  std::vector<int32_t> best(12);
  std::vector<double> gain(12);
  model_gains(t, vi, start.data(), 3, best.data(), gain.data());
  CHECK(best[0] == 1 && best[1] == 0 && gain[0] < 0 && gain[0] == gain[1]);
  if (!vi) CHECK(gain[0] == -5.0);
  const RfInfo r = vi ? run<double>(t, vi, start, 10, &end, &hist) : run<uint64_t>(t, vi, start, 10, &end, &hist);
  CHECK(r.trials == 2 && r.rounds == 1 && r.moved == 1 && r.converged == 1 && r.K == 2);
  CHECK(vi ? std::fabs(r.value) < 1e-14 : r.value == 0.0);
  CHECK(end[0] == 0 && end[1] == 0);
  for (int i = 2; i < 12; ++i) CHECK(end[i] == 1);
  // no rounds allowed: the start relabelled, not converged since candidates exist
  std::vector<int32_t> shifted(start);
  for (auto& x : shifted) x += 7;
  const RfInfo r0 = run<uint64_t>(t, false, shifted, 0, &end, &hist);
  CHECK(r0.rounds == 0 && r0.trials == 0 && r0.converged == 0 && r0.K == 3 && end == start);
  // a minimum: returned with no trial
  std::vector<int32_t> fin{0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
  const RfInfo r1 = run<uint64_t>(t, false, fin, 5, &end, &hist);
  CHECK(r1.rounds == 0 && r1.trials == 0 && r1.converged == 1 && end == fin && r1.start == r1.value);
}

// gains that promise what the loss does not keep (as VI's rounding can): five candidates,
// trials of 5, 3, 2 and 1 moves all rejected, and k = 1 ends the run as converged
static void test_single_move_rejected() {
  const int N = 8;
  int calls = 0;
  std::vector<size_t> sizes;
  RfInfo info;
  std::vector<int32_t> start(N, 0), end(N);
  for (int i = 4; i < N; ++i) start[i] = 1;
  std::vector<double> hist(4, -1.0);
  rf_run<double>(start.data(), N, 3,
                 [&](const int32_t*, int K, int32_t* b, double* g) {
                   CHECK(K == 2);
                   // points 1..5 would change sides; point 0 stays, so relabelling keeps the names
                   for (int i = 0; i < N; ++i) {
                     const bool cand = i >= 1 && i <= 5;
                     b[i] = cand ? 1 - start[i] : start[i];
                     g[i] = cand ? -1e-17 * (i + 1) : 0.0;
                   }
                 },
                 [&](const int32_t* c, int) {
                   size_t moved = 0;
                   for (int i = 0; i < N; ++i) moved += c[i] != start[i];
                   if (calls++) sizes.push_back(moved);
                   return 1.0;
                 },
                 end.data(), &info, hist.data());
  CHECK(info.trials == 4 && info.rounds == 0 && info.converged == 1 && info.moved == 0 && end == start);
  CHECK(sizes.size() == 4 && sizes[0] == 5 && sizes[1] == 3 && sizes[2] == 2 && sizes[3] == 1);
  CHECK(hist[0] == 1.0 && hist[1] == -1.0);
}

int main() {
  test_helpers();
  test_descent(false);
  test_descent(true);
  test_halving(false);
  test_halving(true);
  test_single_move_rejected();
  std::printf("trace refine ok\n");
  return 0;
}
