// trace_merge_test.cpp -- the host rules of csrc/trace_merge.hpp, driven by a CPU model of the
// merge gains, the single-move gains and the two losses on small traces: the tie order of the
// best pair, empty classes never chosen, the path's labels, values and step count, and the
// alternation of descent and merges with its max_merges bound and its end on a rejected merge.
// tests/test_trace_merge_host.py builds and runs it, once more under the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../split_and_merge_gibbs_sampling_amd/csrc/trace_merge.hpp"

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
static std::vector<uint64_t> sizes(const Trace& t, const int32_t* c, int Ka) {
  std::vector<uint64_t> n((size_t)Ka, 0);
  for (int i = 0; i < t.N; ++i) n[c[i]]++;
  return n;
}

// M A + P - 2 Q
static uint64_t binder_loss(const Trace& t, const int32_t* c, int Ka) {
  const auto n = sizes(t, c, Ka);
  int64_t A = 0, P = 0, Q = 0;
  for (int a = 0; a < Ka; ++a) A += c2((int64_t)n[a]);
  for (int m = 0; m < t.M; ++m) {
    std::vector<int64_t> nz((size_t)t.Kz, 0);
    for (int i = 0; i < t.N; ++i) nz[t.z[(size_t)m * t.N + i]]++;
    for (int b = 0; b < t.Kz; ++b) P += c2(nz[b]);
    for (int64_t x : table(t, c, Ka, m)) Q += c2(x);
  }
  return (uint64_t)(t.M * A + P - 2 * Q);
}
static double vi_loss(const Trace& t, const int32_t* c, int Ka) {
  const auto n = sizes(t, c, Ka);
  double hc = 0.0, s = 0.0;
  for (int a = 0; a < Ka; ++a) hc += xlog2x((int64_t)n[a]);
  for (int m = 0; m < t.M; ++m) {
    std::vector<int64_t> nz((size_t)t.Kz, 0);
    for (int i = 0; i < t.N; ++i) nz[t.z[(size_t)m * t.N + i]]++;
    for (int b = 0; b < t.Kz; ++b) s += xlog2x(nz[b]);
    for (int64_t x : table(t, c, Ka, m)) s -= 2 * xlog2x(x);
  }
  return (hc + s / t.M) / t.N;
}

// the merge gains by the formulas of include/hdpm.h
static void model_pairs(const Trace& t, bool vi, const int32_t* c, int Ka, double* g) {
  const auto n = sizes(t, c, Ka);
  std::vector<double> F((size_t)Ka * Ka, 0.0);
  std::vector<int64_t> X((size_t)Ka * Ka, 0);
  for (int m = 0; m < t.M; ++m) {
    const auto T = table(t, c, Ka, m);
    for (int a = 0; a < Ka; ++a)
      for (int b = 0; b < Ka; ++b)
        for (int z = 0; z < t.Kz; ++z) {
          const int64_t s = T[(size_t)a * t.Kz + z], u = T[(size_t)b * t.Kz + z];
          F[(size_t)a * Ka + b] += mg_f((double)s, (double)u);
          X[(size_t)a * Ka + b] += s * u;
        }
  }
  for (int a = 0; a < Ka; ++a)
    for (int b = 0; b < Ka; ++b) {
      double& o = g[(size_t)a * Ka + b];
      if (a == b || !n[a] || !n[b]) o = 0.0;
      else if (vi) o = (t.M * mg_f((double)n[a], (double)n[b]) - 2.0 * F[(size_t)a * Ka + b]) / ((double)t.M * t.N);
      else o = (double)((int64_t)t.M * (int64_t)n[a] * (int64_t)n[b] - 2 * X[(size_t)a * Ka + b]);
    }
}

// the single-move gains and their argmin (trace_refine_test.cpp's model)
static void model_moves(const Trace& t, bool vi, const int32_t* c, int Ka, int32_t* best, double* gain) {
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
      else if (vi)
        g = (t.M * (rf_h((double)n[b]) - rf_h((double)(n[a] - 1))) - 2.0 * (s[b] - s[a])) / ((double)t.M * t.N);
      else g = (double)(t.M * (n[b] - n[a] - 1) - 2 * (aff[b] - aff[a]));
      if (g < bg) { bg = g; bb = b; }
    }
    best[i] = bb;
    gain[i] = bg;
  }
}

// blocks of points: every draw has the blocks of `whole`; the first `split` draws also cut
// each block of `whole` that `cut` names in two halves
static Trace block_trace(int M, const std::vector<int>& whole, const std::vector<int>& cut, int split,
                         std::vector<int32_t>* est) {
  int N = 0;
  for (int w : whole) N += w;
  Trace t{M, N, (int)(2 * whole.size()), std::vector<int>((size_t)M * N)};
  est->assign((size_t)N, 0);
  int i0 = 0;
  for (size_t k = 0; k < whole.size(); ++k) {
    for (int i = 0; i < whole[k]; ++i) {
      const bool second = cut[k] && i >= whole[k] / 2;
      (*est)[(size_t)(i0 + i)] = (int32_t)(2 * k + (second ? 1 : 0));
      for (int m = 0; m < M; ++m) t.z[(size_t)m * N + i0 + i] = (int)(2 * k + (second && m < split ? 1 : 0));
    }
    i0 += whole[k];
  }
  return t;
}

template <class V>
struct Run {
  std::vector<int32_t> cl;
  RfInfo info;
  int32_t merges;
  std::vector<double> hist;
};

template <class V, class LossFn>
static Run<V> run(const Trace& t, bool vi, const std::vector<int32_t>& start, int max_rounds, int max_merges,
                  LossFn loss) {
  Run<V> r{std::vector<int32_t>((size_t)t.N), {}, -1, std::vector<double>((size_t)(max_rounds + max_merges + 1), -1.0)};
  std::vector<double> g;
  mg_run<V>(
      start.data(), t.N, max_rounds, max_merges,
      [&](const int32_t* c, int K, int32_t* best, double* gain) { model_moves(t, vi, c, K, best, gain); }, loss,
      [&](const int32_t* c, int K) {
        g.assign((size_t)K * K, 0.0);
        model_pairs(t, vi, c, K, g.data());
        const auto n = sizes(t, c, K);
        return mg_best(g.data(), n.data(), K);
      },
      r.cl.data(), &r.info, &r.merges, r.hist.data());
  return r;
}

int main() {
  // ---- f: the log1p form, symmetric to the bit, 0 with an empty side
  for (int s = 1; s < 40; ++s)
    for (int u = 1; u < 40; ++u) {
      const double want = xlog2x(s + u) - xlog2x(s) - xlog2x(u);
      CHECK(std::fabs(mg_f(s, u) - want) <= 1e-12 * (1.0 + want));
      CHECK(mg_f(s, u) == mg_f(u, s));
    }
  CHECK(mg_f(0.0, 5.0) == 0.0 && mg_f(5.0, 0.0) == 0.0 && mg_f(0.0, 0.0) == 0.0);

  // ---- the best pair: ties to the lowest a, then the lowest b; empty classes never chosen
  {
    const int Ka = 5;
    std::vector<double> g((size_t)Ka * Ka, 1.0);
    auto set = [&](int a, int b, double v) { g[(size_t)a * Ka + b] = g[(size_t)b * Ka + a] = v; };
    std::vector<uint64_t> n{3, 2, 4, 1, 2};
    set(1, 4, -2.0);
    set(2, 3, -2.0);
    set(1, 3, -2.0);
    MgPair p = mg_best(g.data(), n.data(), Ka);
    CHECK(p.a == 1 && p.b == 3 && p.gain == -2.0);
    set(0, 4, -2.0);
    p = mg_best(g.data(), n.data(), Ka);
    CHECK(p.a == 0 && p.b == 4);
    // class 0 empties: its entries, whatever they hold, are out
    n[0] = 0;
    set(0, 1, -INFINITY);
    p = mg_best(g.data(), n.data(), Ka);
    CHECK(p.a == 1 && p.b == 3);
    // all gains positive: the smallest still wins (the path merges whatever the sign)
    std::fill(g.begin(), g.end(), 7.0);
    set(2, 4, 6.5);
    p = mg_best(g.data(), n.data(), Ka);
    CHECK(p.a == 2 && p.b == 4 && p.gain == 6.5);
    // fewer than two non-empty classes
    std::vector<uint64_t> one{0, 0, 9, 0, 0}, none(5, 0);
    p = mg_best(g.data(), one.data(), Ka);
    CHECK(p.a == -1 && p.b == -1 && p.gain == 0.0);
    p = mg_best(g.data(), none.data(), Ka);
    CHECK(p.a == -1 && p.b == -1 && p.gain == 0.0);
    CHECK(mg_nonempty(n.data(), Ka) == 4 && mg_nonempty(one.data(), Ka) == 1);
  }

  // ---- the path on a CPU model: labels with an empty class, both losses
  for (int vi = 0; vi < 2; ++vi) {
    std::mt19937 rng(5 + vi);
    const int M = 6, N = 60, Kz = 4, Ka = 7;          // labels 0..6, class 3 empty
    Trace t{M, N, Kz, std::vector<int>((size_t)M * N)};
    std::vector<int32_t> c((size_t)N);
    for (int i = 0; i < N; ++i) {
      const int truth = (int)(rng() % 3);
      for (int m = 0; m < M; ++m) t.z[(size_t)m * N + i] = rng() % 6 == 0 ? (int)(rng() % Kz) : truth;
      c[i] = (int32_t)(truth + 4 * (rng() % 2));      // 0, 1, 2, 4, 5, 6
    }
    std::vector<int32_t> cur(c);
    auto n = sizes(t, cur.data(), Ka);
    CHECK(n[3] == 0 && mg_nonempty(n.data(), Ka) == 6);
    std::vector<int32_t> merge(12, -9);
    std::vector<double> sg(6, -9.0), val(7, -9.0);
    std::vector<int> seen_changed;
    auto value = [&]() { return vi ? vi_loss(t, cur.data(), Ka) : (double)binder_loss(t, cur.data(), Ka); };
    const int steps = mg_path(
        n.data(), Ka, 1,
        [&](int changed, double* g) {
          seen_changed.push_back(changed);
          model_pairs(t, vi != 0, cur.data(), Ka, g);
        },
        [&](int a, int b) {
          for (auto& x : cur) if (x == b) x = a;
        },
        value, merge.data(), sg.data(), val.data());
    CHECK(steps == 5 && merge[10] == -9 && sg[5] == -9.0 && val[6] == -9.0);
    std::vector<int32_t> chk(c);
    CHECK(val[0] == (vi ? vi_loss(t, chk.data(), Ka) : (double)binder_loss(t, chk.data(), Ka)));
    CHECK(seen_changed[0] == -1);
    for (int s = 0; s < steps; ++s) {
      const int a = merge[2 * s], b = merge[2 * s + 1];
      CHECK(0 <= a && a < b && b < Ka && a != 3 && b != 3);     // the lower label stays, the empty class is never named
      if (s > 0) CHECK(seen_changed[(size_t)s] == merge[2 * (s - 1)]);
      bool has_a = false, has_b = false;
      for (auto x : chk) { has_a |= x == a; has_b |= x == b; }
      CHECK(has_a && has_b);                                     // both still stand when they merge
      for (auto& x : chk) if (x == b) x = a;
      const double v = vi ? vi_loss(t, chk.data(), Ka) : (double)binder_loss(t, chk.data(), Ka);
      CHECK(val[(size_t)s + 1] == v);
      if (vi) CHECK(std::fabs(val[(size_t)s + 1] - val[(size_t)s] - sg[(size_t)s]) < 1e-12);
      else CHECK(val[(size_t)s + 1] - val[(size_t)s] == sg[(size_t)s]);
    }
    CHECK(n[(size_t)merge[2 * (steps - 1)]] == (uint64_t)N && mg_nonempty(n.data(), Ka) == 1);
    // the truth's three classes are the path's minimum
    int arg = 0;
    for (int s = 1; s <= steps; ++s) if (val[(size_t)s] < val[(size_t)arg]) arg = s;
    CHECK(arg == 3);
    // k_min at or above the classes: no step, value[0] alone; null outputs are allowed
    auto n2 = sizes(t, c.data(), Ka);
    cur = c;
    int calls = 0;
    double v0 = -1.0;
    CHECK(mg_path(n2.data(), Ka, 6, [&](int, double*) { ++calls; }, [&](int, int) { ++calls; }, value,
                  (int32_t*)nullptr, (double*)nullptr, &v0) == 0);
    CHECK(mg_path(n2.data(), Ka, 200, [&](int, double*) { ++calls; }, [&](int, int) { ++calls; }, value,
                  (int32_t*)nullptr, (double*)nullptr, (double*)nullptr) == 0);
    CHECK(calls == 0 && v0 == val[0]);
    CHECK(mg_path(n2.data(), Ka, 4, [&](int, double* g) { model_pairs(t, vi != 0, cur.data(), Ka, g); },
                  [&](int a, int b) { for (auto& x : cur) if (x == b) x = a; }, value, (int32_t*)nullptr,
                  (double*)nullptr, (double*)nullptr) == 2);
    CHECK(mg_nonempty(n2.data(), Ka) == 4);
  }

  // ---- the alternation.  One stalled pair: the draws join its halves in 6 of 10 draws
  {
    std::vector<int32_t> est;
    const Trace t = block_trace(10, {12, 8}, {1, 0}, 4, &est);       // estimate: 6 / 6 / 8
    std::vector<int32_t> best((size_t)t.N);
    std::vector<double> gain((size_t)t.N);
    std::vector<int32_t> d(est);
    const int K = rf_relabel(d.data(), t.N);
    CHECK(K == 3);
    for (int vi = 0; vi < 2; ++vi) {
      model_moves(t, vi != 0, d.data(), K, best.data(), gain.data());
      for (double g : gain) CHECK(!(g < 0.0));                       // no single move helps
    }
    CHECK(binder_loss(t, d.data(), K) == 216);
    auto rb = run<uint64_t>(t, false, est, 100, 5, [&](const int32_t* c, int k) { return binder_loss(t, c, k); });
    CHECK(rb.merges == 1 && rb.info.converged == 1 && rb.info.K == 2 && rb.info.rounds == 0 && rb.info.trials == 1);
    CHECK(rb.info.start == 216.0 && rb.info.value == 144.0 && rb.hist[0] == 216.0 && rb.hist[1] == 144.0);
    CHECK(rb.hist[2] == -1.0);
    for (int i = 0; i < t.N; ++i) CHECK(rb.cl[(size_t)i] == (i < 12 ? 0 : 1));
    auto rv = run<double>(t, true, est, 100, 5, [&](const int32_t* c, int k) { return vi_loss(t, c, k); });
    CHECK(rv.merges == 1 && rv.info.converged == 1 && rv.info.K == 2);
    CHECK(std::fabs(rv.info.start - 0.36) < 1e-12 && std::fabs(rv.info.value - 0.24) < 1e-12);
    // no merge allowed: the negative pair is left, converged = 0, the start relabelled
    auto r0 = run<uint64_t>(t, false, est, 100, 0, [&](const int32_t* c, int k) { return binder_loss(t, c, k); });
    CHECK(r0.merges == 0 && r0.info.converged == 0 && r0.info.K == 3 && r0.info.trials == 0);
    CHECK(r0.info.value == 216.0 && r0.cl == d);
    // a rejected merge ends the run: a loss that never falls
    auto rr = run<uint64_t>(t, false, est, 100, 5, [&](const int32_t*, int) { return (uint64_t)77; });
    CHECK(rr.merges == 0 && rr.info.converged == 1 && rr.info.trials == 1 && rr.info.K == 3 && rr.cl == d);
  }
  // two stalled pairs: max_merges bounds the merges, converged tells whether one was left
  {
    std::vector<int32_t> est;
    const Trace t = block_trace(10, {12, 8, 10}, {1, 0, 1}, 4, &est);
    auto loss = [&](const int32_t* c, int k) { return binder_loss(t, c, k); };
    auto r1 = run<uint64_t>(t, false, est, 100, 1, loss);
    CHECK(r1.merges == 1 && r1.info.converged == 0 && r1.info.K == 4);
    auto r2 = run<uint64_t>(t, false, est, 100, 2, loss);
    CHECK(r2.merges == 2 && r2.info.converged == 1 && r2.info.K == 3);
    CHECK(r2.hist[0] > r2.hist[1] && r2.hist[1] > r2.hist[2] && r2.hist[2] == r2.info.value && r2.hist[3] == -1.0);
    auto r9 = run<uint64_t>(t, false, est, 100, 9, loss);
    CHECK(r9.merges == 2 && r9.info.converged == 1 && r9.cl == r2.cl);
  }
  // random traces: descent and merges alternate to a partition that neither improves (Binder is
  // exact: checked by brute force), the history falls strictly and counts rounds and merges
  int alternated = 0;
  for (uint32_t seed = 1; seed <= 12; ++seed) {
    std::mt19937 rng(seed);
    const int M = 7, Kz = 4;
    int N = 48;
    Trace t{M, N, Kz, std::vector<int>((size_t)M * N)};
    std::vector<int32_t> start((size_t)N);
    if (seed % 2) {
      for (int i = 0; i < N; ++i) {
        const int truth = (int)(rng() % 3);
        for (int m = 0; m < M; ++m) t.z[(size_t)m * N + i] = rng() % 4 == 0 ? (int)(rng() % Kz) : truth;
        start[(size_t)i] = (int32_t)(rng() % 8);
      }
    } else {
      // the stalled blocks with a few points misplaced: rounds first, then merges
      t = block_trace(10, {12, 8, 10}, {1, 0, 1}, 4, &start);
      N = t.N;
      for (int k = 0; k < 3; ++k) start[(size_t)(rng() % (uint32_t)N)] = (int32_t)(rng() % 6);
    }
    auto loss = [&](const int32_t* c, int k) { return binder_loss(t, c, k); };
    auto r = run<uint64_t>(t, false, start, 100, 20, loss);
    CHECK(r.info.converged == 1);
    const int K = r.info.K, len = r.info.rounds + r.merges + 1;
    CHECK((double)loss(r.cl.data(), K) == r.info.value && r.hist[(size_t)len - 1] == r.info.value);
    CHECK(r.hist[0] == r.info.start && r.hist[(size_t)len] == -1.0);
    for (int s = 1; s < len; ++s) CHECK(r.hist[(size_t)s] < r.hist[(size_t)s - 1]);
    const uint64_t L = loss(r.cl.data(), K);
    for (int i = 0; i < N; ++i)
      for (int b = 0; b <= K && b < 255; ++b) {
        std::vector<int32_t> d(r.cl);
        d[(size_t)i] = b;
        CHECK(binder_loss(t, d.data(), K + 1) >= L);
      }
    for (int a = 0; a < K; ++a)
      for (int b = a + 1; b < K; ++b) {
        std::vector<int32_t> d(r.cl);
        for (auto& x : d) if (x == b) x = a;
        CHECK(binder_loss(t, d.data(), K) >= L);
      }
    if (r.merges > 0 && r.info.rounds > 0) ++alternated;
    // out of rounds with candidates left: no merge is tried
    auto rz = run<uint64_t>(t, false, start, 0, 20, loss);
    CHECK(rz.info.converged == 0 && rz.merges == 0 && rz.info.rounds == 0 && rz.info.trials == 0);
    // the same run with VI ends too, with a falling history
    auto rv = run<double>(t, true, start, 100, 20, [&](const int32_t* c, int k) { return vi_loss(t, c, k); });
    for (int s = 1; s < rv.info.rounds + rv.merges + 1; ++s) CHECK(rv.hist[(size_t)s] < rv.hist[(size_t)s - 1]);
  }
  CHECK(alternated > 0);
  std::printf("trace merge ok (%d runs with rounds and merges)\n", alternated);
  return 0;
}
