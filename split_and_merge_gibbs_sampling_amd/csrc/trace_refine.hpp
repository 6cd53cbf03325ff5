// trace_refine.hpp -- the descent rule of hdpm_trace_refine, as functions of plain arrays.
//
// A partition c is refined by single-point moves.  The device gives, per point i, the class
// best[i] with the smallest gain[i] (the change of the loss if i alone moves there; label Ka
// is a new class of its own).  One round on the current partition with loss L:
//
//   1. the candidates are the points with gain < 0;
//   2. of the candidates whose best is the new class only the one with the smallest gain
//      stays (the lowest index breaking a tie): at most one new class per round;
//   3. no candidate: stop, converged -- c is a minimum under single-point moves;
//   4. the candidates are ordered by (gain ascending, index ascending), k their number;
//   5. trial: the first k moves applied at once, the result relabelled 0..K-1 by first
//      appearance (emptied classes go, K <= 255), its loss evaluated exactly; accepted iff
//      strictly below L; otherwise k = 1 stops the run (converged: a single move's gain is
//      the exact change, so only VI's rounding can reject it) and else k = ceil(k / 2);
//   6. after an accepted trial the next round starts from the full candidate set; after
//      max_rounds accepted rounds the run stops with converged = 0 if candidates remain.
//
// Simultaneous moves are no descent by themselves (two singletons that always co-cluster
// each gain by joining the other; moving both gains nothing), so every trial is tested on
// the evaluated loss: every accepted round is a strict descent, and the run ends.
//
// Plain C++, no HIP: summary_host.cpp drives it with the device's gains and losses,
// tests/cpp/trace_refine_test.cpp with a CPU model of both.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hdpm {

// h(t) = (t + 1) log2(t + 1) - t log2 t, h(0) = 0: what one more member adds to t log2 t.
// Never the difference of the two products, which loses eight digits at t = 1e6.
inline double rf_h(double t) {
  return t > 0.0 ? std::log2(t + 1.0) + t * std::log1p(1.0 / t) / 0.6931471805599453 : 0.0;
}

struct RfMove {
  int32_t i, to;
  double gain;
};

// steps 1, 2 and 4: the moves of one round in the order they are tried
inline void rf_select(const int32_t* best, const double* gain, int64_t N, int Ka, std::vector<RfMove>& out) {
  out.clear();
  int64_t fresh = -1;   // where the one new-class candidate sits in out
  for (int64_t i = 0; i < N; ++i) {
    if (!(gain[i] < 0.0)) continue;
    const RfMove mv{(int32_t)i, best[i], gain[i]};
    if (best[i] != Ka) out.push_back(mv);
    else if (fresh < 0) { fresh = (int64_t)out.size(); out.push_back(mv); }
    else if (gain[i] < out[(size_t)fresh].gain) out[(size_t)fresh] = mv;
  }
  std::sort(out.begin(), out.end(),
            [](const RfMove& x, const RfMove& y) { return x.gain < y.gain || (x.gain == y.gain && x.i < y.i); });
}

// labels (0..255) to 0..K-1 by first appearance, in place; returns K
inline int rf_relabel(int32_t* cl, int64_t N) {
  int map[256];
  std::fill(map, map + 256, -1);
  int K = 0;
  for (int64_t i = 0; i < N; ++i) {
    int& m = map[cl[i]];
    if (m < 0) m = K++;
    cl[i] = m;
  }
  return K;
}

// step 5's partition: the first k moves applied to cl, relabelled; returns K
inline int rf_apply(const int32_t* cl, int64_t N, const RfMove* mv, size_t k, int32_t* out) {
  std::copy(cl, cl + N, out);
  for (size_t q = 0; q < k; ++q) out[mv[q].i] = mv[q].to;
  return rf_relabel(out, N);
}

inline size_t rf_halve(size_t k) { return (k + 1) / 2; }

struct RfInfo {
  int32_t rounds, trials, converged, K;
  int64_t moved;
  double start, value;
};

// The whole run.  gains(cl, K, best, gain) fills best / gain (N each) for the partition cl
// with labels 0..K-1; loss(cl, K) is its exact loss as a V (VI's double, Binder's integer),
// compared as a V and reported as a double.  cl_out (N) gets the end state, history
// (max_rounds + 1, or null) the loss at the start and after each accepted round.
template <class V, class GainFn, class LossFn>
void rf_run(const int32_t* cl, int64_t N, int max_rounds, GainFn gains, LossFn loss, int32_t* cl_out, RfInfo* info,
            double* history) {
  std::vector<int32_t> cur(cl, cl + N), next((size_t)N), best((size_t)N);
  std::vector<double> gain((size_t)N);
  std::vector<RfMove> mv;
  RfInfo r{0, 0, 0, 0, 0, 0.0, 0.0};
  int K = rf_relabel(cur.data(), N);
  V L = loss(cur.data(), K);
  r.start = (double)L;
  if (history) history[0] = (double)L;
  for (;;) {
    gains(cur.data(), K, best.data(), gain.data());
    rf_select(best.data(), gain.data(), N, K, mv);
    if (mv.empty()) { r.converged = 1; break; }
    if (r.rounds >= max_rounds) break;
    bool accepted = false;
    for (size_t k = mv.size();; k = rf_halve(k)) {
      const int Kn = rf_apply(cur.data(), N, mv.data(), k, next.data());
      const V Ln = loss(next.data(), Kn);
      ++r.trials;
      if (Ln < L) {
        cur.swap(next);
        K = Kn;
        L = Ln;
        r.moved += (int64_t)k;
        ++r.rounds;
        if (history) history[r.rounds] = (double)L;
        accepted = true;
        break;
      }
      if (k == 1) break;
    }
    if (!accepted) { r.converged = 1; break; }
  }
  r.K = K;
  r.value = (double)L;
  std::copy(cur.begin(), cur.end(), cl_out);
  if (info) *info = r;
}

}  // namespace hdpm
