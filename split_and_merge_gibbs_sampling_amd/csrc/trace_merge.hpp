// trace_merge.hpp -- the host rules of hdpm_trace_merge_gains, hdpm_trace_merge_path and
// hdpm_trace_refine_merge, as functions of plain arrays.
//
// The device gives the Ka x Ka matrix of merge gains of a partition (trace_merge.hip): the
// change of the loss if classes a and b became one; 0 on the diagonal and for a pair with an
// empty class.
//
//   best pair     the pair a < b of non-empty classes with the smallest gain; the lowest a wins
//                 a tie, then the lowest b.  Fewer than two non-empty classes: {-1, -1}, gain 0.
//                 An empty class is never a candidate, whatever its entries hold.
//   path          greedy agglomeration from K0 non-empty classes down to k_min: steps =
//                 max(0, K0 - k_min).  Each step merges the best pair of the current state,
//                 whether or not its gain is negative; the merged class keeps the lower label a
//                 and b becomes empty.  value[0] is the loss of the start and value[s + 1] the
//                 loss after step s, evaluated from the folded tables, never the running sum of
//                 the gains.
//   refine_merge  alternates two phases.  The single-move descent of trace_refine.hpp (rf_run,
//                 with the rounds left of max_rounds) ends at c with loss L.  Out of rounds with
//                 candidates left: stop, converged = 0.  Otherwise the pair gains of c: no pair
//                 with gain < 0 stops the run with converged = 1 (c is a minimum under
//                 single-point moves and pair merges); after max_merges accepted merges a
//                 negative pair stops it with converged = 0.  Else the best pair is tried: the
//                 merged partition relabelled by first appearance, its loss evaluated exactly,
//                 accepted iff strictly below L.  A rejected merge stops the run with converged
//                 = 1 (VI only, by rounding); an accepted one is followed by the descent again.
//                 Every accepted step lowers the evaluated loss strictly, so the run ends.
//                 trials counts the evaluated trials of both phases.
//
// Plain C++, no HIP: summary_host.cpp drives it with the device's gains and losses,
// tests/cpp/trace_merge_test.cpp with a CPU model of both.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "trace_refine.hpp"

namespace hdpm {

// f(s, t) = (s + t) log2(s + t) - s log2 s - t log2 t, 0 if either is 0: what a merge adds to
// sum x log2 x.  Never the difference of the products, which loses eleven digits at (1e6, 1).
inline double mg_f(double s, double t) {
  return s > 0.0 && t > 0.0 ? (s * std::log1p(t / s) + t * std::log1p(s / t)) / 0.6931471805599453 : 0.0;
}

struct MgPair {
  int32_t a, b;
  double gain;
};

// the best pair of a Ka x Ka gain matrix (the upper triangle is read) with class sizes n
inline MgPair mg_best(const double* gain, const uint64_t* n, int Ka) {
  MgPair r{-1, -1, 0.0};
  for (int a = 0; a < Ka; ++a) {
    if (n[a] == 0) continue;
    for (int b = a + 1; b < Ka; ++b) {
      if (n[b] == 0) continue;
      const double g = gain[(size_t)a * Ka + b];
      if (r.a < 0 || g < r.gain) r = MgPair{a, b, g};
    }
  }
  return r;
}

inline int mg_nonempty(const uint64_t* n, int Ka) {
  int k = 0;
  for (int a = 0; a < Ka; ++a) k += n[a] != 0;
  return k;
}

// The path.  n: the Ka class sizes, updated as the classes merge.  gains(changed, g) fills the
// Ka x Ka matrix g of the current state (changed: the class the last fold changed, -1 at the
// start); fold(a, b) merges b into a; value() is the loss of the current state.  merge
// (steps x 2), step_gain (steps), val (steps + 1) may be null.  Returns the steps.
template <class GainFn, class FoldFn, class ValueFn>
int mg_path(uint64_t* n, int Ka, int k_min, GainFn gains, FoldFn fold, ValueFn value, int32_t* merge,
            double* step_gain, double* val) {
  const int steps = std::max(0, mg_nonempty(n, Ka) - k_min);
  std::vector<double> g((size_t)Ka * Ka);
  if (val) val[0] = value();
  int changed = -1;
  for (int s = 0; s < steps; ++s) {
    gains(changed, g.data());
    const MgPair p = mg_best(g.data(), n, Ka);
    if (merge) { merge[2 * s] = p.a; merge[2 * s + 1] = p.b; }
    if (step_gain) step_gain[s] = p.gain;
    fold(p.a, p.b);
    n[p.a] += n[p.b];
    n[p.b] = 0;
    changed = p.a;
    if (val) val[s + 1] = value();
  }
  return steps;
}

// cl (labels 0..K-1) with class b relabelled a, then relabelled by first appearance; returns K
inline int mg_apply(const int32_t* cl, int64_t N, int a, int b, int32_t* out) {
  for (int64_t i = 0; i < N; ++i) out[i] = cl[i] == b ? a : cl[i];
  return rf_relabel(out, N);
}

// The alternation.  gains / loss as in rf_run; pairs(cl, K) is the best pair of the partition
// cl with labels 0..K-1, all non-empty.  history (max_rounds + max_merges + 1, or null): the
// loss at the start and after each accepted round or merge.
template <class V, class GainFn, class LossFn, class PairFn>
void mg_run(const int32_t* cl, int64_t N, int max_rounds, int max_merges, GainFn gains, LossFn loss, PairFn pairs,
            int32_t* cl_out, RfInfo* info, int32_t* merges, double* history) {
  std::vector<int32_t> cur(cl, cl + N), next((size_t)N);
  RfInfo tot{0, 0, 0, 0, 0, 0.0, 0.0};
  int nm = 0, pos = 0;
  for (bool first = true;; first = false) {
    RfInfo r;
    rf_run<V>(cur.data(), N, max_rounds - tot.rounds, gains, loss, next.data(), &r, history ? history + pos : nullptr);
    cur.swap(next);
    if (first) tot.start = r.start;
    tot.rounds += r.rounds;
    tot.trials += r.trials;
    tot.moved += r.moved;
    tot.K = r.K;
    tot.value = r.value;
    pos += r.rounds;
    if (!r.converged) break;                       // out of rounds with candidates left
    const MgPair p = pairs(cur.data(), tot.K);
    if (p.a < 0 || !(p.gain < 0.0)) { tot.converged = 1; break; }
    if (nm >= max_merges) break;
    const V L = loss(cur.data(), tot.K);
    const int Kn = mg_apply(cur.data(), N, p.a, p.b, next.data());
    const V Ln = loss(next.data(), Kn);
    ++tot.trials;
    if (!(Ln < L)) { tot.converged = 1; break; }
    cur.swap(next);
    tot.K = Kn;
    tot.value = (double)Ln;
    ++nm;
    ++pos;
    if (history) history[pos] = (double)Ln;
  }
  std::copy(cur.begin(), cur.end(), cl_out);
  if (info) *info = tot;
  if (merges) *merges = nm;
}

}  // namespace hdpm
