// trace_tree.hpp -- weighted average linkage on the groups of a label trace, exact integers.
//
// The U groups are the distinct label columns of the M saved draws (trace_summary.hip,
// k_tg_*), group u holding w_u points, S[u][v] = #{m: sig_u[m] == sig_v[m]} the draws in
// which two groups share a cluster.  For clusters A, B of groups
//
//   Q_AB = sum_{u in A, v in B} w_u w_v S_uv       (uint64; the caller checks N^2 M < 2^63)
//
// is the summed co-clustering count of their points, and Q_AB / (w_A w_B) = M x the average
// psm between them: the quantity average linkage on 1 - psm maximises.  Merging adds rows of
// Q; two averages are compared by cross-multiplication in unsigned __int128, so no floating
// point decides a merge.
//
// Merge order (the rule include/hdpm.h states): among the active pairs with the largest
// Q_AB / (w_A w_B), the pair whose smaller `first` is smallest, then whose larger `first` is
// smallest; the merged cluster keeps the smaller `first`.  A cluster is named by its member
// group with the smallest `first`.  Each cluster caches its best partner among the clusters
// of higher index under that total order (a pair belongs to its lower index); a merge
// rescans the merged cluster and the lower clusters whose partner was merged away, the other
// lower clusters compare their cached partner with the new cluster.  The sequence is exactly
// the greedy one.  With the groups numbered by ascending `first` the heavy groups of a
// settled trace have the lowest indices, so the many light groups above them never rescan
// when a heavy group grows: O(U^2) there, O(U^3) at worst.
//
// Plain C++, no HIP: summary_host.cpp includes it, and tests/cpp/trace_tree_test.cpp checks it on
// the host against an O(U^3) loop.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace hdpm {

typedef unsigned __int128 tt_u128;

// merge[(U - 1) x 2]: the two clusters of step s, each named by its member group with the
// smallest `first`, the one that keeps its name in column 0.  height[U - 1]:
// 1 - Q_AB / (M w_A w_B) as a double (inspection only).  `first` values are distinct.
inline void tt_avg_linkage(int U, const uint64_t* w0, const uint64_t* first, const uint32_t* S, uint64_t M,
                           int32_t* merge, double* height) {
  if (U < 2) return;
  const size_t n = (size_t)U;
  // Q(a, b) lives at [min(a, b)][max(a, b)]: the upper triangle only
  std::vector<uint64_t> Q(n * n), w(w0, w0 + U);
  for (size_t u = 0; u < n; ++u)
    for (size_t v = u + 1; v < n; ++v) Q[u * n + v] = w[u] * w[v] * (uint64_t)S[u * n + v];
  auto q = [&](int a, int b) -> uint64_t& { return a < b ? Q[(size_t)a * n + b] : Q[(size_t)b * n + a]; };
  std::vector<char> act(n, 1);
  // nn[a]: the best partner of a among the active clusters of higher index (-1: none), so
  // every pair is owned by its lower index and the best pair overall is the best (a, nn[a])
  std::vector<int> nn(n, -1);
  // is the pair (a, b) before the pair (c, d) in the merge order?
  auto before = [&](int a, int b, int c, int d) {
    const tt_u128 l = (tt_u128)q(a, b) * (w[c] * w[d]);
    const tt_u128 r = (tt_u128)q(c, d) * (w[a] * w[b]);
    if (l != r) return l > r;
    uint64_t a0 = first[a], a1 = first[b], c0 = first[c], c1 = first[d];
    if (a0 > a1) std::swap(a0, a1);
    if (c0 > c1) std::swap(c0, c1);
    return a0 != c0 ? a0 < c0 : a1 < c1;
  };
  auto scan = [&](int a) {
    int best = -1;
    for (int x = a + 1; x < U; ++x)
      if (act[x] && (best < 0 || before(a, x, a, best))) best = x;
    nn[a] = best;
  };
  for (int a = 0; a < U; ++a) scan(a);
  for (int s = 0; s < U - 1; ++s) {
    int ba = -1;
    for (int a = 0; a < U; ++a)
      if (act[a] && nn[a] >= 0 && (ba < 0 || before(a, nn[a], ba, nn[ba]))) ba = a;
    int A = ba, B = nn[ba];
    if (first[B] < first[A]) std::swap(A, B);      // A keeps its name and holds the merged cluster
    merge[2 * s] = A;
    merge[2 * s + 1] = B;
    height[s] = 1.0 - (double)q(A, B) / ((double)M * (double)w[A] * (double)w[B]);
    act[B] = 0;
    for (int x = 0; x < U; ++x)
      if (act[x] && x != A) q(A, x) += q(B, x);
    w[A] += w[B];
    if (s == U - 2) break;
    // A's own pairs (those above it) afresh; a cluster below A or B whose partner was one of
    // them rescans, any other cluster below A only compares the merged cluster with its partner
    scan(A);
    for (int x = 0; x < U; ++x) {
      if (!act[x] || x == A) continue;
      if (nn[x] == A || nn[x] == B) scan(x);
      else if (x < A && (nn[x] < 0 || before(x, A, x, nn[x]))) nn[x] = A;
    }
  }
}

// The cut into k clusters (1 <= k <= U): the state after the first U - k merges.  out[u] is
// the cluster of group u, 0..k-1 in order of first appearance over u = 0, 1, ... (with the
// groups numbered by ascending `first`, the order of first appearance over the points).
inline void tt_cut(int U, const int32_t* merge, int k, int32_t* out) {
  std::vector<int32_t> par((size_t)U), lab((size_t)U, -1);
  for (int u = 0; u < U; ++u) par[u] = u;
  for (int s = 0; s < U - k; ++s) par[merge[2 * s + 1]] = merge[2 * s];
  int32_t next = 0;
  for (int u = 0; u < U; ++u) {
    int r = u;
    while (par[r] != r) r = par[r];
    for (int x = u; par[x] != r && x != r;) {
      const int y = par[x];
      par[x] = r;
      x = y;
    }
    if (lab[r] < 0) lab[r] = next++;
    out[u] = lab[r];
  }
}

}  // namespace hdpm
