// csrc/trace_tree.hpp against the greedy definition written out: at every step all active
// pairs are scored from the groups' own w and S (no merged rows kept), the best is taken
// under the tie rule with __int128 fractions, and the merge lists must be identical.
// Random symmetric S with few distinct values (ties at every level), weights up to 1e5,
// `first` in index order and permuted; the cuts of tt_cut against a relabelled replay.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../split_and_merge_gibbs_sampling_amd/csrc/trace_tree.hpp"

typedef unsigned __int128 u128;

static void greedy(int U, const std::vector<uint64_t>& w, const std::vector<uint64_t>& first,
                   const std::vector<uint32_t>& S, std::vector<int32_t>& merge) {
  std::vector<std::vector<int>> mem((size_t)U);
  std::vector<char> act((size_t)U, 1);
  for (int u = 0; u < U; ++u) mem[u] = {u};
  merge.assign((size_t)std::max(0, U - 1) * 2, -1);
  for (int s = 0; s < U - 1; ++s) {
    int bA = -1, bB = -1;
    u128 bq = 0, bd = 1;
    uint64_t b0 = 0, b1 = 0;
    for (int A = 0; A < U; ++A) {
      if (!act[A]) continue;
      for (int B = A + 1; B < U; ++B) {
        if (!act[B]) continue;
        u128 q = 0, wa = 0, wb = 0;
        for (int u : mem[A]) wa += w[u];
        for (int v : mem[B]) wb += w[v];
        for (int u : mem[A])
          for (int v : mem[B]) q += (u128)w[u] * w[v] * S[(size_t)u * U + v];
        const u128 d = wa * wb;
        uint64_t f0 = std::min(first[A], first[B]), f1 = std::max(first[A], first[B]);
        bool take = bA < 0;
        if (!take) {
          const u128 l = q * bd, r = bq * d;      // q / d against bq / bd
          take = l > r || (l == r && (f0 < b0 || (f0 == b0 && f1 < b1)));
        }
        if (take) { bA = A; bB = B; bq = q; bd = d; b0 = f0; b1 = f1; }
      }
    }
    if (first[bB] < first[bA]) std::swap(bA, bB);
    merge[2 * s] = bA;
    merge[2 * s + 1] = bB;
    mem[bA].insert(mem[bA].end(), mem[bB].begin(), mem[bB].end());
    // the merged cluster keeps the smaller first, which is bA's own already
    act[bB] = 0;
  }
}

static int run_case(int U, int levels, uint64_t wmax, bool permute, unsigned seed) {
  std::mt19937_64 g(seed);
  std::vector<uint64_t> w((size_t)U), first((size_t)U);
  for (int u = 0; u < U; ++u) {
    w[u] = 1 + g() % wmax;
    first[u] = (uint64_t)u * 3 + 1;
  }
  if (permute) std::shuffle(first.begin(), first.end(), g);
  const uint32_t M = 40;
  std::vector<uint32_t> S((size_t)U * U, M);
  for (int u = 0; u < U; ++u)
    for (int v = u + 1; v < U; ++v) S[(size_t)u * U + v] = S[(size_t)v * U + u] = (uint32_t)(g() % levels) * (M / levels);
  std::vector<int32_t> want, got((size_t)std::max(0, U - 1) * 2, -7);
  std::vector<double> h((size_t)std::max(0, U - 1), -1.0);
  greedy(U, w, first, S, want);
  hdpm::tt_avg_linkage(U, w.data(), first.data(), S.data(), M, got.data(), h.data());
  if (got != want) {
    for (size_t s = 0; s + 1 < got.size(); s += 2)
      if (got[s] != want[s] || got[s + 1] != want[s + 1]) {
        std::printf("U=%d levels=%d seed=%u: step %zu got (%d,%d) want (%d,%d)\n", U, levels, seed, s / 2, got[s],
                    got[s + 1], want[s], want[s + 1]);
        break;
      }
    return 1;
  }
  for (double x : h)
    if (!(x >= 0.0 && x <= 1.0)) { std::printf("height %g out of range\n", x); return 1; }
  // cuts: replay the merges on a label vector, relabel by first appearance
  std::vector<int32_t> cl((size_t)U), out((size_t)U);
  for (int k = 1; k <= U; ++k) {
    for (int u = 0; u < U; ++u) cl[u] = u;
    for (int s = 0; s < U - k; ++s)
      for (int u = 0; u < U; ++u)
        if (cl[u] == want[2 * s + 1]) cl[u] = want[2 * s];
    std::vector<int32_t> name((size_t)U, -1);
    int32_t next = 0;
    for (int u = 0; u < U; ++u) {
      if (name[cl[u]] < 0) name[cl[u]] = next++;
      cl[u] = name[cl[u]];
    }
    hdpm::tt_cut(U, got.data(), k, out.data());
    if (next != k || out != cl) { std::printf("U=%d: cut %d differs\n", U, k); return 1; }
    if (U > 40 && k > 12 && k < U - 12) k += 6;      // every cut when small, a stride in the middle of large trees
  }
  return 0;
}

int main() {
  int bad = 0, cases = 0;
  const int sizes[] = {1, 2, 3, 17, 200};
  for (int U : sizes)
    for (int levels : {1, 2, 4, 20})
      for (int perm = 0; perm < 2; ++perm)
        for (unsigned seed = 0; seed < (U >= 200 ? 2u : 6u); ++seed) {
          bad += run_case(U, levels, levels == 1 ? 1 : 100000, perm != 0, seed * 31 + U);
          ++cases;
        }
  // equal weights with few levels: exact rational ties between clusters of different sizes
  for (unsigned seed = 0; seed < 6; ++seed) {
    bad += run_case(17, 2, 1, true, 1000 + seed);
    bad += run_case(60, 3, 2, false, 2000 + seed);
    cases += 2;
  }
  std::printf("%d cases, %d bad\n", cases, bad);
  if (bad == 0) std::printf("trace tree ok\n");
  return bad != 0;
}
