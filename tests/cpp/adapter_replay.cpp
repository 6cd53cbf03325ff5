// adapter_replay.cpp -- test infrastructure: replays the Rcpp adapter's C-ABI call sequence
// (integration/hdpm_chain.hpp, the body of integration/launcher_hip.cpp) against the CPU
// oracle's run_markov_chain (oracle/src/chain.c, la:6-174), over consecutive calls that
// share one random stream as consecutive R calls do without set.seed (zoo_simulator.R runs
// several chains in a row): .Random.seed in -> chain -> the advanced .Random.seed out -> the
// next call.
//
// Input (binary, little-endian; written by tests/test_gpu_adapter.py):
//   int32 n, d; f64 gamma; int32 attrisize[d]; f64 v[d], w[d]; f64 data[n * d] (column-major,
//   the NumericMatrix); uint32 seed (set.seed); int32 ncalls; per call: int32 params[12]
//   (hdpm_chain_params order), int32 has_init, int32 init[n] when has_init.
// Output: one line per poisoned input and per call; exit status 0 when every check passes.
// Compared per call: the status, and on success total_cls, c_i, accepted, final_ass and every
// saved iteration's centers and sigmas (the oracle's traced driver) bit for bit,
// log-likelihoods within 1e-10 relative (north_star), the 625-word stream after the call.  On an error status both sides must stop with the same status.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../integration/hdpm_chain.hpp"

extern "C" {
typedef struct {
  int verbose, m, iterations, L, burnin, t, r;
  int neal8, split_merge, n8_step_size, sam_step_size, thinning;
  int fast;
} orc_chain_params;
int orc_run_markov_chain_trace(const double* data_colmajor, int n, int d, const int* attrisize, double gamma,
                               const double* v, const double* w, const orc_chain_params* p, const int* c_i_init,
                               int32_t* rng_state, int* out_total_cls, int* out_c_i, double* out_loglik,
                               int* out_accepted, int* final_ass, int* out_moves, int* out_k_all,
                               double* out_centers, double* out_sigmas, int64_t trace_rows_cap);
void orc_ffi_set_seed(uint32_t seed, int32_t* state);
}

template <class T>
static bool rd(FILE* f, T* p, size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: adapter_replay spec.bin\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0, d = 0;
  double gamma = 0;
  if (!rd(f, &n, 1) || !rd(f, &d, 1) || !rd(f, &gamma, 1)) return 2;
  std::vector<int32_t> att(d);
  std::vector<double> v(d), w(d), data((size_t)n * d);
  uint32_t seed = 0;
  int32_t ncalls = 0;
  if (!rd(f, att.data(), d) || !rd(f, v.data(), d) || !rd(f, w.data(), d) || !rd(f, data.data(), data.size()) ||
      !rd(f, &seed, 1) || !rd(f, &ncalls, 1))
    return 2;
  int bad = 0;
  // the adapter rejects a data matrix whose doubles are not integer levels 1..m_j before any
  // narrowing cast (hdpm_chain.hpp), with HDPM_E_ARG and the stream untouched
  {
    const double poison[] = {1.5, 257.0, 0.0, -1.0, NAN, (double)att[0] + 1.0};
    for (double x : poison) {
      std::vector<double> bad_data = data;
      bad_data[(size_t)(n / 2)] = x;   // column 0, row n / 2
      std::vector<int32_t> st(625);
      orc_ffi_set_seed(seed, st.data());
      const std::vector<int32_t> st0 = st;
      hdpm_chain_params p0{};
      p0.m = 3; p0.iterations = 1; p0.L = 2; p0.neal8 = 1; p0.n8_step_size = 1; p0.sam_step_size = 1; p0.thinning = 1;
      hdpm_adapter::ChainResult res;
      std::string err;
      const int se = hdpm_adapter::run_markov_chain(bad_data.data(), n, d, att.data(), gamma, v.data(), w.data(), p0,
                                                    nullptr, st.data(), &res, &err);
      const bool ok = se == HDPM_E_ARG && st == st0 && !err.empty();
      std::printf("poisoned data %g: status %d (%s), %s\n", x, se, err.c_str(), ok ? "rejected" : "MISMATCH");
      bad += !ok;
    }
  }
  std::vector<int32_t> st_eng(625), st_orc(625);
  orc_ffi_set_seed(seed, st_eng.data());
  st_orc = st_eng;
  for (int call = 0; call < ncalls; ++call) {
    int32_t pr[12], has_init = 0;
    if (!rd(f, pr, 12) || !rd(f, &has_init, 1)) return 2;
    std::vector<int32_t> init;
    if (has_init) {
      init.resize(n);
      if (!rd(f, init.data(), n)) return 2;
    }
    hdpm_chain_params p;
    std::memcpy(&p, pr, sizeof(pr));
    orc_chain_params op = {pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6], pr[7], pr[8], pr[9], pr[10], pr[11], 1};
    const int it = p.iterations;
    std::vector<int> tot(it), cis((size_t)it * n), acc(it), fin(n);
    std::vector<double> ll(it);
    // every saved iteration's K x d centers and sigmas, appended row-wise (K <= n + 2)
    const int64_t cap = (int64_t)it * (n + 2);
    std::vector<double> ocen((size_t)cap * d), osig((size_t)cap * d);
    const int so = orc_run_markov_chain_trace(data.data(), n, d, att.data(), gamma, v.data(), w.data(), &op,
                                              has_init ? init.data() : nullptr, st_orc.data(), tot.data(),
                                              cis.data(), ll.data(), acc.data(), fin.data(), nullptr, nullptr,
                                              ocen.data(), osig.data(), cap);
    hdpm_adapter::ChainResult res;
    std::string err;
    const auto wall0 = std::chrono::steady_clock::now();
    const int se = hdpm_adapter::run_markov_chain(data.data(), n, d, att.data(), gamma, v.data(), w.data(), p,
                                                  has_init ? init.data() : nullptr, st_eng.data(), &res, &err);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
    std::string why;
    if (so != se) {
      why = "status oracle " + std::to_string(so) + " engine " + std::to_string(se) + " (" + err + ")";
    } else if (so == 0) {
      size_t row = 0;                    // of saved iteration a in ocen / osig
      for (int a = 0; a < it && why.empty(); row += (size_t)tot[a], ++a) {
        if (res.total_cls[a] != tot[a]) why = "total_cls at " + std::to_string(a);
        else if (std::memcmp(res.c_i[a].data(), &cis[(size_t)a * n], (size_t)n * 4) != 0) why = "c_i at " + std::to_string(a);
        else if (res.accepted[a] != acc[a]) why = "accepted at " + std::to_string(a);
        else if (!(std::fabs(res.loglikelihood[a] - ll[a]) <= 1e-10 * std::fabs(ll[a])))
          why = "loglikelihood at " + std::to_string(a);
        else if (res.centers[a].size() != (size_t)tot[a] * d || res.sigmas[a].size() != (size_t)tot[a] * d)
          why = "centers / sigmas shape at " + std::to_string(a);
        else if (std::memcmp(res.centers[a].data(), &ocen[row * d], (size_t)tot[a] * d * 8) != 0)
          why = "centers at " + std::to_string(a);
        else if (std::memcmp(res.sigmas[a].data(), &osig[row * d], (size_t)tot[a] * d * 8) != 0)
          why = "sigmas at " + std::to_string(a);
      }
      if (why.empty() && std::memcmp(res.final_ass.data(), fin.data(), (size_t)n * 4) != 0) why = "final_ass";
      if (why.empty() && st_eng != st_orc) why = "random stream after the call";
      // la:79: `time` covers the iterations only (the clock starts after init_chain)
      if (why.empty() && !(res.time_s >= 0.0 && res.time_s <= wall)) why = "time outside the call";
    }
    std::printf("call %d: status %d, %s\n", call, so, why.empty() ? "match" : ("MISMATCH " + why).c_str());
    bad += !why.empty();
    if (so != 0 && so == se) {
      // the reference stops at the failing draw; the engine's stream position after an error
      // is not specified: later calls restart from a fresh seed
      orc_ffi_set_seed(seed + 1000u + (uint32_t)call, st_eng.data());
      st_orc = st_eng;
    }
  }
  std::fclose(f);
  return bad ? 1 : 0;
}
