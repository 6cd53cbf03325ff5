// summary_host.cpp -- host side of the posterior summaries (summary_host.hpp): the dense
// psm of posterior.hip, the matrix-free summaries of trace_summary.hip, the uncertainty
// calls of trace_uncertainty.hip, the single-point moves of trace_refine.hip (their descent
// rule is in trace_refine.hpp), the pair merges of trace_merge.hip (their rules are in
// trace_merge.hpp), the average-linkage search of trace_tree.hpp and the
// posterior predictive of predict.hip with the class profiles of profile.hip.  The arithmetic
// that turns the device's integer sums into losses is in trace_loss.hpp, that of the
// predictive's tables and checks in predict_host.hpp, the profiles' checks and cuts in
// profile_host.hpp.
#include "summary_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "../../include/hdpm.h"
#include "predict_host.hpp"
#include "profile_host.hpp"
#include "summary_launch.hpp"
#include "trace_loss.hpp"
#include "trace_merge.hpp"
#include "trace_refine.hpp"
#include "trace_tree.hpp"

namespace hdpm {

constexpr size_t kTraceBudget = (size_t)256 << 20;      // default table bytes per block of candidates
constexpr size_t kTraceStageWords = (size_t)16 << 20;   // labels uploaded per block of draws (64 MB)

// ---- the dense psm (posterior.hip)
int Summaries::psm_build(const int32_t* c_trace, int32_t M, int32_t N) {
  if (!c_trace || M <= 0 || N <= 0) return HDPM_E_ARG;
  if (tl_label_max(c_trace, (int64_t)M * N) < 0) { err = "psm: labels must be in 0..254"; return HDPM_E_ARG; }
  const int Mp = (M + 15) & ~15;
  d_psm_trace.ensure((size_t)M * N);
  d_psm_lab.ensure((size_t)N * Mp);
  d_psm_cnt.ensure((size_t)N * N);
  HIPCHK(hipMemcpyAsync(d_psm_trace.p, c_trace, (size_t)M * N * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(launch_psm(d_psm_trace.p, M, N, d_psm_lab.p, d_psm_cnt.p, stream));
  HIPCHK(hipStreamSynchronize(stream));
  psm_N = N;
  psm_M = M;
  return HDPM_OK;
}
int Summaries::psm_rows(int32_t row0, int32_t nrows, double* out) {
  const int N = psm_N;
  if (!out || N == 0 || row0 < 0 || nrows < 0 || row0 + nrows > N) return HDPM_E_ARG;
  std::vector<uint32_t> c((size_t)nrows * N);
  HIPCHK(hipMemcpyAsync(c.data(), d_psm_cnt.p + (size_t)row0 * N, c.size() * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  const double M = (double)psm_M;
  for (size_t q = 0; q < c.size(); ++q) out[q] = (double)c[q] / M;
  return HDPM_OK;
}
int Summaries::psm_vi_lb(const int32_t* cls, int32_t ncand, double* out) {
  const int N = psm_N;
  if (!cls || !out || N == 0 || ncand <= 0) return HDPM_E_ARG;
  d_psm_cls.ensure((size_t)ncand * N);
  d_psm_all.ensure((size_t)N);
  d_psm_same.ensure((size_t)ncand * N);
  HIPCHK(hipMemcpyAsync(d_psm_cls.p, cls, (size_t)ncand * N * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(launch_vi_terms(d_psm_cnt.p, N, psm_M, d_psm_cls.p, ncand, d_psm_all.p, d_psm_same.p, stream));
  std::vector<double> all((size_t)N);
  std::vector<double> same((size_t)ncand * N);
  HIPCHK(hipMemcpyAsync(all.data(), d_psm_all.p, all.size() * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(same.data(), d_psm_same.p, same.size() * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  std::vector<int> sz;
  for (int c = 0; c < ncand; ++c) {
    const int32_t* cl = cls + (size_t)c * N;
    int mx = 0;
    for (int i = 0; i < N; ++i) mx = std::max(mx, cl[i]);
    sz.assign((size_t)mx + 1, 0);
    for (int i = 0; i < N; ++i) {
      if (cl[i] < 0) { err = "psm: negative cluster label"; return HDPM_E_ARG; }
      sz[cl[i]]++;
    }
    double f = 0.0;
    for (int i = 0; i < N; ++i)
      f = f + tl_vi_lb_term(std::log2((double)sz[cl[i]]), std::log2(all[i]), std::log2(same[(size_t)c * N + i]), N);
    out[c] = f;
  }
  return HDPM_OK;
}

// ---- matrix-free posterior summary (trace_summary.hip): shared by the trace_* calls
// what a call needs to have been made before it
int Summaries::need(bool groups, bool tree) {
  if (tr_N == 0) { err = "trace: hdpm_trace_build has not been called"; return HDPM_E_ARG; }
  if (groups && tg_U == 0) { err = "trace: hdpm_trace_groups has not been called"; return HDPM_E_ARG; }
  if (tree && !tg_tree) { err = "trace: hdpm_trace_avg_tree has not been called"; return HDPM_E_ARG; }
  return HDPM_OK;
}

// the candidates' labels checked (0..254); *Ka = the largest cluster count among them
int Summaries::check(const int32_t* cls, int ncand, int* Ka) {
  if (int st = need(false, false)) return st;
  if (!cls || ncand <= 0) { err = "trace: no candidate partitions"; return HDPM_E_ARG; }
  const int mx = tl_label_max(cls, (int64_t)ncand * tr_N);
  if (mx < 0) { err = "trace: candidate labels must be in 0..254"; return HDPM_E_ARG; }
  *Ka = mx + 1;
  return HDPM_OK;
}

// A set of candidate partitions: of the points (cls: count x N labels, rows of Np bytes
// against the label bytes of the draws) or, with cls == nullptr, the cuts of the tree into
// k0, k0 + 1, ... clusters (one label per group of equal label columns, rows of Up bytes
// against the groups' signatures, weighted by the groups' sizes).
struct Summaries::Cands {
  const int32_t* cls;
  int k0, count;
};

// The candidates in blocks of at most budget / (M x Ka x Kz x 4) (and kTraceMaxBlock): their
// tables, then the per-entry sums (terms; `all` with the first block if want_all) and the
// per-candidate reductions (reduce); f(c0, nc, rows) runs with the block's results on the
// device and the block's label bytes in rows.  A candidate's results do not depend on the
// block it falls in.
template <class F>
void Summaries::blocks(Cands cd, int Ka, bool terms, bool want_all, bool reduce, F f) {
  const bool cuts = !cd.cls;
  const int M = tr_M, Kz = tr_Kz, n = cuts ? tg_U : tr_N, width = cuts ? tg_Up : tr_Np;
  DevBuf<uint8_t>& d_rows = cuts ? d_tg_cut : d_tr_cls;
  DevBuf<uint64_t>& d_all = cuts ? d_tg_all : d_tr_all;
  DevBuf<uint64_t>& d_same = cuts ? d_tg_same : d_tr_same;
  if (!cuts && want_all && !terms && !reduce) {
    // `all` alone needs the draws' sizes only: no tables, no candidate on the device; the
    // gather runs its sizes row (candidate count 0) and f sees an empty first block
    d_tr_all.ensure((size_t)tr_N);
    HIPCHK(launch_tr_gather(d_tr_lab.p, nullptr, tr_N, tr_Np, M, 0, Ka, Kz, nullptr, d_tr_sizes.p, d_tr_all.p, nullptr,
                            stream));
    HIPCHK(hipStreamSynchronize(stream));
    f(0, 0, nullptr);
    return;
  }
  const size_t per = (size_t)M * Ka * Kz;
  const size_t cb = tl_block(tr_budget, per, (size_t)cd.count);
  d_rows.ensure(cb * width);
  d_tr_tab.ensure(cb * per);
  if (terms) d_same.ensure(cb * n);
  if (want_all) d_all.ensure((size_t)n);
  if (reduce) {
    d_tr_q1.ensure(cb * M);
    d_tr_l1.ensure(cb * M);
    d_tr_q.ensure(cb);
    d_tr_l.ensure(cb);
  }
  std::vector<uint8_t> bytes(cb * width);
  std::vector<int32_t> cut(cuts ? (size_t)n : 0);
  for (int c0 = 0; c0 < cd.count; c0 += (int)cb) {
    const int nc = std::min((int)cb, cd.count - c0);
    std::memset(bytes.data(), 0xFF, bytes.size());
    for (int c = 0; c < nc; ++c) {
      if (cuts) tt_cut(n, tg_merge.data(), cd.k0 + c0 + c, cut.data());
      const int32_t* cl = cuts ? cut.data() : cd.cls + (size_t)(c0 + c) * n;
      uint8_t* row = bytes.data() + (size_t)c * width;
      for (int i = 0; i < n; ++i) row[i] = (uint8_t)cl[i];
    }
    HIPCHK(hipMemcpyAsync(d_rows.p, bytes.data(), (size_t)nc * width, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(d_tr_tab.p, 0, (size_t)nc * per * 4, stream));
    uint64_t* all = want_all && c0 == 0 ? d_all.p : nullptr;
    if (cuts) {
      HIPCHK(launch_tg_tables(d_tg_sigT.p, d_rows.p, d_tg_w.p, n, width, M, nc, Ka, Kz, d_tr_tab.p, stream));
      if (terms)
        HIPCHK(launch_tg_gather(d_tg_sigT.p, d_rows.p, n, width, M, nc, Ka, Kz, d_tr_tab.p, d_tr_sizes.p, all,
                                d_same.p, stream));
    } else {
      HIPCHK(launch_tr_tables(d_tr_lab.p, d_rows.p, width, M, nc, Ka, Kz, d_tr_tab.p, stream));
      if (terms)
        HIPCHK(launch_tr_gather(d_tr_lab.p, d_rows.p, n, width, M, nc, Ka, Kz, d_tr_tab.p, d_tr_sizes.p, all,
                                d_same.p, stream));
    }
    if (reduce) HIPCHK(launch_tr_reduce(d_tr_tab.p, nc, M, Ka * Kz, d_tr_q1.p, d_tr_l1.p, d_tr_q.p, d_tr_l.p, stream));
    // the point candidates' f finds the stream drained; the cuts' f queues its copies behind
    // the block and waits once
    if (!cuts) HIPCHK(hipStreamSynchronize(stream));
    f(c0, nc, bytes.data());
  }
}

// The losses of a set of candidates (trace_losses, trace_cut_losses).  VI.lb sums one term
// per point: over the points in double and index order (the terms on the host's threads,
// as psm_vi_lb sums them), over the groups weighted by their sizes in long double (the few
// groups' terms on the calling thread).
void Summaries::losses(Cands cd, int Ka, double* vi_lb, double* vi, uint64_t* binder_A, uint64_t* binder_Q) {
  const bool cuts = !cd.cls, terms = vi_lb != nullptr, reduce = vi || binder_Q;
  const int N = tr_N, n = cuts ? tg_U : N, width = cuts ? tg_Up : tr_Np;
  const double dM = (double)tr_M;
  std::vector<uint64_t> all, same, q, sz((size_t)Ka);
  std::vector<double> l, lall, term, lsz((size_t)Ka);
  auto each = [&](auto body) {
    if (cuts) body(0, n);
    else parallel_for(n, body);
  };
  blocks(cd, Ka, terms, terms, reduce, [&](int c0, int nc, const uint8_t* rows) {
    if (terms) {
      if (c0 == 0) {
        all.resize((size_t)n);
        HIPCHK(hipMemcpyAsync(all.data(), (cuts ? d_tg_all : d_tr_all).p, (size_t)n * 8, hipMemcpyDeviceToHost,
                              stream));
      }
      same.resize((size_t)nc * n);
      HIPCHK(hipMemcpyAsync(same.data(), (cuts ? d_tg_same : d_tr_same).p, same.size() * 8, hipMemcpyDeviceToHost,
                            stream));
    }
    if (reduce) {
      q.resize((size_t)nc);
      l.resize((size_t)nc);
      HIPCHK(hipMemcpyAsync(q.data(), d_tr_q.p, (size_t)nc * 8, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(l.data(), d_tr_l.p, (size_t)nc * 8, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    if (terms && c0 == 0) {
      // log2 sum_j psm_ij is the same for every candidate
      lall.resize((size_t)n);
      term.resize((size_t)n);
      each([&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) lall[i] = std::log2((double)all[i] / dM);
      });
    }
    for (int c = 0; c < nc; ++c) {
      const uint8_t* cl = rows + (size_t)c * width;
      std::fill(sz.begin(), sz.end(), 0);
      for (int i = 0; i < n; ++i) sz[cl[i]] += cuts ? tg_w[i] : 1;
      const TlSizes s = tl_sizes(sz.data(), Ka, lsz.data());
      if (terms) {
        // the expression of psm_vi_lb, with psm sums = integer sums / M
        const uint64_t* sm = same.data() + (size_t)c * n;
        each([&](int64_t i0, int64_t i1) {
          for (int64_t i = i0; i < i1; ++i)
            term[i] = tl_vi_lb_term(lsz[cl[i]], lall[i], std::log2((double)sm[i] / dM), N);
        });
        double f = 0.0;
        long double fw = 0.0L;
        if (cuts) for (int i = 0; i < n; ++i) fw += (long double)tg_w[i] * (long double)term[i];
        else for (int i = 0; i < n; ++i) f = f + term[i];
        vi_lb[c0 + c] = cuts ? (double)fw : f;
      }
      if (vi) vi[c0 + c] = tl_vi(s.hc, tr_S, l[c], dM, N);
      if (binder_A) binder_A[c0 + c] = s.A;
      if (binder_Q) binder_Q[c0 + c] = q[c];
    }
  });
}

int Summaries::trace_build(const int32_t* c_trace, int32_t M, int32_t N, int64_t table_budget_bytes) {
  if (!c_trace || M <= 0 || N <= 0 || table_budget_bytes < 0) { err = "trace: bad arguments"; return HDPM_E_ARG; }
  const int mx = tl_label_max(c_trace, (int64_t)M * N);
  if (mx < 0) { err = "trace: labels must be in 0..254"; return HDPM_E_ARG; }
  tr_N = 0;   // no trace until this one is complete
  tg_U = 0;   // and no groups or tree of the previous one
  pr_d = 0;   // nor its draws' parameters
  tg_counts = tg_tree = false;
  const int Np = (int)(((int64_t)N + 15) & ~(int64_t)15);
  d_tr_lab.ensure((size_t)M * Np);
  d_tr_sizes.ensure((size_t)M * 256);
  d_tr_q1.ensure((size_t)M);
  d_tr_l1.ensure((size_t)M);
  d_tr_q.ensure(1);
  d_tr_l.ensure(1);
  {
    // the int32 labels go up in blocks of draws through one staging buffer, freed at the end
    const int mb = (int)std::min<size_t>((size_t)M, std::max<size_t>(1, kTraceStageWords / (size_t)N));
    DevBuf<int32_t> stage;
    stage.ensure((size_t)mb * N);
    for (int m0 = 0; m0 < M; m0 += mb) {
      const int nm = std::min(mb, M - m0);
      HIPCHK(hipMemcpyAsync(stage.p, c_trace + (size_t)m0 * N, (size_t)nm * N * 4, hipMemcpyHostToDevice, stream));
      HIPCHK(launch_tr_pack(stage.p, nm, N, Np, d_tr_lab.p + (size_t)m0 * Np, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
  }
  HIPCHK(hipMemsetAsync(d_tr_sizes.p, 0, (size_t)M * 256 * 4, stream));
  HIPCHK(launch_tr_sizes(d_tr_lab.p, Np, M, d_tr_sizes.p, stream));
  HIPCHK(launch_tr_reduce(d_tr_sizes.p, 1, M, 256, d_tr_q1.p, d_tr_l1.p, d_tr_q.p, d_tr_l.p, stream));
  HIPCHK(hipMemcpyAsync(&tr_P, d_tr_q.p, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(&tr_S, d_tr_l.p, 8, hipMemcpyDeviceToHost, stream));
  // the per-draw P_m and S_m stay on the host (later calls reuse d_tr_q1 / d_tr_l1), with
  // the draws' cluster counts from the size rows
  tr_Pm.resize((size_t)M);
  tr_Sm.resize((size_t)M);
  tr_Km.assign((size_t)M, 0);
  std::vector<uint32_t> sizes((size_t)M * 256);
  HIPCHK(hipMemcpyAsync(tr_Pm.data(), d_tr_q1.p, (size_t)M * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(tr_Sm.data(), d_tr_l1.p, (size_t)M * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(sizes.data(), d_tr_sizes.p, sizes.size() * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (int m = 0; m < M; ++m)
    for (int b = 0; b < 256; ++b) tr_Km[m] += sizes[(size_t)m * 256 + b] != 0u;
  tr_M = M;
  tr_Np = Np;
  tr_Kz = mx + 1;
  tr_budget = table_budget_bytes > 0 ? (size_t)table_budget_bytes : kTraceBudget;
  tr_N = N;
  return HDPM_OK;
}
int Summaries::trace_terms(const int32_t* cls, int32_t ncand, uint64_t* all, uint64_t* same) {
  int Ka = 0;
  if (int st = check(cls, ncand, &Ka)) return st;
  if (!all && !same) return HDPM_OK;
  const size_t N = (size_t)tr_N;
  blocks({cls, 0, ncand}, Ka, same != nullptr, all != nullptr, false, [&](int c0, int nc, const uint8_t*) {
    if (all && c0 == 0) HIPCHK(hipMemcpyAsync(all, d_tr_all.p, N * 8, hipMemcpyDeviceToHost, stream));
    if (same)
      HIPCHK(hipMemcpyAsync(same + (size_t)c0 * N, d_tr_same.p, (size_t)nc * N * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  });
  return HDPM_OK;
}
int Summaries::trace_losses(const int32_t* cls, int32_t ncand, double* vi_lb, double* vi, uint64_t* binder_Q,
                            uint64_t* binder_P) {
  int Ka = 0;
  if (int st = check(cls, ncand, &Ka)) return st;
  if (binder_P) *binder_P = tr_P;
  if (vi_lb || vi || binder_Q) losses({cls, 0, ncand}, Ka, vi_lb, vi, nullptr, binder_Q);
  return HDPM_OK;
}
int Summaries::trace_tables(const int32_t* cls, int32_t ncand, int32_t m0, int32_t nm, uint32_t* out) {
  int Ka = 0;
  if (int st = check(cls, ncand, &Ka)) return st;
  if (!out || m0 < 0 || nm <= 0 || (int64_t)m0 + nm > tr_M) {
    err = "trace: draws m0 .. m0 + nm - 1 must lie in 0 .. M - 1";
    return HDPM_E_ARG;
  }
  const int M = tr_M, Kz = tr_Kz;
  const size_t cells = (size_t)Ka * Kz;
  std::memset(out, 0, (size_t)ncand * nm * 65536 * 4);
  std::vector<uint32_t> t((size_t)nm * cells);
  blocks({cls, 0, ncand}, Ka, false, false, false, [&](int c0, int nc, const uint8_t*) {
    for (int c = 0; c < nc; ++c) {
      HIPCHK(hipMemcpyAsync(t.data(), d_tr_tab.p + ((size_t)c * M + m0) * cells, t.size() * 4, hipMemcpyDeviceToHost,
                            stream));
      HIPCHK(hipStreamSynchronize(stream));
      for (int m = 0; m < nm; ++m)
        for (int a = 0; a < Ka; ++a)
          std::memcpy(out + (((size_t)(c0 + c) * nm + m) * 256 + a) * 256, t.data() + ((size_t)m * Ka + a) * Kz,
                      (size_t)Kz * 4);
    }
  });
  return HDPM_OK;
}

// ---- how far the estimate can be trusted (trace_uncertainty.hip)
int Summaries::trace_distances(const int32_t* cls, int32_t ncand, double* vi, uint64_t* binder, int32_t* draw_k) {
  int Ka = 0;
  if (int st = check(cls, ncand, &Ka)) return st;
  const int N = tr_N, M = tr_M;
  if (draw_k) std::memcpy(draw_k, tr_Km.data(), (size_t)M * 4);
  if (!vi && !binder) return HDPM_OK;
  std::vector<uint64_t> q1, sz((size_t)Ka);
  std::vector<double> l1, lsz((size_t)Ka);
  // the per-(candidate, draw) sums of k_tr_reduce, as they stand before k_tr_reduce_draws
  blocks({cls, 0, ncand}, Ka, false, false, true, [&](int c0, int nc, const uint8_t* rows) {
    q1.resize((size_t)nc * M);
    l1.resize((size_t)nc * M);
    HIPCHK(hipMemcpyAsync(q1.data(), d_tr_q1.p, q1.size() * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(l1.data(), d_tr_l1.p, l1.size() * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int c = 0; c < nc; ++c) {
      const uint8_t* cl = rows + (size_t)c * tr_Np;
      std::fill(sz.begin(), sz.end(), 0);
      for (int i = 0; i < N; ++i) sz[cl[i]]++;
      const TlSizes s = tl_sizes(sz.data(), Ka, lsz.data());
      for (int m = 0; m < M; ++m) {
        const size_t o = (size_t)(c0 + c) * M + m, k = (size_t)c * M + m;
        if (vi) vi[o] = tl_vi_draw(s.hc, tr_Sm[m], l1[k], N);
        if (binder) binder[o] = s.A + tr_Pm[m] - 2 * q1[k];
      }
    }
  });
  return HDPM_OK;
}
int Summaries::trace_affinity(const int32_t* cl, int32_t Ka, uint64_t* aff, uint64_t* cross) {
  int used = 0;   // the largest label + 1
  if (int st = check(cl, 1, &used)) return st;
  if (Ka < 1 || Ka > 255) { err = "trace: Ka must be in 1..255"; return HDPM_E_ARG; }
  if (used > Ka) { err = "trace: the partition's labels must be in 0..Ka-1"; return HDPM_E_ARG; }
  const int N = tr_N, Np = tr_Np, M = tr_M, Kz = tr_Kz;
  if (cross && !tl_fits63((uint64_t)N, (uint64_t)M)) {
    err = "trace: N^2 M does not fit 63 bits: the sums of cross would overflow";
    return HDPM_E_ARG;
  }
  if (!aff && !cross) return HDPM_OK;
  // one candidate always fits a block: its tables, then their transpose
  blocks({cl, 0, 1}, Ka, false, false, false, [&](int, int, const uint8_t*) {
    const size_t per = (size_t)M * Ka * Kz;
    d_tr_tabT.ensure(per);
    HIPCHK(launch_tr_transpose(d_tr_tab.p, M, Ka, Kz, d_tr_tabT.p, stream));
    if (cross) {
      d_tr_cross.ensure((size_t)Ka * Ka);
      HIPCHK(hipMemsetAsync(d_tr_cross.p, 0, (size_t)Ka * Ka * 8, stream));
      HIPCHK(launch_tr_cross(d_tr_tabT.p, M, Ka, Kz, d_tr_cross.p, stream));
      HIPCHK(hipMemcpyAsync(cross, d_tr_cross.p, (size_t)Ka * Ka * 8, hipMemcpyDeviceToHost, stream));
    }
    if (aff) {
      // blocks of points: the staging (pb x Ka x 8 bytes) within the table budget, in whole
      // groups of 16 points and at least one; each block goes to the caller as it completes
      size_t pb = (tr_budget / ((size_t)Ka * 8)) & ~(size_t)15;
      pb = std::min(std::max<size_t>(pb, 16), (size_t)Np);
      d_tr_aff.ensure(pb * Ka);
      for (int64_t i0 = 0; i0 < N; i0 += (int64_t)pb) {
        const int np = (int)std::min<int64_t>((int64_t)pb, N - i0);
        HIPCHK(launch_tr_affinity(d_tr_lab.p, Np, M, Ka, Kz, d_tr_tabT.p, (int)i0, np, d_tr_aff.p, stream));
        HIPCHK(hipMemcpyAsync(aff + (size_t)i0 * Ka, d_tr_aff.p, (size_t)np * Ka * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
      }
    }
    HIPCHK(hipStreamSynchronize(stream));
  });
  return HDPM_OK;
}

// ---- a point estimate refined by single-point moves (trace_refine.hip, trace_refine.hpp)
// cl checked, labels 0..Ka-1: the tables of the one candidate, their transposed form for the
// loss, then blocks of points: sums, gains and argmin on the device, best / gain (and the
// full rows on request) to the caller as each block completes
void Summaries::move_gains(const int32_t* cl, int Ka, int loss, int32_t* best, double* gain, double* full) {
  const int N = tr_N, Np = tr_Np, M = tr_M, Kz = tr_Kz, L = Ka + 1;
  blocks({cl, 0, 1}, Ka, false, false, false, [&](int, int, const uint8_t* rows) {
    const size_t per = (size_t)M * Ka * Kz;
    std::vector<uint64_t> sz((size_t)L, 0);
    for (int i = 0; i < N; ++i) sz[rows[i]]++;
    std::vector<double> ct((size_t)L + Ka, 0.0);
    for (int b = 0; b < L; ++b) ct[b] = loss == HDPM_LOSS_VI ? rf_h((double)sz[b]) : (double)sz[b];
    if (loss == HDPM_LOSS_VI)
      for (int a = 0; a < Ka; ++a) ct[L + a] = sz[a] > 0 ? rf_h((double)(sz[a] - 1)) : 0.0;
    d_rf_ct.ensure(ct.size());
    HIPCHK(hipMemcpyAsync(d_rf_ct.p, ct.data(), ct.size() * 8, hipMemcpyHostToDevice, stream));
    const void* tabT;
    if (loss == HDPM_LOSS_VI) {
      d_rf_h.ensure(per * 2);
      HIPCHK(launch_rf_htable(d_tr_tab.p, M, Ka, Kz, d_rf_h.p, stream));
      tabT = d_rf_h.p;
    } else {
      d_tr_tabT.ensure(per);
      HIPCHK(launch_tr_transpose(d_tr_tab.p, M, Ka, Kz, d_tr_tabT.p, stream));
      tabT = d_tr_tabT.p;
    }
    // blocks of points: the staging (pb x (Ka + 1) x 8 bytes) within the table budget, in
    // whole groups of 16 points and at least one (trace_affinity's rule)
    size_t pb = (tr_budget / ((size_t)L * 8)) & ~(size_t)15;
    pb = std::min(std::max<size_t>(pb, 16), (size_t)Np);
    d_rf_stage.ensure(pb * L);
    d_rf_best.ensure(pb);
    d_rf_gain.ensure(pb);
    for (int64_t i0 = 0; i0 < N; i0 += (int64_t)pb) {
      const int np = (int)std::min<int64_t>((int64_t)pb, N - i0);
      HIPCHK(launch_rf_gains(loss, d_tr_lab.p, d_tr_cls.p, Np, M, Ka, Kz, tabT, (int)i0, np, d_rf_ct.p, N,
                             full ? 1 : 0, d_rf_stage.p, d_rf_best.p, d_rf_gain.p, stream));
      if (best) HIPCHK(hipMemcpyAsync(best + i0, d_rf_best.p, (size_t)np * 4, hipMemcpyDeviceToHost, stream));
      if (gain) HIPCHK(hipMemcpyAsync(gain + i0, d_rf_gain.p, (size_t)np * 8, hipMemcpyDeviceToHost, stream));
      if (full)
        HIPCHK(hipMemcpyAsync(full + (size_t)i0 * L, d_rf_stage.p, (size_t)np * L * 8, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
  });
}
int Summaries::trace_move_gains(const int32_t* cl, int32_t Ka, int32_t loss, int32_t* best, double* gain,
                                double* full) {
  int used = 0;   // the largest label + 1
  if (int st = check(cl, 1, &used)) return st;
  if (Ka < 1 || Ka > 255) { err = "trace: Ka must be in 1..255"; return HDPM_E_ARG; }
  if (used > Ka) { err = "trace: the partition's labels must be in 0..Ka-1"; return HDPM_E_ARG; }
  if (loss != HDPM_LOSS_VI && loss != HDPM_LOSS_BINDER) { err = "trace: unknown loss"; return HDPM_E_ARG; }
  if (best || gain || full) move_gains(cl, Ka, loss, best, gain, full);
  return HDPM_OK;
}
// the loss of one partition (labels 0..K-1) as the descents compare it: hdpm_trace_losses' vi,
// and Binder's integer M A + P - 2 Q
double Summaries::vi_of(const int32_t* c, int K) {
  double v = 0.0;
  losses({c, 0, 1}, K, nullptr, &v, nullptr, nullptr);
  return v;
}
uint64_t Summaries::binder_of(const int32_t* c, int K) {
  uint64_t A = 0, Q = 0;
  losses({c, 0, 1}, K, nullptr, nullptr, &A, &Q);
  return (uint64_t)tr_M * A + tr_P - 2 * Q;
}
static void rf_export(const RfInfo& r, hdpm_refine_info* info) {
  info->rounds = r.rounds;
  info->trials = r.trials;
  info->converged = r.converged;
  info->K = r.K;
  info->moved = r.moved;
  info->start = r.start;
  info->value = r.value;
}
int Summaries::trace_refine(const int32_t* cl, int32_t loss, int32_t max_rounds, int32_t* cl_out,
                            hdpm_refine_info* info, double* history) {
  int used = 0;
  if (int st = check(cl, 1, &used)) return st;
  if (loss != HDPM_LOSS_VI && loss != HDPM_LOSS_BINDER) { err = "trace: unknown loss"; return HDPM_E_ARG; }
  if (max_rounds < 0 || !cl_out) { err = "trace: refine needs max_rounds >= 0 and cl_out"; return HDPM_E_ARG; }
  if (loss == HDPM_LOSS_BINDER && !tl_fits63((uint64_t)tr_N, (uint64_t)tr_M)) {
    err = "trace: N^2 M does not fit 63 bits: Binder's integer would overflow";
    return HDPM_E_ARG;
  }
  auto gains = [&](const int32_t* c, int K, int32_t* best, double* gain) {
    move_gains(c, K, loss, best, gain, nullptr);
  };
  RfInfo r;
  if (loss == HDPM_LOSS_VI) {
    rf_run<double>(cl, tr_N, max_rounds, gains, [&](const int32_t* c, int K) { return vi_of(c, K); }, cl_out, &r,
                   history);
  } else {
    rf_run<uint64_t>(cl, tr_N, max_rounds, gains, [&](const int32_t* c, int K) { return binder_of(c, K); }, cl_out,
                     &r, history);
  }
  if (info) rf_export(r, info);
  return HDPM_OK;
}

// ---- pair merges (trace_merge.hip, trace_merge.hpp)
// what hdpm_trace_affinity refuses, an unknown loss, and Binder's 63-bit bound
int Summaries::check_one(const int32_t* cl, int32_t Ka, int32_t loss) {
  int used = 0;   // the largest label + 1
  if (int st = check(cl, 1, &used)) return st;
  if (Ka < 1 || Ka > 255) { err = "trace: Ka must be in 1..255"; return HDPM_E_ARG; }
  if (used > Ka) { err = "trace: the partition's labels must be in 0..Ka-1"; return HDPM_E_ARG; }
  if (loss != HDPM_LOSS_VI && loss != HDPM_LOSS_BINDER) { err = "trace: unknown loss"; return HDPM_E_ARG; }
  if (loss == HDPM_LOSS_BINDER && !tl_fits63((uint64_t)tr_N, (uint64_t)tr_M)) {
    err = "trace: N^2 M does not fit 63 bits: Binder's integer would overflow";
    return HDPM_E_ARG;
  }
  return HDPM_OK;
}
// the tables of the one candidate stand in d_tr_tab: their transpose, and the class sizes
void Summaries::merge_setup(const uint8_t* rows, int Ka, std::vector<uint64_t>& sz) {
  sz.assign((size_t)Ka, 0);
  for (int i = 0; i < tr_N; ++i) sz[rows[i]]++;
  d_tr_tabT.ensure((size_t)tr_M * Ka * tr_Kz);
  HIPCHK(launch_tr_transpose(d_tr_tab.p, tr_M, Ka, tr_Kz, d_tr_tabT.p, stream));
}
// the Ka x Ka gains of the tables in d_tr_tabT with class sizes sz, to the host.  only >= 0:
// VI's partial sums of the last call stand, and only the pairs of that class are taken again
void Summaries::merge_gains(int loss, int Ka, int only, const std::vector<uint64_t>& sz, double* gain) {
  const int M = tr_M, Kz = tr_Kz;
  const size_t KK = (size_t)Ka * Ka;
  std::vector<double> n(sz.begin(), sz.end());
  d_mg_n.ensure((size_t)Ka);
  d_mg_gain.ensure(KK);
  HIPCHK(hipMemcpyAsync(d_mg_n.p, n.data(), (size_t)Ka * 8, hipMemcpyHostToDevice, stream));
  if (loss == HDPM_LOSS_VI) {
    d_mg_part.ensure((size_t)mg_slices(M) * KK);
    HIPCHK(launch_mg_pairs(d_tr_tabT.p, M, Ka, Kz, only, d_mg_part.p, stream));
  } else {
    d_tr_cross.ensure(KK);
    HIPCHK(hipMemsetAsync(d_tr_cross.p, 0, KK * 8, stream));
    HIPCHK(launch_tr_cross(d_tr_tabT.p, M, Ka, Kz, d_tr_cross.p, stream));
  }
  HIPCHK(launch_mg_gain(loss, d_mg_part.p, d_tr_cross.p, d_mg_n.p, M, Ka, tr_N, d_mg_gain.p, stream));
  HIPCHK(hipMemcpyAsync(gain, d_mg_gain.p, KK * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
}
int Summaries::trace_merge_gains(const int32_t* cl, int32_t Ka, int32_t loss, double* gain, int32_t* best,
                                 double* best_gain) {
  if (int st = check_one(cl, Ka, loss)) return st;
  if (!gain && !best && !best_gain) return HDPM_OK;
  std::vector<double> g((size_t)Ka * Ka);
  std::vector<uint64_t> sz;
  blocks({cl, 0, 1}, Ka, false, false, false, [&](int, int, const uint8_t* rows) {
    merge_setup(rows, Ka, sz);
    merge_gains(loss, Ka, -1, sz, g.data());
  });
  const MgPair p = mg_best(g.data(), sz.data(), Ka);
  if (gain) std::copy(g.begin(), g.end(), gain);
  if (best) { best[0] = p.a; best[1] = p.b; }
  if (best_gain) *best_gain = p.gain;
  return HDPM_OK;
}
int Summaries::trace_merge_path(const int32_t* cl, int32_t Ka, int32_t loss, int32_t k_min, int32_t* merge,
                                double* step_gain, double* value, int32_t* steps) {
  if (int st = check_one(cl, Ka, loss)) return st;
  if (k_min < 1) { err = "trace: merge_path needs k_min >= 1"; return HDPM_E_ARG; }
  const int M = tr_M, N = tr_N, Kz = tr_Kz;
  int nsteps = 0;
  std::vector<uint64_t> sz;
  std::vector<double> lsz((size_t)Ka);
  // one table pass; then folds, pair gains and the reductions of the folded tables
  blocks({cl, 0, 1}, Ka, false, false, false, [&](int, int, const uint8_t* rows) {
    merge_setup(rows, Ka, sz);
    auto loss_now = [&]() {
      uint64_t q = 0;
      double l = 0.0;
      HIPCHK(launch_tr_reduce(d_tr_tab.p, 1, M, Ka * Kz, d_tr_q1.p, d_tr_l1.p, d_tr_q.p, d_tr_l.p, stream));
      HIPCHK(hipMemcpyAsync(&q, d_tr_q.p, 8, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(&l, d_tr_l.p, 8, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      const TlSizes s = tl_sizes(sz.data(), Ka, lsz.data());
      return loss == HDPM_LOSS_VI ? tl_vi(s.hc, tr_S, l, (double)M, N) : (double)((uint64_t)M * s.A + tr_P - 2 * q);
    };
    nsteps = mg_path(
        sz.data(), Ka, k_min, [&](int changed, double* g) { merge_gains(loss, Ka, changed, sz, g); },
        [&](int a, int b) { HIPCHK(launch_mg_fold(d_tr_tab.p, d_tr_tabT.p, M, Ka, Kz, a, b, stream)); }, loss_now, merge,
        step_gain, value);
  });
  if (steps) *steps = nsteps;
  return HDPM_OK;
}
int Summaries::trace_refine_merge(const int32_t* cl, int32_t loss, int32_t max_rounds, int32_t max_merges,
                                  int32_t* cl_out, hdpm_refine_info* info, int32_t* merges, double* history) {
  int used = 0;
  if (int st = check(cl, 1, &used)) return st;
  if (int st = check_one(cl, used, loss)) return st;
  if (max_rounds < 0 || max_merges < 0 || !cl_out) {
    err = "trace: refine_merge needs max_rounds >= 0, max_merges >= 0 and cl_out";
    return HDPM_E_ARG;
  }
  auto gains = [&](const int32_t* c, int K, int32_t* best, double* gain) {
    move_gains(c, K, loss, best, gain, nullptr);
  };
  std::vector<double> g;
  std::vector<uint64_t> sz;
  auto pairs = [&](const int32_t* c, int K) {
    g.resize((size_t)K * K);
    blocks({c, 0, 1}, K, false, false, false, [&](int, int, const uint8_t* rows) {
      merge_setup(rows, K, sz);
      merge_gains(loss, K, -1, sz, g.data());
    });
    return mg_best(g.data(), sz.data(), K);
  };
  RfInfo r;
  if (loss == HDPM_LOSS_VI) {
    mg_run<double>(cl, tr_N, max_rounds, max_merges, gains, [&](const int32_t* c, int K) { return vi_of(c, K); },
                   pairs, cl_out, &r, merges, history);
  } else {
    mg_run<uint64_t>(cl, tr_N, max_rounds, max_merges, gains,
                     [&](const int32_t* c, int K) { return binder_of(c, K); }, pairs, cl_out, &r, merges, history);
  }
  if (info) rf_export(r, info);
  return HDPM_OK;
}

// ---- average-linkage search on the groups of equal label columns (trace_summary.hip k_tg_*,
// trace_tree.hpp)
void Summaries::group_counts() {
  if (tg_counts) return;
  const size_t U = (size_t)tg_U;
  d_tg_S.ensure(U * U);
  HIPCHK(launch_tg_counts(d_tg_sig.p, tg_U, tr_M, tg_Mp, d_tg_S.p, stream));
  HIPCHK(hipStreamSynchronize(stream));
  tg_counts = true;
}
int Summaries::trace_groups(int32_t max_groups, int32_t hash_bits, int32_t* U_out) {
  if (int st = need(false, false)) return st;
  if (max_groups == 0) max_groups = HDPM_TRACE_GROUPS_DEFAULT;
  if (max_groups < 0 || max_groups > HDPM_TRACE_GROUPS_MAX || hash_bits < 0 || hash_bits > 32) {
    err = "trace: max_groups must be in 1.." + std::to_string(HDPM_TRACE_GROUPS_MAX) + " and hash_bits in 0..32";
    return HDPM_E_ARG;
  }
  const int N = tr_N, Np = tr_Np, M = tr_M;
  if (!tl_fits63((uint64_t)N, (uint64_t)M)) {
    err = "trace: N^2 M does not fit 63 bits: the tree's integer sums would overflow";
    return HDPM_E_ARG;
  }
  tg_U = 0;
  tg_counts = tg_tree = false;
  uint32_t T = 1024;
  while (T < 4u * (uint32_t)max_groups) T <<= 1;
  d_tg_rep.ensure(T);
  d_tg_slotfirst.ensure(T);
  d_tg_slotgid.ensure(T);
  d_tg_pslot.ensure((size_t)N);
  d_tg_ctl.ensure(2);
  HIPCHK(hipMemsetAsync(d_tg_rep.p, 0xFF, (size_t)T * 4, stream));
  HIPCHK(hipMemsetAsync(d_tg_slotfirst.p, 0xFF, (size_t)T * 4, stream));
  HIPCHK(hipMemsetAsync(d_tg_ctl.p, 0, 8, stream));
  HIPCHK(launch_tg_insert(d_tr_lab.p, N, Np, M, hash_bits, T, (uint32_t)max_groups, d_tg_rep.p, d_tg_slotfirst.p,
                          d_tg_pslot.p, d_tg_ctl.p, stream));
  uint32_t ctl[2] = {0u, 0u};
  std::vector<uint32_t> sf((size_t)T);
  HIPCHK(hipMemcpyAsync(ctl, d_tg_ctl.p, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(sf.data(), d_tg_slotfirst.p, (size_t)T * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (ctl[1]) {
    err = "trace: more than max_groups = " + std::to_string(max_groups) +
          " distinct label columns: the trace is too unsettled for the average-linkage search";
    return HDPM_E_ARG;
  }
  // the groups numbered by ascending smallest member: whichever slot a column landed in
  std::vector<std::pair<uint32_t, uint32_t>> order;
  for (uint32_t s = 0; s < T; ++s)
    if (sf[s] != 0xFFFFFFFFu) order.emplace_back(sf[s], s);
  std::sort(order.begin(), order.end());
  const int U = (int)order.size();
  if (U == 0 || (uint32_t)U != ctl[0]) { err = "trace: the group table is inconsistent"; return HDPM_E_DEVICE; }
  std::vector<uint32_t> gid((size_t)T, 0u);
  tg_first.resize((size_t)U);
  for (int u = 0; u < U; ++u) {
    tg_first[u] = order[u].first;
    gid[order[u].second] = (uint32_t)u;
  }
  const int Mp = (M + 63) & ~63, Up = (U + 15) & ~15;
  d_tg_of.ensure((size_t)N);
  d_tg_first.ensure((size_t)U);
  d_tg_w.ensure((size_t)U);
  d_tg_sig.ensure((size_t)U * Mp);
  d_tg_sigT.ensure((size_t)M * Up);
  HIPCHK(hipMemcpyAsync(d_tg_slotgid.p, gid.data(), (size_t)T * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_tg_first.p, tg_first.data(), (size_t)U * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(d_tg_w.p, 0, (size_t)U * 4, stream));
  HIPCHK(launch_tg_finish(d_tr_lab.p, N, Np, M, U, Mp, Up, d_tg_pslot.p, d_tg_slotgid.p, d_tg_first.p, d_tg_of.p,
                          d_tg_w.p, d_tg_sig.p, d_tg_sigT.p, stream));
  tg_w.resize((size_t)U);
  HIPCHK(hipMemcpyAsync(tg_w.data(), d_tg_w.p, (size_t)U * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  tg_Mp = Mp;
  tg_Up = Up;
  tg_U = U;
  if (U_out) *U_out = U;
  return HDPM_OK;
}
int Summaries::trace_group_info(int32_t* first, int32_t* weight, int32_t* group_of, uint32_t* counts) {
  if (int st = need(true, false)) return st;
  const size_t U = (size_t)tg_U;
  if (first) std::memcpy(first, tg_first.data(), U * 4);
  if (weight) std::memcpy(weight, tg_w.data(), U * 4);
  if (group_of) HIPCHK(hipMemcpyAsync(group_of, d_tg_of.p, (size_t)tr_N * 4, hipMemcpyDeviceToHost, stream));
  if (counts) {
    group_counts();
    HIPCHK(hipMemcpyAsync(counts, d_tg_S.p, U * U * 4, hipMemcpyDeviceToHost, stream));
  }
  HIPCHK(hipStreamSynchronize(stream));
  return HDPM_OK;
}
int Summaries::trace_avg_tree(int32_t* merge, double* height) {
  if (int st = need(true, false)) return st;
  const size_t U = (size_t)tg_U;
  if (!tg_tree) {
    group_counts();
    std::vector<uint32_t> S(U * U);
    HIPCHK(hipMemcpyAsync(S.data(), d_tg_S.p, U * U * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<uint64_t> w(tg_w.begin(), tg_w.end()), first(tg_first.begin(), tg_first.end());
    tg_merge.assign((U - 1) * 2, 0);
    tg_height.assign(U - 1, 0.0);
    tt_avg_linkage((int)U, w.data(), first.data(), S.data(), (uint64_t)tr_M, tg_merge.data(), tg_height.data());
    tg_tree = true;
  }
  if (merge && U > 1) std::memcpy(merge, tg_merge.data(), (U - 1) * 2 * 4);
  if (height && U > 1) std::memcpy(height, tg_height.data(), (U - 1) * 8);
  return HDPM_OK;
}
int Summaries::trace_cut_losses(int32_t k0, int32_t nk, double* vi_lb, double* vi, uint64_t* binder_A,
                                uint64_t* binder_Q) {
  if (int st = need(true, true)) return st;
  if (k0 < 1 || nk < 1 || (int64_t)k0 + nk - 1 > std::min(tg_U, 255)) {
    err = "trace: cuts k0 .. k0 + nk - 1 must lie in 1 .. min(U, 255)";
    return HDPM_E_ARG;
  }
  if (vi_lb || vi || binder_A || binder_Q) losses({nullptr, k0, nk}, k0 + nk - 1, vi_lb, vi, binder_A, binder_Q);
  return HDPM_OK;
}
int Summaries::trace_cut_labels(int32_t k, int32_t* cl) {
  if (int st = need(true, true)) return st;
  if (!cl || k < 1 || k > tg_U) { err = "trace: the cut k must lie in 1 .. U"; return HDPM_E_ARG; }
  const int N = tr_N, U = tg_U;
  std::vector<int32_t> cut((size_t)U);
  tt_cut(U, tg_merge.data(), k, cut.data());
  d_tg_cutw.ensure((size_t)U);
  d_tg_cl.ensure((size_t)N);
  HIPCHK(hipMemcpyAsync(d_tg_cutw.p, cut.data(), (size_t)U * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(launch_tg_expand(d_tg_of.p, d_tg_cutw.p, N, d_tg_cl.p, stream));
  HIPCHK(hipMemcpyAsync(cl, d_tg_cl.p, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return HDPM_OK;
}

// ---- the posterior predictive from the recorded centers and sigmas (predict.hip)
int Summaries::predict_build(int32_t d, const int32_t* attrisize, double gamma, const int32_t* total_cls,
                             const double* centers, const double* sigmas) {
  if (int st = need(false, false)) return st;
  pr_d = 0;
  pr_emm = false;
  if (!total_cls || !centers || !sigmas) { err = "predict: bad arguments"; return HDPM_E_ARG; }
  err = pr_check_model(d, attrisize, gamma);
  if (!err.empty()) return HDPM_E_ARG;
  const int M = tr_M;
  std::vector<uint32_t> sizes((size_t)M * 256);
  HIPCHK(hipMemcpyAsync(sizes.data(), d_tr_sizes.p, sizes.size() * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  pr_off.assign((size_t)M + 1, 0);
  int Kmax = 0;
  for (int s = 0; s < M; ++s) {
    err = pr_check_draw(s, total_cls[s], sizes.data() + (size_t)s * 256);
    if (!err.empty()) return HDPM_E_ARG;
    pr_off[s + 1] = pr_off[s] + total_cls[s];
    Kmax = std::max(Kmax, total_cls[s]);
  }
  for (int s = 0; s < M; ++s) {
    err = pr_check_params(s, total_cls[s], d, attrisize, centers + (size_t)pr_off[s] * d,
                          sigmas + (size_t)pr_off[s] * d);
    if (!err.empty()) return HDPM_E_ARG;
  }
  const int64_t rows = pr_off[M];
  const size_t d4 = (size_t)pr_d4(d);
  std::vector<uint8_t> cen((size_t)rows * d4);
  std::vector<double> mm((size_t)rows * d * 2), lognk((size_t)rows);
  parallel_for(rows, [&](int64_t r0, int64_t r1) {
    pr_build_tables(r1 - r0, d, attrisize, centers + (size_t)r0 * d, sigmas + (size_t)r0 * d, cen.data() + r0 * d4,
                    mm.data() + (size_t)r0 * d * 2);
  });
  for (int s = 0; s < M; ++s)
    for (int k = 0; k < total_cls[s]; ++k) lognk[pr_off[s] + k] = std::log((double)sizes[(size_t)s * 256 + k]);
  d_pr_cen.ensure(cen.size());
  d_pr_mm.ensure(mm.size());
  d_pr_lognk.ensure(lognk.size());
  d_pr_off.ensure(pr_off.size());
  d_pr_sig.ensure((size_t)rows * d);
  HIPCHK(hipMemcpyAsync(d_pr_sig.p, sigmas, (size_t)rows * d * 8, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_pr_cen.p, cen.data(), cen.size(), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_pr_mm.p, mm.data(), mm.size() * 8, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_pr_lognk.p, lognk.data(), lognk.size() * 8, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_pr_off.p, pr_off.data(), pr_off.size() * 8, hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
  pr_att.assign(attrisize, attrisize + d);
  pr_gamma = gamma;
  pr_w0 = std::log(gamma) + pr_ll0(d, attrisize);
  pr_Kmax = Kmax;
  pr_d = d;
  return HDPM_OK;
}

// what every predict call needs: a trace, its parameters, and rows of codes in range (partial:
// 0, a missing attribute, is in range)
int Summaries::need_predict(const uint8_t* codes, int64_t rows, bool partial) {
  if (int st = need(false, false)) return st;
  if (pr_d == 0) { err = "predict: hdpm_predict_build has not been called"; return HDPM_E_ARG; }
  if (!codes || rows <= 0) { err = "predict: no rows"; return HDPM_E_ARG; }
  std::atomic<int64_t> bad{-1};
  parallel_for(rows, [&](int64_t r0, int64_t r1) {
    const int64_t at = partial ? pr_bad_code_partial(codes + (size_t)r0 * pr_d, r1 - r0, pr_d, pr_att.data())
                               : pr_bad_code(codes + (size_t)r0 * pr_d, r1 - r0, pr_d, pr_att.data());
    if (at < 0) return;
    int64_t seen = bad.load(), mine = r0 * pr_d + at;
    while ((seen < 0 || mine < seen) && !bad.compare_exchange_weak(seen, mine)) {}
  });
  if (bad.load() >= 0) {
    err = partial ? pr_code_message_partial(bad.load(), pr_d) : pr_code_message(bad.load(), pr_d);
    return HDPM_E_ARG;
  }
  return HDPM_OK;
}

// Rows in blocks whose device staging (packed codes, scratch columns, outputs) obeys the table
// budget, against draws s0 .. s1 - 1; each block's results go to the caller as it completes.
// tab: the tables of the partition (Ka classes) for coclass.  ll / resp: one draw.  A row's
// results do not depend on the block it falls in.  miss: code 0 is a missing attribute
// (k_pr_part; all the draws, no ll / resp).
void Summaries::predict_blocks(const uint8_t* codes, int64_t ny, int s0, int s1, const uint32_t* tab, int Ka,
                               double* lpd, double* p_new, double* coclass, double* ll, double* resp, bool miss) {
  const int d = pr_d;
  const size_t nw = (size_t)pr_d4(d) / 4;
  const size_t K1 = (size_t)(pr_off[s0 + 1] - pr_off[s0]);   // the clusters of the one draw of ll / resp
  const size_t per_row = nw * 4 + ((size_t)pr_Kmax + 1) * 8 + (tab ? (size_t)Ka * 8 : 0) + 16 + (ll ? K1 * 8 : 0) +
                         (resp ? (K1 + 1) * 8 : 0) + (miss ? 8 : 0);
  const size_t nb = pr_block(tr_budget, per_row, (size_t)ny);
  std::vector<double> w0;
  const double log_gamma = std::log(pr_gamma);
  if (miss) {
    d_pr_w0.ensure(nb);
    w0.resize(nb);
  }
  d_pr_cw.ensure(nw * nb);
  d_pr_w.ensure(((size_t)pr_Kmax + 1) * nb);
  d_pr_out.ensure(2 * nb);
  if (tab) d_pr_cc.ensure((size_t)Ka * nb);
  if (ll) d_pr_ll.ensure(K1 * nb);
  if (resp) d_pr_resp.ensure((K1 + 1) * nb);
  std::vector<uint32_t> cw(nw * nb);
  std::vector<double> t;
  auto take = [&](const double* dev, size_t cols, int64_t i0, int64_t nr, double* out) {
    // cols x nb on the device to rows of cols values
    t.resize(cols * nb);
    HIPCHK(hipMemcpyAsync(t.data(), dev, t.size() * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    parallel_for(nr, [&](int64_t r0, int64_t r1) {
      for (int64_t r = r0; r < r1; ++r)
        for (size_t c = 0; c < cols; ++c) out[(size_t)(i0 + r) * cols + c] = t[c * nb + r];
    });
  };
  for (int64_t i0 = 0; i0 < ny; i0 += (int64_t)nb) {
    const int64_t nr = std::min<int64_t>((int64_t)nb, ny - i0);
    parallel_for(nr, [&](int64_t r0, int64_t r1) { pr_pack_rows(codes + (size_t)i0 * d, r0, r1, d, nb, cw.data()); });
    HIPCHK(hipMemcpyAsync(d_pr_cw.p, cw.data(), cw.size() * 4, hipMemcpyHostToDevice, stream));
    PrNewArgs a{};
    a.cw = d_pr_cw.p;
    a.nrows = nr;
    a.nbp = (int64_t)nb;
    a.d = d;
    a.s0 = s0;
    a.s1 = s1;
    a.cen = d_pr_cen.p;
    a.mm = d_pr_mm.p;
    a.lognk = d_pr_lognk.p;
    a.off = d_pr_off.p;
    a.w0 = pr_w0;
    a.log_ng = std::log((double)tr_N + pr_gamma);
    a.w = d_pr_w.p;
    a.tab = tab;
    a.Ka = Ka;
    a.Kz = tr_Kz;
    a.na = d_pr_na.p;
    a.cc = d_pr_cc.p;
    a.lpd = lpd ? d_pr_out.p : nullptr;
    a.p_new = p_new ? d_pr_out.p + nb : nullptr;
    a.ll_out = ll ? d_pr_ll.p : nullptr;
    a.resp_out = resp ? d_pr_resp.p : nullptr;
    if (miss) {
      parallel_for(nr, [&](int64_t r0, int64_t r1) {
        for (int64_t r = r0; r < r1; ++r)
          w0[r] = log_gamma + pr_ll0_row(codes + (size_t)(i0 + r) * d, d, pr_att.data());
      });
      HIPCHK(hipMemcpyAsync(d_pr_w0.p, w0.data(), (size_t)nr * 8, hipMemcpyHostToDevice, stream));
      PrPartArgs pa{a, d_pr_w0.p, nullptr, 0, nullptr, 1, 1, s1 - s0};
      HIPCHK(launch_pr_part(pa, stream));
    } else {
      HIPCHK(launch_pr_new(a, stream));
    }
    if (lpd) HIPCHK(hipMemcpyAsync(lpd + i0, d_pr_out.p, (size_t)nr * 8, hipMemcpyDeviceToHost, stream));
    if (p_new) HIPCHK(hipMemcpyAsync(p_new + i0, d_pr_out.p + nb, (size_t)nr * 8, hipMemcpyDeviceToHost, stream));
    if (tab) take(d_pr_cc.p, (size_t)Ka, i0, nr, coclass);
    if (ll) take(d_pr_ll.p, K1, i0, nr, ll);
    if (resp) take(d_pr_resp.p, K1 + 1, i0, nr, resp);
    HIPCHK(hipStreamSynchronize(stream));
  }
}

// the exps of the (match, mismatch) pairs and attrisize on the device, built at the first call
// after predict_build that reads them (imputation, the profiles' code law)
void Summaries::need_emm() {
  if (pr_emm) return;
  const size_t n = (size_t)pr_off[tr_M] * pr_d * 2;
  d_pr_emm.ensure(n);
  d_pr_att.ensure((size_t)pr_d);
  HIPCHK(launch_pr_exp(d_pr_mm.p, (int64_t)n, d_pr_emm.p, stream));
  HIPCHK(hipMemcpyAsync(d_pr_att.p, pr_att.data(), (size_t)pr_d * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
  pr_emm = true;
}

// Imputation: blocks of rows (whole quanta of 64) and, within a block, chunks of draws, cut so
// that the block's staging -- packed codes, scratch columns, carried sums, the entries' list,
// pmf rows and carried sums, and the rows' records of one chunk of draws -- obeys the table
// budget (at least one quantum and one draw).  Per chunk k_pr_part leaves the records and
// k_pr_impute folds them into the entries' sums; a lane's walk over all the draws of a block is
// what a launch costs, so the rows stay together as far as they can and the draws are cut.  No
// result depends on either cut.
void Summaries::impute_blocks(const uint8_t* codes, int64_t ny, int ld, double* pmf, double* lpd) {
  const int d = pr_d, M = tr_M;
  const size_t q = kPrRowQuantum, nw = (size_t)pr_d4(d) / 4;
  need_emm();
  const size_t rec1 = (size_t)pr_Kmax + 2;                    // the longest record of one draw
  const size_t row_bytes = nw * 4 + ((size_t)pr_Kmax + 1) * 8 + 16 + 8 + 24 + rec1 * 8;
  const size_t entry_bytes = (size_t)ld * 8 + 24;
  const size_t nq = ((size_t)ny + q - 1) / q;
  std::vector<int64_t> qoff(nq + 1);
  pr_missing_offsets(codes, ny, d, q, qoff.data());
  struct Block { size_t q0, nq; };
  std::vector<Block> blk;
  size_t nb = 0;
  int64_t nemax = 0;
  for (size_t q0 = 0; q0 < nq;) {
    const size_t n = pr_impute_quanta(qoff.data(), nq, q0, tr_budget, row_bytes, entry_bytes, (int64_t)1 << 28);
    blk.push_back({q0, n});
    nb = std::max(nb, n * q);
    nemax = std::max(nemax, qoff[q0 + n] - qoff[q0]);
    q0 += n;
  }
  d_pr_cw.ensure(nw * nb);
  d_pr_w.ensure(((size_t)pr_Kmax + 1) * nb);
  d_pr_out.ensure(2 * nb);
  d_pr_w0.ensure(nb);
  d_pr_carry.ensure(3 * nb);
  d_pr_ent.ensure((size_t)nemax * 2);
  d_pr_pmf.ensure((size_t)nemax * ld);
  d_pr_st.ensure((size_t)nemax * 2);
  std::vector<uint32_t> cw(nw * nb), ent((size_t)nemax * 2);
  std::vector<double> w0(nb);
  const double log_gamma = std::log(pr_gamma);
  const int64_t whole = pr_off[M] + 2 * (int64_t)M;           // the record of all the draws
  for (const Block& b : blk) {
    const int64_t i0 = (int64_t)(b.q0 * q), nr = std::min<int64_t>((int64_t)(b.nq * q), ny - i0);
    const int64_t e0 = qoff[b.q0], ne = qoff[b.q0 + b.nq] - e0;
    parallel_for(nr, [&](int64_t r0, int64_t r1) {
      pr_pack_rows(codes + (size_t)i0 * d, r0, r1, d, nb, cw.data());
      for (int64_t r = r0; r < r1; ++r)
        w0[r] = log_gamma + pr_ll0_row(codes + (size_t)(i0 + r) * d, d, pr_att.data());
    });
    pr_missing_entries(codes, i0, i0 + nr, d, ent.data());
    HIPCHK(hipMemcpyAsync(d_pr_cw.p, cw.data(), cw.size() * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_pr_w0.p, w0.data(), (size_t)nr * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_pr_ent.p, ent.data(), (size_t)ne * 8, hipMemcpyHostToDevice, stream));
    // what the budget leaves for the records, in doubles per row of this block; the buffer
    // holds this block's rows, not the largest block's
    const int64_t rstride = pr_impute_rstride(tr_budget, b.nq * q, row_bytes, ne, entry_bytes, rec1, whole);
    d_pr_r.ensure((size_t)rstride * (b.nq * q));
    PrPartArgs pa{};
    PrNewArgs& a = pa.n;
    a.cw = d_pr_cw.p;
    a.nrows = nr;
    a.nbp = (int64_t)nb;
    a.d = d;
    a.cen = d_pr_cen.p;
    a.mm = d_pr_mm.p;
    a.lognk = d_pr_lognk.p;
    a.off = d_pr_off.p;
    a.log_ng = std::log((double)tr_N + pr_gamma);
    a.w = d_pr_w.p;
    a.lpd = lpd ? d_pr_out.p : nullptr;
    pa.w0 = d_pr_w0.p;
    pa.r = d_pr_r.p;
    pa.rstride = rstride;
    pa.carry = d_pr_carry.p;
    pa.M = M;
    PrImpArgs ia{};
    ia.ent = d_pr_ent.p;
    ia.nent = (int)ne;
    ia.d = d;
    ia.ld = ld;
    ia.st = d_pr_st.p;
    ia.att = d_pr_att.p;
    ia.cen = d_pr_cen.p;
    ia.emm = d_pr_emm.p;
    ia.off = d_pr_off.p;
    ia.r = d_pr_r.p;
    ia.rstride = rstride;
    ia.pmf = d_pr_pmf.p;
    for (int s0 = 0; s0 < M;) {
      const int s1 = pr_draw_chunk(pr_off.data(), M, s0, rstride);
      a.s0 = ia.s0 = s0;
      a.s1 = ia.s1 = s1;
      pa.first = ia.first = s0 == 0;
      pa.last = ia.last = s1 == M;
      HIPCHK(launch_pr_part(pa, stream));
      HIPCHK(launch_pr_impute(ia, stream));
      s0 = s1;
    }
    if (ne > 0)
      HIPCHK(hipMemcpyAsync(pmf + (size_t)e0 * ld, d_pr_pmf.p, (size_t)ne * ld * 8, hipMemcpyDeviceToHost, stream));
    if (lpd) HIPCHK(hipMemcpyAsync(lpd + i0, d_pr_out.p, (size_t)nr * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));        // the staging is reused by the next block
  }
}

int Summaries::predict_new(const uint8_t* codes, int32_t ny, const int32_t* cl, int32_t Ka, double* lpd,
                           double* p_new, double* coclass) {
  if (int st = need_predict(codes, ny)) return st;
  if (coclass) {
    if (!cl) { err = "predict: coclass needs a partition of the training points"; return HDPM_E_ARG; }
    err = pr_check_classes(cl, tr_N, Ka);
    if (!err.empty()) return HDPM_E_ARG;
  }
  if (!lpd && !p_new && !coclass) return HDPM_OK;
  if (!coclass) {
    predict_blocks(codes, ny, 0, tr_M, nullptr, 0, lpd, p_new, nullptr, nullptr, nullptr);
    return HDPM_OK;
  }
  std::vector<double> na((size_t)Ka, 0.0);
  for (int i = 0; i < tr_N; ++i) na[cl[i]] += 1.0;
  d_pr_na.ensure((size_t)Ka);
  HIPCHK(hipMemcpyAsync(d_pr_na.p, na.data(), (size_t)Ka * 8, hipMemcpyHostToDevice, stream));
  // one candidate always fits a block: its tables stay on the device while the rows go through
  blocks({cl, 0, 1}, Ka, false, false, false, [&](int, int, const uint8_t*) {
    predict_blocks(codes, ny, 0, tr_M, d_tr_tab.p, Ka, lpd, p_new, coclass, nullptr, nullptr);
  });
  return HDPM_OK;
}

int Summaries::predict_own(const uint8_t* codes, double* lppd, double* var, double* logcpo) {
  if (int st = need_predict(codes, tr_N)) return st;
  if (!lppd && !var && !logcpo) return HDPM_OK;
  const int d = pr_d, N = tr_N;
  const size_t nw = (size_t)pr_d4(d) / 4;
  const size_t nb = pr_block(tr_budget, nw * 4 + 24, (size_t)N);
  d_pr_cw.ensure(nw * nb);
  d_pr_out.ensure(3 * nb);
  std::vector<uint32_t> cw(nw * nb);
  for (int64_t i0 = 0; i0 < N; i0 += (int64_t)nb) {
    const int64_t nr = std::min<int64_t>((int64_t)nb, N - i0);
    parallel_for(nr, [&](int64_t r0, int64_t r1) { pr_pack_rows(codes + (size_t)i0 * d, r0, r1, d, nb, cw.data()); });
    HIPCHK(hipMemcpyAsync(d_pr_cw.p, cw.data(), cw.size() * 4, hipMemcpyHostToDevice, stream));
    PrOwnArgs a{};
    a.cw = d_pr_cw.p;
    a.nrows = nr;
    a.nbp = (int64_t)nb;
    a.row0 = i0;
    a.d = d;
    a.M = tr_M;
    a.Np = tr_Np;
    a.lab = d_tr_lab.p;
    a.cen = d_pr_cen.p;
    a.mm = d_pr_mm.p;
    a.off = d_pr_off.p;
    a.lppd = lppd ? d_pr_out.p : nullptr;
    a.var = var ? d_pr_out.p + nb : nullptr;
    a.logcpo = logcpo ? d_pr_out.p + 2 * nb : nullptr;
    HIPCHK(launch_pr_own(a, stream));
    if (lppd) HIPCHK(hipMemcpyAsync(lppd + i0, d_pr_out.p, (size_t)nr * 8, hipMemcpyDeviceToHost, stream));
    if (var) HIPCHK(hipMemcpyAsync(var + i0, d_pr_out.p + nb, (size_t)nr * 8, hipMemcpyDeviceToHost, stream));
    if (logcpo) HIPCHK(hipMemcpyAsync(logcpo + i0, d_pr_out.p + 2 * nb, (size_t)nr * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  return HDPM_OK;
}

int Summaries::predict_loglik(int32_t s, const uint8_t* codes, int32_t ny, double* ll, double* resp) {
  if (int st = need_predict(codes, ny)) return st;
  if (s < 0 || s >= tr_M) {
    err = "predict: draw " + std::to_string(s) + " is outside 0.." + std::to_string(tr_M - 1);
    return HDPM_E_ARG;
  }
  if (ll || resp) predict_blocks(codes, ny, s, s + 1, nullptr, 0, nullptr, nullptr, nullptr, ll, resp);
  return HDPM_OK;
}

// Rows with missing attributes (code 0): predict_new's outputs with those attributes left out
// of every sum
int Summaries::predict_partial(const uint8_t* codes, int32_t ny, const int32_t* cl, int32_t Ka, double* lpd,
                               double* p_new, double* coclass) {
  if (int st = need_predict(codes, ny, true)) return st;
  if (coclass) {
    if (!cl) { err = "predict: coclass needs a partition of the training points"; return HDPM_E_ARG; }
    err = pr_check_classes(cl, tr_N, Ka);
    if (!err.empty()) return HDPM_E_ARG;
  }
  if (!lpd && !p_new && !coclass) return HDPM_OK;
  if (!coclass) {
    predict_blocks(codes, ny, 0, tr_M, nullptr, 0, lpd, p_new, nullptr, nullptr, nullptr, true);
    return HDPM_OK;
  }
  std::vector<double> na((size_t)Ka, 0.0);
  for (int i = 0; i < tr_N; ++i) na[cl[i]] += 1.0;
  d_pr_na.ensure((size_t)Ka);
  HIPCHK(hipMemcpyAsync(d_pr_na.p, na.data(), (size_t)Ka * 8, hipMemcpyHostToDevice, stream));
  blocks({cl, 0, 1}, Ka, false, false, false, [&](int, int, const uint8_t*) {
    predict_blocks(codes, ny, 0, tr_M, d_tr_tab.p, Ka, lpd, p_new, coclass, nullptr, nullptr, true);
  });
  return HDPM_OK;
}

// The law of every missing code given its row's observed ones: pmf[n_missing x ld], entries in
// row-major order of the codes; lpd as predict_partial gives it
int Summaries::predict_impute(const uint8_t* codes, int32_t ny, int64_t n_missing, int32_t ld, double* pmf,
                              double* lpd) {
  if (int st = need_predict(codes, ny, true)) return st;
  const int64_t have = pr_count_missing(codes, ny, pr_d);
  if (n_missing != have) {
    err = "predict: n_missing is " + std::to_string(n_missing) + " but the rows hold " + std::to_string(have) +
          " missing codes";
    return HDPM_E_ARG;
  }
  err = pr_check_ld(codes, ny, pr_d, pr_att.data(), ld);
  if (!err.empty()) return HDPM_E_ARG;
  if (have > 0 && !pmf) { err = "predict: no pmf"; return HDPM_E_ARG; }
  if (have == 0 && !lpd) return HDPM_OK;
  if (have == 0) predict_blocks(codes, ny, 0, tr_M, nullptr, 0, lpd, nullptr, nullptr, nullptr, nullptr, true);
  else impute_blocks(codes, ny, ld, pmf, lpd);
  return HDPM_OK;
}

// ---- what each class of an estimate is (profile.hip, profile_host.hpp): the tables of the one
// candidate stay on the device while the draws go through in chunks (u_s, then Welford's sums)
// and the attributes in blocks (the level rows), each copied to the caller as it completes
int Summaries::predict_profile(const int32_t* cl, int32_t Ka, int32_t ld, uint64_t* center_cnt, double* code_pmf,
                               double* sigma_mean, double* sigma_var, double* sigma_trace) {
  if (int st = need(false, false)) return st;
  if (pr_d == 0) { err = "profile: hdpm_predict_build has not been called"; return HDPM_E_ARG; }
  if (!cl) { err = "profile: no partition"; return HDPM_E_ARG; }
  err = pr_check_classes(cl, tr_N, Ka);
  if (!err.empty()) return HDPM_E_ARG;
  err = pf_check_ld(pr_d, pr_att.data(), ld);
  if (!err.empty()) return HDPM_E_ARG;
  const bool sig = sigma_mean || sigma_var || sigma_trace, lev = center_cnt || code_pmf;
  if (!sig && !lev) return HDPM_OK;
  const int d = pr_d, M = tr_M, Kz = tr_Kz;
  std::vector<double> na((size_t)Ka, 0.0);
  for (int i = 0; i < tr_N; ++i) na[cl[i]] += 1.0;
  d_pr_na.ensure((size_t)Ka);
  HIPCHK(hipMemcpyAsync(d_pr_na.p, na.data(), (size_t)Ka * 8, hipMemcpyHostToDevice, stream));
  if (code_pmf) need_emm();
  blocks({cl, 0, 1}, Ka, false, false, false, [&](int, int, const uint8_t*) {
    if (sig) {
      const size_t n = (size_t)Ka * d;
      const std::vector<int> cut = pf_draw_chunks(tr_budget, Ka, d, M);
      size_t most = 0;
      for (size_t c = 0; c + 1 < cut.size(); ++c) most = std::max(most, (size_t)(cut[c + 1] - cut[c]));
      d_pf_u.ensure(most * n);
      d_pf_st.ensure(4 * n);                          // (mean, m2) carried, then mean and var
      for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int s0 = cut[c], s1 = cut[c + 1];
        HIPCHK(launch_pf_sigma({d_tr_tab.p, Ka, Kz, d, s0, s1, d_pr_off.p, d_pr_sig.p, d_pr_na.p, d_pf_u.p}, stream));
        if (sigma_mean || sigma_var)
          HIPCHK(launch_pf_welford({d_pf_u.p, (int)n, s0, s1, M, d_pf_st.p, d_pf_st.p + 2 * n, d_pf_st.p + 3 * n},
                                   stream));
        if (sigma_trace)
          HIPCHK(hipMemcpyAsync(sigma_trace + (size_t)s0 * n, d_pf_u.p, (size_t)(s1 - s0) * n * 8,
                                hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));         // the staging is reused by the next chunk
      }
      if (sigma_mean) HIPCHK(hipMemcpyAsync(sigma_mean, d_pf_st.p + 2 * n, n * 8, hipMemcpyDeviceToHost, stream));
      if (sigma_var) HIPCHK(hipMemcpyAsync(sigma_var, d_pf_st.p + 3 * n, n * 8, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    if (lev) {
      const int slot_bytes = (center_cnt ? 8 : 0) + (code_pmf ? 8 : 0);
      const std::vector<int> cut = pf_attr_blocks(tr_budget, Ka, ld, slot_bytes, d);
      size_t most = 0;
      for (size_t c = 0; c + 1 < cut.size(); ++c) most = std::max(most, (size_t)(cut[c + 1] - cut[c]));
      const size_t cap = (size_t)Ka * most * ld;
      if (center_cnt) d_pf_cnt.ensure(cap);
      if (code_pmf) d_pf_law.ensure(cap);
      for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int j0 = cut[c], jb = cut[c + 1] - cut[c];
        const size_t row = (size_t)jb * ld * 8;
        HIPCHK(launch_pf_levels({d_tr_tab.p, M, Ka, Kz, d, j0, jb, ld, 0, d_pr_off.p, d_pr_cen.p, d_pr_emm.p,
                                 d_pr_att.p, d_pr_na.p, center_cnt ? d_pf_cnt.p : nullptr,
                                 code_pmf ? d_pf_law.p : nullptr},
                                stream));
        // class a's rows of the block are contiguous on both sides: Ka pieces of jb x ld slots
        if (center_cnt)
          HIPCHK(hipMemcpy2DAsync(center_cnt + (size_t)j0 * ld, (size_t)d * ld * 8, d_pf_cnt.p, row, row, (size_t)Ka,
                                  hipMemcpyDeviceToHost, stream));
        if (code_pmf)
          HIPCHK(hipMemcpy2DAsync(code_pmf + (size_t)j0 * ld, (size_t)d * ld * 8, d_pf_law.p, row, row, (size_t)Ka,
                                  hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));         // the staging is reused by the next block
      }
    }
  });
  return HDPM_OK;
}

}  // namespace hdpm
