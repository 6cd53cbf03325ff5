// summary_launch.hpp -- launchers of the posterior-summary kernels: posterior.hip
// (launch_psm, launch_vi_terms), trace_summary.hip (launch_tr_pack .. launch_tr_reduce,
// launch_tg_*) and trace_uncertainty.hip (launch_tr_transpose, launch_tr_affinity,
// launch_tr_cross), trace_refine.hip (launch_rf_htable, launch_rf_gains), trace_merge.hip
// (launch_mg_pairs, launch_mg_gain, launch_mg_fold), predict.hip
// (launch_pr_new .. launch_pr_impute) and profile.hip (launch_pf_*).  Included by the units that
// define them and by summary_host.cpp, their only caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hdpm {

hipError_t launch_psm(const int32_t* trace, int M, int N, uint8_t* lab, uint32_t* cnt, hipStream_t s);
hipError_t launch_vi_terms(const uint32_t* cnt, int N, int M, const int32_t* cls, int ncand, double* all, double* same,
                           hipStream_t s);
hipError_t launch_tr_pack(const int32_t* trace, int nm, int N, int Np, uint8_t* lab, hipStream_t s);
hipError_t launch_tr_sizes(const uint8_t* lab, int Np, int M, uint32_t* sizes, hipStream_t s);
hipError_t launch_tr_tables(const uint8_t* lab, const uint8_t* cls, int Np, int M, int ncand, int Ka, int Kz,
                            uint32_t* tab, hipStream_t s);
hipError_t launch_tr_gather(const uint8_t* lab, const uint8_t* cls, int N, int Np, int M, int ncand, int Ka, int Kz,
                            const uint32_t* tab, const uint32_t* sizes, uint64_t* all, uint64_t* same,
                            hipStream_t s);
hipError_t launch_tr_reduce(const uint32_t* tab, int ncand, int M, int cells, uint64_t* q1, double* l1, uint64_t* q,
                            double* l, hipStream_t s);
hipError_t launch_tr_transpose(const uint32_t* tab, int M, int Ka, int Kz, uint32_t* tabT, hipStream_t s);
hipError_t launch_tr_affinity(const uint8_t* lab, int Np, int M, int Ka, int Kz, const uint32_t* tabT, int i0, int npts,
                              uint64_t* out, hipStream_t s);
hipError_t launch_tr_cross(const uint32_t* tabT, int M, int Ka, int Kz, uint64_t* cross, hipStream_t s);
// trace_refine.hip.  launch_rf_gains: the staged sums of npts points from i0, then their gains
// (over the sums, if full) and argmin; tabT is launch_rf_htable's array for HDPM_LOSS_VI and
// launch_tr_transpose's for HDPM_LOSS_BINDER, ct the class table k_rf_best describes.
hipError_t launch_rf_htable(const uint32_t* tab, int M, int Ka, int Kz, double* tabH, hipStream_t s);
hipError_t launch_rf_gains(int loss, const uint8_t* lab, const uint8_t* cls, int Np, int M, int Ka, int Kz,
                           const void* tabT, int i0, int npts, const double* ct, int N, int full, uint64_t* stage,
                           int32_t* best, double* gain, hipStream_t s);
// trace_merge.hip.  launch_mg_pairs: VI's per-slice partial sums of all pairs (only < 0) or of the
// pairs of class `only`, into part (mg_slices(M) x Ka x Ka doubles).  launch_mg_gain: the Ka x Ka
// gains from part (HDPM_LOSS_VI) or from launch_tr_cross's integers (HDPM_LOSS_BINDER) and the
// class sizes n (Ka doubles).  launch_mg_fold: row b of every draw's table added into row a
// and zeroed, in tab (M x Ka x Kz) and tabT (M x Kz x Ka); either may be null.
int mg_slices(int M);
hipError_t launch_mg_pairs(const uint32_t* tabT, int M, int Ka, int Kz, int only, double* part, hipStream_t s);
hipError_t launch_mg_gain(int loss, const double* part, const uint64_t* cross, const double* n, int M, int Ka, int N,
                          double* gain, hipStream_t s);
hipError_t launch_mg_fold(uint32_t* tab, uint32_t* tabT, int M, int Ka, int Kz, int a, int b, hipStream_t s);
hipError_t launch_tg_insert(const uint8_t* lab, int N, int Np, int M, int hash_bits, uint32_t tslots,
                            uint32_t max_groups, uint32_t* rep, uint32_t* first, uint32_t* pslot, uint32_t* ctl,
                            hipStream_t s);
hipError_t launch_tg_finish(const uint8_t* lab, int N, int Np, int M, int U, int Mp, int Up, const uint32_t* pslot,
                            const uint32_t* slot_gid, const uint32_t* first, uint32_t* group_of, uint32_t* weight,
                            uint8_t* sig, uint8_t* sigT, hipStream_t s);
hipError_t launch_tg_counts(const uint8_t* sig, int U, int M, int Mp, uint32_t* S, hipStream_t s);
hipError_t launch_tg_tables(const uint8_t* sigT, const uint8_t* cut, const uint32_t* w, int U, int Up, int M, int ncut,
                            int Ka, int Kz, uint32_t* tab, hipStream_t s);
hipError_t launch_tg_gather(const uint8_t* sigT, const uint8_t* cut, int U, int Up, int M, int ncut, int Ka, int Kz,
                            const uint32_t* tab, const uint32_t* sizes, uint64_t* all, uint64_t* same, hipStream_t s);
hipError_t launch_tg_expand(const uint32_t* group_of, const int32_t* cut, int N, int32_t* cl, hipStream_t s);

// predict.hip.  The parameter tables of all draws (predict_host.hpp): parameter row off[s] + k
// is cluster k of draw s; cen holds its centers as bytes (rows of d rounded up to a multiple
// of 4), mm its (match, mismatch) pairs (rows of d pairs), lognk its log size.  A block of
// rows is cw: word w of row r, four codes, at cw[w * nbp + r].
constexpr int kPrThreads = 256;     // rows of a tile, one per lane
constexpr int kPrG = 8;             // clusters staged together = accumulators of a lane
constexpr int kPrDC = 256;          // attributes of a staged chunk (a multiple of 4)
constexpr int kPrOwnDraws = 4;      // draws in flight per lane of k_pr_own

struct PrNewArgs {
  const uint32_t* cw;
  int64_t nrows, nbp;
  int d, s0, s1;                    // draws s0 .. s1 - 1
  const uint8_t* cen;
  const double* mm;
  const double* lognk;
  const int64_t* off;               // M + 1
  double w0, log_ng;                // log gamma + ll_0; log(N + gamma)
  double* w;                        // scratch, (Kmax + 1) x nbp
  const uint32_t* tab;              // T^s[a][k] as k_tr_tables lays it out (M x Ka x Kz), or null
  int Ka, Kz;
  const double* na;                 // Ka class sizes
  double* cc;                       // Ka x nbp: the fold's running sums, coclass at the end
  double* lpd;                      // nbp each, or null
  double* p_new;
  double* ll_out;                   // one draw: K x nbp, or null
  double* resp_out;                 // one draw: (K + 1) x nbp, slot 0 the new cluster, or null
};
struct PrOwnArgs {
  const uint32_t* cw;
  int64_t nrows, nbp, row0;         // the block's first row is point row0 of the trace
  int d, M, Np;
  const uint8_t* lab;               // the trace's label bytes, M x Np
  const uint8_t* cen;
  const double* mm;
  const int64_t* off;
  double* lppd;                     // nbp each, or null
  double* var;
  double* logcpo;
};
// Rows with missing attributes (code 0).  k_pr_part is k_pr_new with the missing attributes
// left out of every sum and a w_0 per row (n.w0, n.ll_out and n.resp_out are not read); for
// k_pr_impute it leaves, per row of the block, a record of up to rstride doubles: draw s at
// off[s] - off[s0] + 2 (s - s0), holding lse, r_0, r_1 .. r_K.  A wave of k_pr_impute reads
// a draw of its row as one contiguous piece.  The draws may come in chunks s0 .. s1 - 1 of
// 0 .. M - 1, one launch each in order: a row's running sums (lpd's maximum and sum, p_new's
// sum) then pass through carry, double for double, and cc keeps the fold's.
struct PrPartArgs {
  PrNewArgs n;
  const double* w0;                 // nbp: log gamma + ll_0 of the row
  double* r;                        // nbp x rstride, or null
  int64_t rstride;                  // at least off[s1] - off[s0] + 2 (s1 - s0)
  double* carry;                    // 3 x nbp, or null when first and last
  int first, last, M;               // s0 == 0; s1 == M; the draws in all
};
// k_pr_impute: a wave per missing entry, lanes over the levels.  ent holds (row of the block,
// attribute) per entry; emm the exps of mm; the draws are the chunk s0 .. s1 - 1 that k_pr_part
// just left in r.  Between chunks A_l stays in the entry's pmf row and (mx, acc) in st.
constexpr int kPrImpWaves = 4;      // entries of a workgroup
struct PrImpArgs {
  const uint32_t* ent;
  int nent;
  int d, s0, s1, first, last, ld;   // first: s0 == 0; last: s1 == M
  double* st;                       // 2 x nent
  const int32_t* att;               // d
  const uint8_t* cen;
  const double* emm;
  const int64_t* off;
  const double* r;                  // the rows' records as k_pr_part left them
  int64_t rstride;
  double* pmf;                      // nent x ld
};
hipError_t launch_pr_new(const PrNewArgs& a, hipStream_t s);
hipError_t launch_pr_own(const PrOwnArgs& a, hipStream_t s);
hipError_t launch_pr_part(const PrPartArgs& a, hipStream_t s);
hipError_t launch_pr_exp(const double* x, int64_t n, double* out, hipStream_t s);
hipError_t launch_pr_impute(const PrImpArgs& a, hipStream_t s);

// profile.hip.  The estimate's tables tab = T^s[a][k] at tab[(s * Ka + a) * Kz + k] (k_tr_tables)
// folded with the parameter tables above; sig holds the raw sigmas, rows of d.
constexpr int kPfThreads = 256;     // lanes of k_pf_sigma over the attributes of one (draw, class)
// k_pf_sigma: u_s of the draws s0 .. s1 - 1, u[((s - s0) * Ka + a) * d + j]
struct PfSigArgs {
  const uint32_t* tab;
  int Ka, Kz, d, s0, s1;
  const int64_t* off;
  const double* sig;
  const double* na;                 // Ka class sizes
  double* u;
};
// k_pf_welford: the chunk's u_s folded into (mean, m2) per (class, attribute), st[0 .. n) the
// means and st[n .. 2n) the m2, n = Ka x d; at the last chunk mean / var receive the results
struct PfWelArgs {
  const double* u;
  int n, s0, s1, M;
  double* st;
  double* mean;                     // n each, or null
  double* var;
};
// k_pf_levels: the level rows of the attributes j0 .. j0 + jb - 1 over all the draws, staged as
// (a * jb + j - j0) * ld + l - 1, every slot written; cnt and law may each be null.  A lane keeps
// its level rows in LDS during the walk: kPfLdsBytes per workgroup (one wave) bound the lanes
// that work (launch_pf_levels sets `lanes`)
constexpr int kPfLdsBytes = 64 << 10;
constexpr int kPfGroup = 4;         // clusters whose parameters a lane fetches together
struct PfLevArgs {
  const uint32_t* tab;
  int M, Ka, Kz, d, j0, jb, ld, lanes;
  const int64_t* off;
  const uint8_t* cen;
  const double* emm;
  const int32_t* att;
  const double* na;
  uint64_t* cnt;
  double* law;
};
hipError_t launch_pf_sigma(const PfSigArgs& a, hipStream_t s);
hipError_t launch_pf_welford(const PfWelArgs& a, hipStream_t s);
hipError_t launch_pf_levels(const PfLevArgs& a, hipStream_t s);

}  // namespace hdpm
