// summary_host.hpp -- the posterior summaries of a context: the state and host logic behind
// hdpm_psm_* (posterior.hip), hdpm_trace_* (trace_summary.hip, trace_uncertainty.hip) and
// hdpm_predict_* (predict.hip, profile.hip).
//
// The summaries work on saved labels and never touch chain state: of their context they use
// the main stream and the error string, bound at construction.  Every method is the body of
// the C call of the same name (include/hdpm.h) and returns its HDPM_* status; HIP errors
// leave as HipError, for the caller's guard.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "host_util.hpp"

struct hdpm_refine_info;

namespace hdpm {

class Summaries {
 public:
  Summaries(hipStream_t& stream, std::string& err) : stream(stream), err(err) {}

  int psm_build(const int32_t* c_trace, int32_t M, int32_t N);
  int psm_rows(int32_t row0, int32_t nrows, double* out);
  int psm_vi_lb(const int32_t* cls, int32_t ncand, double* out);

  int trace_build(const int32_t* c_trace, int32_t M, int32_t N, int64_t table_budget_bytes);
  int trace_terms(const int32_t* cls, int32_t ncand, uint64_t* all, uint64_t* same);
  int trace_losses(const int32_t* cls, int32_t ncand, double* vi_lb, double* vi, uint64_t* binder_Q,
                   uint64_t* binder_P);
  int trace_tables(const int32_t* cls, int32_t ncand, int32_t m0, int32_t nm, uint32_t* out);
  int trace_distances(const int32_t* cls, int32_t ncand, double* vi, uint64_t* binder, int32_t* draw_k);
  int trace_affinity(const int32_t* cl, int32_t Ka, uint64_t* aff, uint64_t* cross);
  int trace_move_gains(const int32_t* cl, int32_t Ka, int32_t loss, int32_t* best, double* gain, double* full);
  int trace_refine(const int32_t* cl, int32_t loss, int32_t max_rounds, int32_t* cl_out, hdpm_refine_info* info,
                   double* history);
  int trace_merge_gains(const int32_t* cl, int32_t Ka, int32_t loss, double* gain, int32_t* best, double* best_gain);
  int trace_merge_path(const int32_t* cl, int32_t Ka, int32_t loss, int32_t k_min, int32_t* merge, double* step_gain,
                       double* value, int32_t* steps);
  int trace_refine_merge(const int32_t* cl, int32_t loss, int32_t max_rounds, int32_t max_merges, int32_t* cl_out,
                         hdpm_refine_info* info, int32_t* merges, double* history);
  int trace_groups(int32_t max_groups, int32_t hash_bits, int32_t* U_out);
  int trace_group_info(int32_t* first, int32_t* weight, int32_t* group_of, uint32_t* counts);
  int trace_avg_tree(int32_t* merge, double* height);
  int trace_cut_losses(int32_t k0, int32_t nk, double* vi_lb, double* vi, uint64_t* binder_A, uint64_t* binder_Q);
  int trace_cut_labels(int32_t k, int32_t* cl);

  int predict_build(int32_t d, const int32_t* attrisize, double gamma, const int32_t* total_cls,
                    const double* centers, const double* sigmas);
  int predict_new(const uint8_t* codes, int32_t ny, const int32_t* cl, int32_t Ka, double* lpd, double* p_new,
                  double* coclass);
  int predict_own(const uint8_t* codes, double* lppd, double* var, double* logcpo);
  int predict_loglik(int32_t s, const uint8_t* codes, int32_t ny, double* ll, double* resp);
  int predict_partial(const uint8_t* codes, int32_t ny, const int32_t* cl, int32_t Ka, double* lpd, double* p_new,
                      double* coclass);
  int predict_impute(const uint8_t* codes, int32_t ny, int64_t n_missing, int32_t ld, double* pmf, double* lpd);
  int predict_profile(const int32_t* cl, int32_t Ka, int32_t ld, uint64_t* center_cnt, double* code_pmf,
                      double* sigma_mean, double* sigma_var, double* sigma_trace);

 private:
  hipStream_t& stream;
  std::string& err;

  // hdpm_psm_*: label bytes, co-clustering counts, VI.lb sums
  DevBuf<int32_t> d_psm_trace, d_psm_cls;
  DevBuf<uint8_t> d_psm_lab;
  DevBuf<uint32_t> d_psm_cnt;
  DevBuf<double> d_psm_all, d_psm_same;
  int psm_N = 0, psm_M = 0;
  // hdpm_trace_*: label bytes (M x Np), cluster sizes of the draws (M x 256), and per block
  // of candidates their label bytes, contingency tables (nc x M x Ka x Kz), per-point sums
  // and per-draw / per-candidate reductions
  DevBuf<uint8_t> d_tr_lab, d_tr_cls;
  DevBuf<uint32_t> d_tr_sizes, d_tr_tab;
  DevBuf<uint64_t> d_tr_all, d_tr_same, d_tr_q1, d_tr_q;
  DevBuf<double> d_tr_l1, d_tr_l;
  int tr_N = 0, tr_M = 0, tr_Np = 0, tr_Kz = 0;
  size_t tr_budget = 0;
  uint64_t tr_P = 0;     // sum_m sum_b C2(n^m_b)
  double tr_S = 0.0;     // sum_m sum_b n^m_b log2 n^m_b
  // per draw (trace_distances): P_m, S_m and the cluster count; the estimate's tables
  // transposed, the staging of one block of points of aff, and cross (trace_affinity)
  std::vector<uint64_t> tr_Pm;
  std::vector<double> tr_Sm;
  std::vector<int32_t> tr_Km;
  DevBuf<uint32_t> d_tr_tabT;
  DevBuf<uint64_t> d_tr_aff, d_tr_cross;
  // the single-point moves (trace_refine.hip): the (h(T), h(T - 1)) pairs of the transposed
  // tables, the class table, and per block of points the staged sums, best and gain
  DevBuf<double> d_rf_h, d_rf_ct, d_rf_gain;
  DevBuf<uint64_t> d_rf_stage;
  DevBuf<int32_t> d_rf_best;
  // the pair merges (trace_merge.hip): VI's per-slice partial sums (slices x Ka x Ka), the class
  // sizes and the Ka x Ka gains; Binder reads d_tr_cross
  DevBuf<double> d_mg_part, d_mg_n, d_mg_gain;
  // groups of equal label columns and their average-linkage tree (trace_groups ..
  // trace_cut_labels): the open-addressing table, group_of per point, the groups'
  // signatures both ways round, S (U x U) once it is first needed, the tree on the host
  DevBuf<uint32_t> d_tg_rep, d_tg_slotfirst, d_tg_pslot, d_tg_ctl, d_tg_slotgid, d_tg_of, d_tg_first, d_tg_w, d_tg_S;
  DevBuf<uint8_t> d_tg_sig, d_tg_sigT, d_tg_cut;
  DevBuf<uint64_t> d_tg_all, d_tg_same;
  DevBuf<int32_t> d_tg_cl, d_tg_cutw;
  int tg_U = 0, tg_Mp = 0, tg_Up = 0;
  bool tg_counts = false, tg_tree = false;
  std::vector<uint32_t> tg_first, tg_w;
  std::vector<int32_t> tg_merge;
  std::vector<double> tg_height;

  // hdpm_predict_*: the parameter tables of the trace's draws (parameter row pr_off[s] + k is
  // cluster k of draw s: center bytes, (match, mismatch) pairs, log sizes) and, per block of
  // rows, the packed codes, the scratch columns and the outputs
  DevBuf<uint8_t> d_pr_cen;
  DevBuf<double> d_pr_mm, d_pr_lognk, d_pr_w, d_pr_cc, d_pr_na, d_pr_out, d_pr_ll, d_pr_resp;
  DevBuf<int64_t> d_pr_off;
  DevBuf<uint32_t> d_pr_cw;
  std::vector<int64_t> pr_off;
  std::vector<int32_t> pr_att;
  int pr_d = 0, pr_Kmax = 0;   // pr_d == 0: no parameters
  double pr_gamma = 0.0, pr_w0 = 0.0;
  // Rows with missing attributes add w_0 per row.  Imputation adds the exps of the pairs and
  // attrisize on the device (built at its first call after predict_build: pr_emm) and, per
  // block of rows, a record per row (lse and r_k of a chunk of draws), the rows' sums carried
  // between chunks, and the entries' list, pmf rows and carried (mx, acc)
  DevBuf<double> d_pr_w0, d_pr_emm, d_pr_r, d_pr_pmf, d_pr_carry, d_pr_st;
  DevBuf<uint32_t> d_pr_ent;
  DevBuf<int32_t> d_pr_att;
  bool pr_emm = false;
  // The profiles of an estimate's classes (profile.hip) add the raw sigmas (rows of d, as the
  // pairs) and, per chunk of draws, u_s with the carried (mean, m2) and the final mean and var;
  // per block of attributes, the level rows of the counts and of the code law
  DevBuf<double> d_pr_sig, d_pf_u, d_pf_st, d_pf_law;
  DevBuf<uint64_t> d_pf_cnt;

  struct Cands;
  void need_emm();
  int need_predict(const uint8_t* codes, int64_t rows, bool partial = false);
  void predict_blocks(const uint8_t* codes, int64_t ny, int s0, int s1, const uint32_t* tab, int Ka, double* lpd,
                      double* p_new, double* coclass, double* ll, double* resp, bool miss = false);
  void impute_blocks(const uint8_t* codes, int64_t ny, int ld, double* pmf, double* lpd);
  int need(bool groups, bool tree);
  int check(const int32_t* cls, int ncand, int* Ka);
  template <class F>
  void blocks(Cands cd, int Ka, bool terms, bool want_all, bool reduce, F f);
  void losses(Cands cd, int Ka, double* vi_lb, double* vi, uint64_t* binder_A, uint64_t* binder_Q);
  void move_gains(const int32_t* cl, int Ka, int loss, int32_t* best, double* gain, double* full);
  double vi_of(const int32_t* c, int K);
  uint64_t binder_of(const int32_t* c, int K);
  int check_one(const int32_t* cl, int32_t Ka, int32_t loss);
  void merge_setup(const uint8_t* rows, int Ka, std::vector<uint64_t>& sz);
  void merge_gains(int loss, int Ka, int only, const std::vector<uint64_t>& sz, double* gain);
  void group_counts();
};

}  // namespace hdpm
