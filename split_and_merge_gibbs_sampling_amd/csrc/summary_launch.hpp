// summary_launch.hpp -- launchers of the posterior-summary kernels: posterior.hip
// (launch_psm, launch_vi_terms), trace_summary.hip (launch_tr_pack .. launch_tr_reduce,
// launch_tg_*) and trace_uncertainty.hip (launch_tr_transpose, launch_tr_affinity,
// launch_tr_cross).  Included by the units that define them and by summary_host.cpp, their
// only caller.
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

}  // namespace hdpm
