// ess_types.h -- launchers of ess_kernels.hip, shared with ess_host.cpp.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

void ess_launch_errors(hipStream_t, int ne, const int* ei, const int* ej, const double* meas, const double* sim3, const uint8_t* fixed, int fix_scale,
                       int variants, double* err);
void ess_launch_blocks(hipStream_t, int ne, int nv, const int* fidx, const int* inc_ptr, const int* inc_list, const double* err, double* blocks,
                       double* grad, double* b);
void essp_launch_assemble(hipStream_t, int ntargets, int ncol, const int* aptr, const int* alist, const double* blocks, double* D, double* Lb);
void essp_launch_factor_round(hipStream_t, const int* cols, int n, const int* colptr, int ncol, const int* tptr, const int* tpa, const int* tpb,
                              double lambda, double* D, double* Lb, int* bad);
void essp_launch_forward_round(hipStream_t, const int* cols, int n, const int* perm, const int* rptr, const int* rslot, const int* rcol,
                               const double* D, const double* Lb, const double* b, double* y);
void essp_launch_backward_round(hipStream_t, const int* cols, int n, const int* perm, const int* colptr, const int* rowidx, const double* D,
                                const double* Lb, const double* y, double* xp, double* x);
void ess_launch_update(hipStream_t, int nv, const int* fidx, const double* x, int fix_scale, double* sim3);
void ess_launch_chi2(hipStream_t, int ne, const double* err, int stride, double* part, double* out);
void ess_launch_correct(hipStream_t, int np, const int* ref, const double* s_old, const double* s_new, double* pts);
