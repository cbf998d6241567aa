// ba_launch.h -- what ba_kernels.hip, the stage files of the reduced camera system (ba_structure.hip, ba_schur.hip, ba_pcg_precond.hip,
// ba_pcg.hip, ba_ppcg.hip, ba_dense.hip) and comm.cpp export to the bundle adjustment's host driver (ba_host.cpp).
// The defining files include it too, so the compiler checks every definition against the declaration the host calls: the
// library links with -shared, where a mismatch would otherwise be an undefined symbol nobody sees before load time.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "ba_types.h"

struct ccm_ctx;

// workgroups of b threads that cover n items (the launchers' grid size)
static inline int nblk(long long n, int b) { return (int)((n + b - 1) / b); }

// ---- comm.cpp
int comm_ranks(const ccm_ctx* c);
int comm_rank(const ccm_ctx* c);
int comm_allreduce_f64(ccm_ctx* c, double* dev, size_t n, bool max_op);
int comm_allreduce_u8_max(ccm_ctx* c, uint8_t* dev, size_t n);

// ---- ba_kernels.hip
void ba_launch_pose_rt(hipStream_t, const BaDev&);
void ba_launch_errors(hipStream_t, const BaDev&, double hd, double* partial, double* out);
void ba_launch_linearize(hipStream_t, const BaDev&, double hd, double lambda, bool keep_hpl, bool landmarks_only);
void ba_launch_lin_pose(hipStream_t, const BaDev&, double hd);
void ba_launch_index_check(hipStream_t, const int* edge_pose, const int* edge_point, int E, int P, int L, int* flags, int* pt_first);
void ba_launch_index_pose_keys(hipStream_t, const int* edge_pose, const int* free_of, int E, int P, int nfree, unsigned* key, unsigned* val);
void ba_launch_index_pose_first(hipStream_t, const unsigned* skey, int E, int nfree, int* pose_first);
void ba_launch_backsub(hipStream_t, const BaDev&, double lambda);
void ba_launch_update(hipStream_t, const BaDev&, double* save_poses, double* save_points);
void ba_launch_errors_scale(hipStream_t, const BaDev&, double hd, double lambda, int add_pose_lambda, double* partial, double* out);
void ba_launch_diag(hipStream_t, const BaDev&, double* tmp_ll, double* pp_diag, double* out_ll_max);
void ba_launch_outliers(hipStream_t, const BaDev&, double th, uint8_t* flag);
void ba_launch_deactivate(hipStream_t, const BaDev&, const uint8_t* flag);

// ---- ba_table.hip: the table route's source (obs, info, points from handles and table) and sink (table positions, handle poses)
void ba_launch_gather_table(hipStream_t, const BaTableArgs&);
void ba_launch_publish_table(hipStream_t, const BaTableArgs&);

// ---- ba_structure.hip: scans and sorts, block structure of the reduced camera system
size_t sp_scan_temp_bytes(size_t n);
hipError_t sp_scan_int(hipStream_t, void* tmp, size_t tmp_bytes, const int* in, int* out, size_t n);
hipError_t sp_scan_flags(hipStream_t, void* tmp, size_t tmp_bytes, const uint8_t* in, int* out, size_t n);
size_t sp_sort_temp_bytes(size_t n);
hipError_t sp_sort_u64(hipStream_t, void* tmp, size_t tmp_bytes, const unsigned* kin, unsigned* kout, const unsigned long long* vin,
                       unsigned long long* vout, size_t n, int bits);
hipError_t sp_sort_u32(hipStream_t, void* tmp, size_t tmp_bytes, const unsigned* kin, unsigned* kout, const unsigned* vin, unsigned* vout, size_t n);
void sp_launch_pair_count(hipStream_t, const BaDev&, int* cnt);
void sp_launch_pair_fill(hipStream_t, const BaDev&, const int* off, unsigned* key, unsigned long long* val);
void sp_launch_mark(hipStream_t, const unsigned* key, long long np, int nfree, uint8_t* map);
void sp_launch_block_coords(hipStream_t, const uint8_t* map, const int* id, long long n2, int nfree, int* br, int* bc, int* diag);
void sp_launch_pair_block(hipStream_t, const unsigned* key, const int* id, long long np, unsigned* out);
void sp_launch_seg_bounds(hipStream_t, const unsigned* sk, long long np, int* st, int* en);
void sp_launch_row_entries(hipStream_t, const int* br, const int* bc, int nb, int nfree, unsigned* key, unsigned* val);
void sp_launch_row_ptr(hipStream_t, const unsigned* skey, int n_ent, int nfree, int* row_ptr);
// ---- ba_schur.hip: one LM trial's Schur complement
void sp_launch_dinv(hipStream_t, const BaDev&, double lambda);
void sp_launch_schur_blocks(hipStream_t, const BaDev&, const double* Y, const unsigned long long* pairs, const int* st, const int* en,
                            const int* br, const int* bc, int nb, double* Hb);
void sp_launch_bschur(hipStream_t, const BaDev&, double* bs);
void sp_launch_add_lambda(hipStream_t, const int* diag, int nfree, double lambda, double* Hb);
void sp_launch_to_dense(hipStream_t, const double* Hb, const int* br, const int* bc, int nb, long long n, double* Hs);
// ---- ba_dense.hip: dense solves, in-place inverse of an SPD matrix
int dense_small_max();
int dense_launch_small_solve(hipStream_t, const double* Hb, const int* blk_row, const int* blk_col, int nb, int n, const double* b, double* x, int* bad, double lambda);
int dense_pitch(long long n);
void dense_launch_solve(hipStream_t, double* A, int n, int lda, const double* b, double* x, int* bad);
void dense_launch_invert(hipStream_t, double* A, int ncp, double* D, int* bad);
// ---- ba_pcg_precond.hip: both preconditioner levels (cluster inverses; coarse matrix and its sizes)
size_t pcg_minv_bytes(int nfree);
hipError_t pcg_launch_minv(hipStream_t, const double* Hb, const int* blk_row, const int* blk_col, int nb, int nfree, double* Minv, int* bad);
int pcg_coarse_dim(int nfree);
int pcg_coarse_pitch(int nfree);
int pcg_coarse_parts(int nfree);
int pcg_coarse_aggregates(int nfree);
int pcg_coarse_agg_keyframes(int nfree);
void pcg_launch_coarse_mark(hipStream_t, const int* blk_row, const int* blk_col, int nb, int nfree, uint8_t* aggmap);
hipError_t pcg_launch_coarse_build(hipStream_t, const double* Hb, const uint8_t* map, const int* id, int nfree, const double* svec, const double* cen,
                                   const int* pairs, int npairs, double* Ac);
void pcg_launch_coarse_complete(hipStream_t, double* A, int nc, int ncp);
void pcg_launch_coarse_mirror(hipStream_t, double* A, int ncp);
// ---- ba_pcg.hip: PCG, classic iteration
size_t pcg_part_doubles(int nfree);             // partial sums of the iteration's dot products
size_t pcg_coarse_rpart_doubles(int nfree);     // block partials of the restricted residual P^T r (PcgCoarse::rc)
void pcg_launch_init(hipStream_t, const double* b, const double* Minv, int nfree, double* w, double* part, double* sc, const PcgCoarse& C);
void pcg_launch_iter(hipStream_t, const double* Hb, const int* row_ptr, const unsigned* ekey, const unsigned* eval, const double* Minv,
                     int nfree, double* w, double* pap_part, double* part, double* sc, int parity, const PcgCoarse& C);
void pcg_launch_publish(hipStream_t, int nfree, double* part, double* sc, const PcgCoarse& C);
// ---- ba_ppcg.hip: pipelined PCG
size_t ppcg_state_doubles(int nfree);
size_t ppcg_ca_doubles(int nfree);
bool ppcg_supported(int nfree);
void ppcg_launch_expand(hipStream_t, const double* Hb, const unsigned* ekey, const unsigned* eval, int n_ent, int nfree, double* Hf, int* ecol);
hipError_t ppcg_launch_init(hipStream_t, const double* b, const double* Minv, const int* row_ptr, int nfree, double* wb, double* part, double* sc,
                            const PcgCoarse& C, const PpcgBufs& B);
void ppcg_launch_iter(hipStream_t, const double* Minv, const int* row_ptr, int nfree, double* wb, double* part, double* sc, const PcgCoarse& C, const PpcgBufs& B);
void ppcg_launch_publish(hipStream_t, const double* part, int nfree, double* sc);
