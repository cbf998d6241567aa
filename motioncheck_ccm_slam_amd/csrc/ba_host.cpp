// ba_host.cpp -- Levenberg-Marquardt driver of the reprojection BA and its C ABI (include/ccm_hot.h).
//
// Mirrors, step for step, what the reference runs through g2o for Optimizer::BundleAdjustmentClient,
// LocalBundleAdjustmentClient and MapFusionGBA (src/Optimizer.cpp:32-212, 349-644, 646-865):
//   SparseOptimizer::optimize            cslam/thirdparty/g2o/g2o/core/sparse_optimizer.cpp:354-419
//   OptimizationAlgorithmLevenberg::solve  .../core/optimization_algorithm_levenberg.cpp:61-189
//   BlockSolver<6,3>::buildSystem/solve  .../core/block_solver.hpp:354-486, 502-604
// The reduced camera system is solved by a dense inverse (in-house block Gauss-Jordan, ba_dense.hip) for small maps and
// by a two-level preconditioned CG on the packed blocks for large ones, in place of LinearSolverEigen's SimplicialLDLT
// (solvers/linear_solver_eigen.h:106-136): any SPD solve of sufficient accuracy is equivalent up to rounding.  With an RCCL communicator attached (ccm_comm_init) the landmarks are
// sharded over the ranks and the reduced system is summed with one all-reduce per LM trial.
#include "ccm_internal.h"
#include "ba_types.h"
#include "ba_math.h"
#include "ba_launch.h"
#include "ba_index.h"
#include "ba_table.h"
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <thread>

struct BaState {
    hipStream_t side = nullptr;            // coarse-level inversion, concurrent with the PCG of the current trial
    hipEvent_t ev_hb = nullptr;            // the side stream has finished reading the reduced system
    hipEvent_t ev_inv = nullptr;           // the side stream has finished an inversion
    hipEvent_t ev_up = nullptr;            // the side stream has finished uploading observations, information values and points
    hipEvent_t ev_copy = nullptr;          // the main stream has copied the last inverse out of the side stream's work matrix
    hipEvent_t ev_chi = nullptr;           // a trial's chi2 has reached the host (the stream goes on with the next iteration's pose-side linearisation)
    std::vector<hipEvent_t> clock_ev;      // phase timers of large problems (events instead of stream synchronisations)
    double* pinned = nullptr;          // PIN_COUNT doubles of page-locked host memory for small device->host reads (slots: PIN_*)
    DevBuf poses, Rt, intr, free_of, pose_of_free, points, edge_pose, edge_point, obs, info, active, err,
           pt_first, pose_first, pose_edges, Hpp, bp, Hpp2, bp2, Hll, bl, Hpl, Dinv, Hs, x, save_poses, save_points,
           partial, scal, flags, info_dev, tmp_ll, pp_diag, gather,
           sp_cnt, sp_off, sp_key, sp_val, sp_key2, sp_val2, sp_map, sp_id, sp_tmp, blk_row, blk_col, diag_id, seg_start, seg_end,
           ent_key, ent_val, ent_key2, ent_val2, row_ptr, Hb, Y, db, Minv, pcg_w, pcg_pap, pcg_part, pcg_sc, pcg_aci, pcg_coarse, pcg_acw, pcg_svec, pcg_hf, pcg_ecol, pcg_ca, pcg_aggmap, pcg_pairs, ce;
};
void ba_state_free(BaState* s)
{
    if (!s) return;
    if (s->side) (void)hipStreamSynchronize(s->side);
    if (s->ev_hb) (void)hipEventDestroy(s->ev_hb);
    if (s->ev_inv) (void)hipEventDestroy(s->ev_inv);
    if (s->ev_up) (void)hipEventDestroy(s->ev_up);
    if (s->ev_copy) (void)hipEventDestroy(s->ev_copy);
    if (s->ev_chi) (void)hipEventDestroy(s->ev_chi);
    for (hipEvent_t e : s->clock_ev) (void)hipEventDestroy(e);
    if (s->pinned) (void)hipHostFree(s->pinned);
    delete s;
}

extern "C" {

int ccm_pose_from_mat4f(const float* T, double* pose)
{
    if (!T || !pose) return CCM_E_ARG;
    double R[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i * 3 + j] = (double)T[i * 4 + j];   // Converter.cc:40-56
    ba_R_to_quat(R, pose);
    ba_quat_normalize(pose);
    for (int i = 0; i < 3; i++) pose[4 + i] = (double)T[i * 4 + 3];
    return CCM_OK;
}

int ccm_pose_to_mat4f(const double* pose, float* T)
{
    if (!T || !pose) return CCM_E_ARG;
    double R[9];
    ba_quat_to_R(pose, R);                                                                     // Converter.cc:86-93
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[i * 4 + j] = (float)R[i * 3 + j];
        T[i * 4 + 3] = (float)pose[4 + i];
    }
    T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
    return CCM_OK;
}

// Landmark ranges of the ranks of a sharded global BA: contiguous, balanced by the Schur cost
// k(k+1)/2 + k + 1 of a k-observation landmark.  cuts[r] .. cuts[r+1]-1 belong to rank r.  Host only.
int ccm_ba_landmark_cuts(const int32_t* edge_point, int n_edges, int n_points, int n_ranks, int32_t* cuts)
{
    if (!cuts || n_ranks < 1 || n_points < 0 || n_edges < 0 || (n_edges > 0 && !edge_point)) return CCM_E_ARG;
    std::vector<int> deg(n_points, 0);
    for (int e = 0; e < n_edges; e++) {
        if (edge_point[e] < 0 || edge_point[e] >= n_points) return CCM_E_ARG;
        deg[edge_point[e]]++;
    }
    double total = 0;
    for (int l = 0; l < n_points; l++) total += 0.5 * deg[l] * (deg[l] + 1) + deg[l] + 1;
    for (int r = 0; r <= n_ranks; r++) cuts[r] = n_points;
    cuts[0] = 0;
    double acc = 0;
    int r = 0;
    for (int l = 0; l < n_points; l++) {
        acc += 0.5 * deg[l] * (deg[l] + 1) + deg[l] + 1;
        while (r + 1 < n_ranks && acc >= total * (r + 1) / n_ranks) cuts[++r] = l + 1;
    }
    return CCM_OK;
}

}  // extern "C"

namespace {
using clk = std::chrono::steady_clock;
inline double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// ---- environment switches of the BA, read in this one place.  All but CCM_DEBUG are read once per process.
struct BaEnv {
    bool host_index_only;      // CCM_BA_HOST_INDEX=1: never index the edge list on the device
    bool split_off;            // CCM_BA_SPLIT_UPLOAD=0: no upload on the auxiliary stream
    bool force_timers;         // CCM_BA_TIMERS=1: per-phase event timers on small problems too
    int dense_max;             // CCM_BA_DENSE_MAX: largest reduced system solved densely
    bool want_coarse;          // CCM_PCG_COARSE=0: the cluster level alone
    double pcg_tol;            // CCM_PCG_TOL: overrides ccm_ba_options.pcg_tol when > 0
    bool no_ahead;             // CCM_BA_NO_LOOKAHEAD=1: test / A-B switch
    bool keep_hpl;             // CCM_BA_KEEP_HPL=1: test / A-B switch
    int reject_at;             // CCM_BA_TEST_REJECT_AT=N: test switch, -1 = not set
};
const BaEnv& ba_env()
{
    static const BaEnv env = [] {
        auto num = [](const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; };
        BaEnv e;
        e.host_index_only = num("CCM_BA_HOST_INDEX", 0) != 0;
        e.split_off = num("CCM_BA_SPLIT_UPLOAD", 1) == 0;
        e.force_timers = num("CCM_BA_TIMERS", 0) != 0;
        e.dense_max = num("CCM_BA_DENSE_MAX", 1536);
        e.want_coarse = num("CCM_PCG_COARSE", 1) != 0;
        e.pcg_tol = getenv("CCM_PCG_TOL") ? atof(getenv("CCM_PCG_TOL")) : 0.0;
        e.no_ahead = num("CCM_BA_NO_LOOKAHEAD", 0) != 0;
        e.keep_hpl = num("CCM_BA_KEEP_HPL", 0) != 0;
        e.reject_at = num("CCM_BA_TEST_REJECT_AT", -1);
        return e;
    }();
    return env;
}
bool ba_env_debug() { return getenv("CCM_DEBUG") != nullptr; }      // per call

// ---- slots of the page-locked scratch (BaState::pinned, doubles) and of the device scalars they mirror (BaState::scal, doubles;
//      BaState::info_dev, ints)
enum {
    PIN_PCG_SC = 0,            // [0..4] the PCG's published scalars ([1] |b|^2, [2] |r|^2, [3] p.Ap)
    PIN_CHI2 = 8,              // chi2, then PIN_SCALE and PIN_STOP: one copy of scal[0..2]
    PIN_SCALE = 9,
    PIN_STOP = 10,             // the collective stop flag as it came back
    PIN_PCG_BAD = 11,          // (int) a cluster of the preconditioner was not positive definite
    PIN_X_OK = 12,             // rank 0's verdict on the solve, out and back
    PIN_STOP_LOCAL = 13,       // this rank's sample of the stop flag on its way up
    PIN_DENSE_INFO = 14,       // (int) verdict of the dense solve
    PIN_COARSE_INFO = 15,      // (int) verdict of the coarse inversion
    PIN_COUNT = 16,
};
enum { SCAL_CHI2 = 0, SCAL_SCALE = 1, SCAL_STOP = 2, SCAL_X_OK = 3, SCAL_HLL_MAX = 5 };      // stop flag: collective; x ok: rank 0's verdict
enum { INFO_DENSE = 0, INFO_MINV = 1, INFO_COARSE = 4, INFO_INDEX = 8 };                     // INFO_INDEX: two ints (unsorted, lowest bad edge)

// Chunk lengths of the PCG graphs (even: the r.z slot parity is the same at the start of every chunk): graphs of 8 and of 2 iterations; a host
// round trip launches as many of them as the contraction observed so far says are still needed (rounded up to 2), then one
// and looks again (k_pcg_direction publishes the scalars after every iteration) -- with the hat-function coarse level a trial takes 20-100 iterations of 45 us, so
// iterations past convergence cost more than round trips.
constexpr int pcg_len[2] = {8, 2};

// How one run of the PCG iteration ended.  Device and communication failures do not travel here: they are the CCM code the run returns.
enum class PcgStatus {
    converged,
    not_positive_definite,     // (or, pipelined, the recurrences broke down)
    no_convergence,
    stale_coarse,              // the coarse inverse this trial was to use came from a system that was not positive definite: run again without it
};

// one trial's PCG: what pcg_run and start_inversion share
struct PcgTrial {
    bool coarse_unverified = false;        // the verdict of the inversion whose inverse this trial uses has not been read yet
    bool side_todo = false;                // this trial's system is still to start the next inversion
    double inv_host_ms = 0;
    int itc = 0, max_it = 0;
    double tol2 = 0;
};

// the LM loop's state (optimization_algorithm_levenberg.cpp:61-189)
struct BaLm {
    double huber = 0;                      // across the stages
    bool first_eval = true;
    int stage = 0, iterations = 0;         // this stage
    double lambda = 0, ni = 2;
    bool ahead_ready = false;              // Hpp_alt / bp_alt hold the pose side of the current state
    int it = 0;                            // this iteration
    double currentChi = 0;
    bool landmark_share_ready = false, hpl_valid = true;
    int qmax = 0;
    double rho = 0;
};

// Everything the stages of one ccm_ba_solve call share.  Its destructor runs however the call is left.
struct BaCall {
    ccm_ctx* const c;
    BaState& S;
    ccm_ba_problem* const pb;
    const ccm_ba_options* const opt;
    ccm_ba_result local_res{};
    ccm_ba_result* res;
    uint8_t* outlier_out;
    BaTableRoute* const route;             // nullptr: the caller's arrays are source and sink
    const hipStream_t st;
    const int ranks, rank;
    const BaEnv& env = ba_env();
    const bool debug = ba_env_debug();
    clk::time_point t_lap = clk::now();
    // sizes: poses, landmarks and edges of the problem; this rank's landmarks [l0, l1) and edges; free poses, unknowns of the reduced
    // system; blocks and landmark pairs of its pattern
    const int P, Lall, Eall;
    int l0 = 0, l1 = 0, L = 0, E = 0, nfree = 0, nb = 0;
    long long n = 0, NP = 0;
    std::vector<int> free_of, pose_of_free;
    bool dev_indexed = false, split_up = false;
    BaEdgeIndex ix;                        // owns the staging copies the uploads read
    hipStream_t up_stream = nullptr;       // copies out of the caller's arrays are queued there ...
    hipEvent_t up_event = nullptr;         // ... and this event follows the last of them
    bool st_reads_host = false;            // uploads queued on st have not been waited for yet
    BaDev D{};
    double* scal = nullptr;                // SCAL_*
    double* partial = nullptr;
    int* info_dev = nullptr;               // INFO_*
    double* Hb = nullptr;                  // packed blocks of the reduced system, then its right-hand side (D.bs)
    // solver choices
    bool use_pcg = false, small_solve = false, pipelined = false, fine_timers = false;
    double pcg_tol = 0;
    int nc = 0, ncp = 0, n_coarse_pairs = 0;
    PcgCoarse PC{}, PC0{};                 // both levels / the cluster level alone (first trial of a call: no coarse inverse exists yet)
    PpcgBufs PB{};
    // Graphs: [level][length]; level 0 = the cluster level alone, 1 = both levels.
    hipGraph_t pcg_graph[4] = {nullptr, nullptr, nullptr, nullptr};
    hipGraphExec_t pcg_exec[4] = {nullptr, nullptr, nullptr, nullptr};
    hipGraph_t inv_graph = nullptr;
    hipGraphExec_t inv_exec = nullptr;
    // side stream
    bool hb_in_use = false;                                // the side stream is still reading this trial's reduced system
    bool coarse_ready = false, coarse_pending = false;     // an inverse is in Aci / an inversion is running on the side stream
    bool copy_recorded = false;                            // ev_copy has been recorded in this call
    bool stop_collective = false;
    double* Hpp_alt = nullptr;             // the look-ahead's second pair of buffers
    double* bp_alt = nullptr;
    std::vector<int> clock_phase;          // phase the interval ENDING at event i belongs to (-1: none)

    BaCall(ccm_ctx* ctx, ccm_ba_problem* problem, const ccm_ba_options* options, ccm_ba_result* result, BaTableRoute* table_route)
        : c(ctx), S(*ctx->ba), pb(problem), opt(options), res(result ? result : &local_res), outlier_out(res->edge_outlier), route(table_route), st(ctx->stream),
          ranks(comm_ranks(ctx)), rank(comm_rank(ctx)), P(problem->n_poses), Lall(problem->n_points), Eall(problem->n_edges)
    {
        *res = ccm_ba_result{};
        res->edge_outlier = outlier_out;
    }
    BaCall(const BaCall&) = delete;
    BaCall& operator=(const BaCall&) = delete;
    ~BaCall()
    {
        // whatever way the call is left, the copies out of the caller's arrays and out of ix have finished by then
        if (up_event) (void)hipEventSynchronize(up_event);
        else if (up_stream) (void)hipStreamSynchronize(up_stream);             // left between the first copy and the event
        if (st_reads_host) (void)hipStreamSynchronize(st);                      // left between an upload and the stage's own synchronisation
        for (int i = 0; i < 4; i++) { if (pcg_exec[i]) (void)hipGraphExecDestroy(pcg_exec[i]); if (pcg_graph[i]) (void)hipGraphDestroy(pcg_graph[i]); }
        if (inv_exec) (void)hipGraphExecDestroy(inv_exec);
        if (inv_graph) (void)hipGraphDestroy(inv_graph);
    }

    template <class T> int upload(DevBuf& b, const T* src, size_t count) { return ccm_upload(c, b, src, count * sizeof(T), st); }
    volatile int& pinned_int(int slot) { return *reinterpret_cast<volatile int*>(S.pinned + slot); }    // pinned: a copy to pageable memory would synchronise
    bool stop_flag_set() const { return opt->stop_flag && *opt->stop_flag; }
    void lap(const char* what);
    void tick(int phase);

    // set-up, in the order ba_solve_impl runs it
    int vertex_maps_and_shard();
    int index_on_device();
    int index_on_host();
    int upload_problem();
    int gather_problem();
    int reserve_workspace();
    int build_block_structure();
    int select_solver();
    void capture_graphs();
    int list_coarse_pairs();
    // LM loop
    bool stop_requested() const { return ranks > 1 ? stop_collective : stop_flag_set(); }
    int sync_stop();
    int eval_chi2(double hd, bool with_scale, double lambda, double* chi, double* scale, bool rt_current = false, bool look_ahead = false);
    int compute_lambda_init(BaLm& lm);
    int schur_step(BaLm& lm);
    int start_inversion(PcgTrial& t);
    int pcg_run(PcgTrial& t, bool pip, PcgStatus* status);
    int solve_pcg(const BaLm& lm, clk::time_point t2, int* ok2, bool* solved);
    int solve_dense(double lambda, int* ok2, bool* dense_info_pending);
    int share_increment(int* ok2);
    int lm_trial(BaLm& lm);
    int lm_stage(BaLm& lm);
    int lm_loop();
    // results
    int read_phase_timers();
    int download();
    int publish();
};

void BaCall::lap(const char* what)
{
    if (!debug) return;
    (void)hipStreamSynchronize(st);
    auto t = clk::now();
    fprintf(stderr, "[ccm] setup %-28s %.3f ms\n", what, std::chrono::duration<double>(t - t_lap).count() * 1e3);
    t_lap = t;
}

// Phase timers (t_linearize / t_schur / t_solve / t_update).  Small problems: host clock, booked where the next necessary
// synchronisation falls.  Large ones (fine_timers): an event on the stream at every phase boundary, read once at the end of the
// call -- round 2 synchronised the stream there instead, four idle gaps of 20-30 us per LM trial once a trial took 3 ms.
void BaCall::tick(int phase)
{
    if (!fine_timers) return;
    const size_t i = clock_phase.size();
    if (i == S.clock_ev.size()) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return; S.clock_ev.push_back(e); }
    if (hipEventRecord(S.clock_ev[i], st) == hipSuccess) clock_phase.push_back(phase);
}

// argument checks; the context's BA state, created on first use
int ba_begin(ccm_ctx* c, const ccm_ba_problem* pb, const ccm_ba_options* opt, bool values_on_device)
{
    if (!c || !pb || !opt) return CCM_E_ARG;
    if (pb->n_poses <= 0 || pb->n_points < 0 || pb->n_edges < 0 || !pb->poses || !pb->intr || (pb->n_edges > 0 && (!pb->edge_pose || !pb->edge_point)) ||
        (!values_on_device && ((pb->n_points > 0 && !pb->points) || (pb->n_edges > 0 && (!pb->obs || !pb->info)))))
        return ccm_fail(c, CCM_E_ARG, "bad BA problem");
    // (every edge's vertex indices are range-checked by the first pass over the edge list, before anything indexes with them)
    CCM_HIP(c, hipSetDevice(c->device));
    if (!c->ba) c->ba = new BaState();
    BaState& S = *c->ba;
    if (!S.pinned && hipHostMalloc((void**)&S.pinned, PIN_COUNT * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        S.pinned = nullptr;
        return ccm_fail(c, CCM_E_NOMEM, "hipHostMalloc failed");
    }
    if (S.side) CCM_HIP(c, hipStreamSynchronize(S.side));      // an earlier call that ended on an error may have left work there
    return CCM_OK;
}

int BaCall::vertex_maps_and_shard()
{
    // ---- vertices
    free_of.resize(P);
    for (int p = 0; p < P; p++) {
        const bool fx = pb->fixed && pb->fixed[p];
        free_of[p] = fx ? -1 : (int)pose_of_free.size();
        if (!fx) pose_of_free.push_back(p);
    }
    nfree = (int)pose_of_free.size();
    n = 6LL * nfree;
    // ---- landmark shard of this rank: contiguous range balanced by Schur cost k(k+1)/2 + k
    l0 = 0; l1 = Lall;
    if (ranks > 1) {
        std::vector<int32_t> cut(ranks + 1);
        if (ccm_ba_landmark_cuts(pb->edge_point, Eall, Lall, ranks, cut.data())) return ccm_fail(c, CCM_E_ARG, "an edge references a landmark out of range");
        l0 = cut[rank]; l1 = cut[rank + 1];
    }
    L = l1 - l0;
    return CCM_OK;
}

// Large unsharded maps: the raw edge list goes up as it is, and the device checks it (vertex ranges, order) and makes the index
// structures (landmark -> edges, free keyframe -> edges by a stable radix sort).  A list that turns out unsorted takes the host path.
int BaCall::index_on_device()
{
    int rc;
    if (!(ranks == 1 && Eall >= 400000 && nfree > 0 && Lall > 0 && !env.host_index_only) || route) return CCM_OK;
    st_reads_host = true;
    if ((rc = upload(S.free_of, free_of.data(), P))) return rc;
    if ((rc = upload(S.edge_pose, pb->edge_pose, Eall))) return rc;
    if ((rc = upload(S.edge_point, pb->edge_point, Eall))) return rc;
    CCM_RESERVE(c, S.pt_first, ((size_t)Lall + 2) * 4); CCM_RESERVE(c, S.pose_first, ((size_t)nfree + 2) * 4);
    CCM_RESERVE(c, S.pose_edges, (size_t)Eall * 4 + 16); CCM_RESERVE(c, S.info_dev, 64);
    CCM_RESERVE(c, S.sp_key, (size_t)Eall * 4 + 16); CCM_RESERVE(c, S.sp_key2, (size_t)Eall * 4 + 16); CCM_RESERVE(c, S.sp_off, (size_t)Eall * 4 + 16);
    const size_t ix_tmp = sp_sort_temp_bytes((size_t)Eall);
    CCM_RESERVE(c, S.sp_tmp, ix_tmp + 256);
    int* flags = S.info_dev.as<int>() + INFO_INDEX;
    const int init_flags[2] = { 0, 0x7FFFFFFF };
    CCM_HIP(c, hipMemcpyAsync(flags, init_flags, 8, hipMemcpyHostToDevice, st));
    ba_launch_index_check(st, S.edge_pose.as<int>(), S.edge_point.as<int>(), Eall, P, Lall, flags, S.pt_first.as<int>());
    ba_launch_index_pose_keys(st, S.edge_pose.as<int>(), S.free_of.as<int>(), Eall, P, nfree, S.sp_key.as<unsigned>(), S.sp_off.as<unsigned>());
    CCM_HIP(c, sp_sort_u32(st, S.sp_tmp.p, ix_tmp, S.sp_key.as<unsigned>(), S.sp_key2.as<unsigned>(), S.sp_off.as<unsigned>(),
                           S.pose_edges.as<unsigned>(), (size_t)Eall));
    ba_launch_index_pose_first(st, S.sp_key2.as<unsigned>(), Eall, nfree, S.pose_first.as<int>());
    int got[2] = { 0, 0 };
    CCM_HIP(c, hipMemcpyAsync(got, flags, 8, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipStreamSynchronize(st));
    st_reads_host = false;
    if (got[1] != 0x7FFFFFFF) return ccm_fail(c, CCM_E_ARG, "edge %d references a vertex out of range", got[1]);
    dev_indexed = got[0] == 0;
    return CCM_OK;
}

// the host's sort and index of this rank's edges (ba_index.h), unless the device has done it
int BaCall::index_on_host()
{
    if (dev_indexed) ix = BaEdgeIndex::unindexed(pb->edge_pose, pb->edge_point, pb->obs, pb->info, Eall);
    else {
        const int NT = Eall >= 400000 ? (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency())) : 1;
        ix = ba_index_edges(pb->edge_pose, pb->edge_point, pb->obs, pb->info, Eall, P, Lall, l0, l1, free_of.data(), nfree, NT);
        if (ix.out_of_range >= 0) return ccm_fail(c, CCM_E_ARG, "edge %lld references a vertex out of range", ix.out_of_range);
    }
    E = ix.E;
    // Per-phase timers need a stream synchronisation at every phase boundary.  On a large graph that costs nothing next to the phases; on a
    // local BA (tens of keyframes, launch-bound) the four extra round trips per LM trial were a quarter of the call, so small problems
    // skip them: their timers still add up to the wall time, but a phase's GPU time is booked where the next necessary sync happens.
    fine_timers = env.force_timers || E >= 200000;
    lap("host: sort + index edges");
    return CCM_OK;
}

// ---- device buffers: the problem and its index
int BaCall::upload_problem()
{
    int rc;
    if (route) return gather_problem();
    st_reads_host = true;                                      // until reserve_workspace has synchronised
    if ((rc = upload(S.poses, pb->poses, 7 * (size_t)P))) return rc;
    if ((rc = upload(S.intr, pb->intr, 4 * (size_t)P))) return rc;
    if ((rc = upload(S.pose_of_free, pose_of_free.data(), nfree))) return rc;
    // Large maps taken where they lie: observations, information values and points (48 of the 65 MB at config 5) are not needed
    // before the first linearisation, so they go up on the context's first auxiliary stream while this stream builds the block
    // structure of the reduced system from the index arrays (pair enumeration, radix sorts: 0.9 ms at config 5).
    split_up = ix.direct && ranks == 1 && Eall >= 400000 && nfree > 0 && !env.split_off;
    if (split_up) {
        hipStream_t up_st = ccm_aux_stream(c, 0);               // (the stream the coarse inversion uses later in the call: S.side)
        if (!up_st) return ccm_fail(c, CCM_E_DEVICE, "hipStreamCreate failed");
        if (!S.ev_up) CCM_HIP(c, hipEventCreateWithFlags(&S.ev_up, hipEventDisableTiming));
        CCM_RESERVE(c, S.points, std::max<size_t>(3 * (size_t)L * 8, 16)); CCM_RESERVE(c, S.obs, std::max<size_t>(2 * (size_t)E * 8, 16));
        CCM_RESERVE(c, S.info, std::max<size_t>((size_t)E * 8, 16));
        up_stream = up_st;                                      // from here on ~BaCall waits for what this stream has been given
        if (L) CCM_HIP(c, hipMemcpyAsync(S.points.p, pb->points + 3 * (size_t)l0, 3 * (size_t)L * 8, hipMemcpyHostToDevice, up_st));
        if (E) CCM_HIP(c, hipMemcpyAsync(S.obs.p, ix.e_obs, 2 * (size_t)E * 8, hipMemcpyHostToDevice, up_st));
        if (E) CCM_HIP(c, hipMemcpyAsync(S.info.p, ix.e_info, (size_t)E * 8, hipMemcpyHostToDevice, up_st));
        CCM_HIP(c, hipEventRecord(S.ev_up, up_st));
        up_event = S.ev_up;
    } else {
        if ((rc = upload(S.points, pb->points + 3 * (size_t)l0, 3 * (size_t)L))) return rc;
        if ((rc = upload(S.obs, ix.e_obs, 2 * (size_t)E))) return rc;
        if ((rc = upload(S.info, ix.e_info, E))) return rc;
    }
    if (!dev_indexed) {                                        // (the device path has these already)
        if ((rc = upload(S.free_of, free_of.data(), P))) return rc;
        if ((rc = upload(S.edge_pose, ix.e_pose, E))) return rc;
        if ((rc = upload(S.edge_point, ix.e_pt, E))) return rc;
        if ((rc = upload(S.pt_first, ix.pt_first.data(), L + 1))) return rc;
        if ((rc = upload(S.pose_first, ix.pose_first.data(), nfree + 1))) return rc;
        if ((rc = upload(S.pose_edges, ix.pose_edges.get(), ix.n_pose_edges))) return rc;
    }
    return CCM_OK;
}

// The table route's upload_problem: poses, intrinsics and the route's lists go up in its one staging copy, the index goes up as above,
// and observations, information values and points are gathered on the device (k_ba_gather_table) where the array route uploads them.
int BaCall::gather_problem()
{
    int rc;
    Staging& G = *route->G;
    BaTableArgs& A = route->A;
    int32_t* feat = G.host<int32_t>(route->o_feat);
    for (int k = 0; k < E; k++) feat[k] = route->obs_feat[ix.edge_id(k)];      // the device's edge order
    if ((rc = G.upload(c, route->in_begin, route->in_end))) return rc;
    CCM_RESERVE(c, S.poses, 7 * (size_t)P * 8); CCM_RESERVE(c, S.intr, 4 * (size_t)P * 8);
    CCM_RESERVE(c, S.points, std::max<size_t>(3 * (size_t)L * 8, 16)); CCM_RESERVE(c, S.obs, std::max<size_t>(2 * (size_t)E * 8, 16));
    CCM_RESERVE(c, S.info, std::max<size_t>((size_t)E * 8, 16));
    CCM_HIP(c, hipMemcpyAsync(S.poses.p, G.dev<double>(route->o_pose_in), 7 * (size_t)P * 8, hipMemcpyDeviceToDevice, st));
    CCM_HIP(c, hipMemcpyAsync(S.intr.p, G.dev<double>(route->o_intr), 4 * (size_t)P * 8, hipMemcpyDeviceToDevice, st));
    st_reads_host = true;                                      // until reserve_workspace has synchronised
    if ((rc = upload(S.pose_of_free, pose_of_free.data(), nfree))) return rc;
    if ((rc = upload(S.free_of, free_of.data(), P))) return rc;
    if ((rc = upload(S.edge_pose, ix.e_pose, E))) return rc;
    if ((rc = upload(S.edge_point, ix.e_pt, E))) return rc;
    if ((rc = upload(S.pt_first, ix.pt_first.data(), L + 1))) return rc;
    if ((rc = upload(S.pose_first, ix.pose_first.data(), nfree + 1))) return rc;
    if ((rc = upload(S.pose_edges, ix.pose_edges.get(), ix.n_pose_edges))) return rc;
    A.P = P; A.L = L; A.E = E;
    A.edge_pose = S.edge_pose.as<int>(); A.edge_feat = G.dev<int>(route->o_feat);
    A.poses = S.poses.as<double>(); A.points = S.points.as<double>(); A.obs = S.obs.as<double>(); A.info = S.info.as<double>();
    ba_launch_gather_table(st, A);
    CCM_HIP(c, hipGetLastError());
    return CCM_OK;
}

// the LM loop's workspace and the device view of the problem (D)
int BaCall::reserve_workspace()
{
    const size_t nxl = (size_t)n + 3 * (size_t)L;
    CCM_RESERVE(c, S.Rt, 12 * (size_t)P * 8);
    CCM_RESERVE(c, S.active, std::max<size_t>(E, 16)); CCM_RESERVE(c, S.flags, std::max<size_t>(E, 16));
    CCM_RESERVE(c, S.err, std::max<size_t>(2 * (size_t)E * 8, 16));
    CCM_RESERVE(c, S.Hpp, std::max<size_t>(36 * (size_t)nfree * 8, 16)); CCM_RESERVE(c, S.bp, std::max<size_t>((size_t)n * 8, 16));
    CCM_RESERVE(c, S.Hpp2, std::max<size_t>(36 * (size_t)nfree * 8, 16)); CCM_RESERVE(c, S.bp2, std::max<size_t>((size_t)n * 8, 16));   // the LM loop's look-ahead (eval_chi2)
    CCM_RESERVE(c, S.Hll, std::max<size_t>(9 * (size_t)L * 8, 16)); CCM_RESERVE(c, S.bl, std::max<size_t>(3 * (size_t)L * 8, 16));
    CCM_RESERVE(c, S.Hpl, std::max<size_t>(18 * (size_t)E * 8, 16)); CCM_RESERVE(c, S.Dinv, std::max<size_t>(9 * (size_t)L * 8, 16));
    CCM_RESERVE(c, S.x, std::max<size_t>(nxl * 8, 16));
    CCM_RESERVE(c, S.save_poses, 7 * (size_t)P * 8); CCM_RESERVE(c, S.save_points, std::max<size_t>(3 * (size_t)L * 8, 16));
    const size_t nb_max = (size_t)(E + 255) / 256 + (nxl + 255) / 256 + 8;             // (ba_launch_errors_scale keeps both kernels' partial sums)
    CCM_RESERVE(c, S.partial, nb_max * 8); CCM_RESERVE(c, S.scal, 64 * 8); CCM_RESERVE(c, S.info_dev, 64);
    CCM_RESERVE(c, S.tmp_ll, std::max<size_t>((size_t)L * 8, 16)); CCM_RESERVE(c, S.pp_diag, std::max<size_t>((size_t)n * 8, 16));
    CCM_HIP(c, hipMemsetAsync(S.active.p, 1, std::max(E, 1), st));
    CCM_HIP(c, hipMemsetAsync(S.err.p, 0, std::max<size_t>(2 * (size_t)E * 8, 16), st));
    CCM_HIP(c, hipMemsetAsync(S.x.p, 0, std::max<size_t>(nxl * 8, 16), st));
    CCM_HIP(c, hipStreamSynchronize(st));    // (the uploads on this stream have read the caller's arrays and ix by here)
    st_reads_host = false;
    lap("upload + allocate");

    D.P = P; D.L = L; D.E = E; D.nfree = nfree;
    D.poses = S.poses.as<double>(); D.Rt = S.Rt.as<double>(); D.intr = S.intr.as<double>();
    D.free_of = S.free_of.as<int>(); D.pose_of_free = S.pose_of_free.as<int>(); D.points = S.points.as<double>();
    D.edge_pose = S.edge_pose.as<int>(); D.edge_point = S.edge_point.as<int>(); D.obs = S.obs.as<double>(); D.info = S.info.as<double>();
    D.active = S.active.as<uint8_t>(); D.err = S.err.as<double>(); D.pt_first = S.pt_first.as<int>();
    D.pose_first = S.pose_first.as<int>(); D.pose_edges = S.pose_edges.as<int>();
    D.Hpp = S.Hpp.as<double>(); D.bp = S.bp.as<double>(); D.Hll = S.Hll.as<double>(); D.bl = S.bl.as<double>();
    D.Hpl = S.Hpl.as<double>(); D.Dinv = S.Dinv.as<double>();
    D.bs = nullptr; D.x = S.x.as<double>();
    scal = S.scal.as<double>();
    partial = S.partial.as<double>();
    info_dev = S.info_dev.as<int>();
    Hpp_alt = S.Hpp2.as<double>();
    bp_alt = S.bp2.as<double>();
    return CCM_OK;
}

// ---- block-sparse structure of the reduced camera system (once per call; see ba_structure.hip), and the PCG's buffers
int BaCall::build_block_structure()
{
    int rc;
    if ((long long)nfree * nfree >= (1LL << 32)) return ccm_fail(c, CCM_E_ARG, "too many free keyframes (%d) for 32-bit block keys", nfree);
    const long long n2 = (long long)nfree * nfree;
    if (nfree > 0) {
        // (both scans run over one item more than they count: the total lands behind the last prefix.  Sized for n2 items, rocPRIM
        // refused the n2 + 1 of the flag scan where n2 fills its last block exactly -- 256 free keyframes)
        const size_t scan_tmp = sp_scan_temp_bytes((size_t)std::max<long long>(n2 + 1, L + 1));
        CCM_RESERVE(c, S.sp_cnt, ((size_t)L + 2) * 4); CCM_RESERVE(c, S.sp_off, ((size_t)L + 2) * 4);
        CCM_RESERVE(c, S.sp_tmp, scan_tmp + 256);
        CCM_HIP(c, hipMemsetAsync(S.sp_cnt.p, 0, ((size_t)L + 2) * 4, st));
        if (L > 0) sp_launch_pair_count(st, D, S.sp_cnt.as<int>());
        CCM_HIP(c, sp_scan_int(st, S.sp_tmp.p, scan_tmp, S.sp_cnt.as<int>(), S.sp_off.as<int>(), (size_t)L + 1));
        int np_i = 0;
        CCM_HIP(c, hipMemcpyAsync(&np_i, S.sp_off.as<int>() + L, 4, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        NP = np_i;
        CCM_RESERVE(c, S.sp_key, std::max<size_t>((size_t)NP * 4, 16)); CCM_RESERVE(c, S.sp_val, std::max<size_t>((size_t)NP * 8, 16));
        CCM_RESERVE(c, S.sp_key2, std::max<size_t>((size_t)NP * 4, 16)); CCM_RESERVE(c, S.sp_val2, std::max<size_t>((size_t)NP * 8, 16));
        if (NP > 0) sp_launch_pair_fill(st, D, S.sp_off.as<int>(), S.sp_key.as<unsigned>(), S.sp_val.as<unsigned long long>());
        CCM_RESERVE(c, S.sp_map, (size_t)n2 + 16); CCM_RESERVE(c, S.sp_id, ((size_t)n2 + 2) * 4);
        CCM_HIP(c, hipMemsetAsync(S.sp_map.p, 0, (size_t)n2 + 16, st));
        sp_launch_mark(st, S.sp_key.as<unsigned>(), NP, nfree, S.sp_map.as<uint8_t>());
        if ((rc = comm_allreduce_u8_max(c, S.sp_map.as<uint8_t>(), (size_t)n2))) return rc;      // union pattern over ranks
        CCM_HIP(c, sp_scan_flags(st, S.sp_tmp.p, scan_tmp, S.sp_map.as<uint8_t>(), S.sp_id.as<int>(), (size_t)n2 + 1));
        CCM_HIP(c, hipMemcpyAsync(&nb, S.sp_id.as<int>() + n2, 4, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        CCM_RESERVE(c, S.blk_row, (size_t)nb * 4); CCM_RESERVE(c, S.blk_col, (size_t)nb * 4); CCM_RESERVE(c, S.diag_id, (size_t)nfree * 4);
        {
            // the scale columns of the prolongation: keyframe translations as they are now, and each aggregate's mean
            const int A = pcg_coarse_agg_keyframes(nfree), nagg = pcg_coarse_aggregates(nfree);
            std::vector<double> sv(3 * (size_t)nfree + 3 * (size_t)nagg, 0.0);
            for (int f = 0; f < nfree; f++) for (int q = 0; q < 3; q++) sv[3 * (size_t)f + q] = pb->poses[7 * (size_t)pose_of_free[f] + 4 + q];
            for (int I = 0; I < nagg; I++) {
                const int f0 = I * A, f1 = std::min(nfree, f0 + A);
                for (int q = 0; q < 3; q++) {
                    double m = 0;
                    for (int f = f0; f < f1; f++) m += sv[3 * (size_t)f + q];
                    sv[3 * (size_t)nfree + 3 * I + q] = m / std::max(1, f1 - f0);
                }
            }
            CCM_RESERVE(c, S.pcg_svec, sv.size() * 8 + 64);
            CCM_HIP(c, hipMemcpyAsync(S.pcg_svec.p, sv.data(), sv.size() * 8, hipMemcpyHostToDevice, st));
            CCM_HIP(c, hipStreamSynchronize(st));                                                         // sv is a local (the stream is idle here: nb has just been read)
        }
        sp_launch_block_coords(st, S.sp_map.as<uint8_t>(), S.sp_id.as<int>(), n2, nfree, S.blk_row.as<int>(), S.blk_col.as<int>(), S.diag_id.as<int>());
        // this rank's pairs sorted by target block (stable: fixed summation order)
        const size_t sort_tmp = sp_sort_temp_bytes((size_t)std::max<long long>(NP, 2LL * nb));
        CCM_RESERVE(c, S.sp_tmp, std::max(sort_tmp, scan_tmp) + 256);
        sp_launch_pair_block(st, S.sp_key.as<unsigned>(), S.sp_id.as<int>(), NP, S.sp_key2.as<unsigned>());
        int bits = 1; while ((1LL << bits) < nb + 1) bits++;
        if (NP > 0) CCM_HIP(c, sp_sort_u64(st, S.sp_tmp.p, sort_tmp, S.sp_key2.as<unsigned>(), S.sp_key.as<unsigned>(),
                                           S.sp_val.as<unsigned long long>(), S.sp_val2.as<unsigned long long>(), (size_t)NP, bits));
        CCM_RESERVE(c, S.seg_start, (size_t)nb * 4); CCM_RESERVE(c, S.seg_end, (size_t)nb * 4);
        CCM_HIP(c, hipMemsetAsync(S.seg_start.p, 0, (size_t)nb * 4, st)); CCM_HIP(c, hipMemsetAsync(S.seg_end.p, 0, (size_t)nb * 4, st));
        sp_launch_seg_bounds(st, S.sp_key.as<unsigned>(), NP, S.seg_start.as<int>(), S.seg_end.as<int>());
        // symmetric row lists for the mat-vec
        CCM_RESERVE(c, S.ent_key, (size_t)nb * 8); CCM_RESERVE(c, S.ent_val, (size_t)nb * 8);
        CCM_RESERVE(c, S.ent_key2, (size_t)nb * 8); CCM_RESERVE(c, S.ent_val2, (size_t)nb * 8);
        sp_launch_row_entries(st, S.blk_row.as<int>(), S.blk_col.as<int>(), nb, nfree, S.ent_key.as<unsigned>(), S.ent_val.as<unsigned>());
        CCM_HIP(c, sp_sort_u32(st, S.sp_tmp.p, sort_tmp, S.ent_key.as<unsigned>(), S.ent_key2.as<unsigned>(), S.ent_val.as<unsigned>(),
                               S.ent_val2.as<unsigned>(), (size_t)2 * nb));
        CCM_RESERVE(c, S.row_ptr, (size_t)nfree * 8);
        CCM_HIP(c, hipMemsetAsync(S.row_ptr.p, 0, (size_t)nfree * 8, st));
        sp_launch_row_ptr(st, S.ent_key2.as<unsigned>(), 2 * nb, nfree, S.row_ptr.as<int>());
        CCM_RESERVE(c, S.Hb, (36 * (size_t)nb + (size_t)n + 8) * 8);          // blocks, then bschur: one all-reduce covers both
        CCM_RESERVE(c, S.Minv, pcg_minv_bytes(nfree)); CCM_RESERVE(c, S.pcg_w, std::max(6 * (size_t)n, ppcg_state_doubles(nfree)) * 8 + 64);
        CCM_RESERVE(c, S.pcg_pap, (size_t)nfree * 8 + 64); CCM_RESERVE(c, S.pcg_part, pcg_part_doubles(nfree) * 8 + 64);
        CCM_RESERVE(c, S.pcg_sc, 64 * 8);
        {
            const size_t nc_ = (size_t)pcg_coarse_dim(nfree), ncp_ = (size_t)pcg_coarse_pitch(nfree);
            CCM_RESERVE(c, S.pcg_aci, ncp_ * ncp_ * 8 + 64); CCM_RESERVE(c, S.pcg_acw, (ncp_ * ncp_ + 48 * 48) * 8 + 64);   // + one block of scratch
            CCM_RESERVE(c, S.pcg_coarse, (pcg_coarse_rpart_doubles(nfree) + nc_ + (size_t)pcg_coarse_parts(nfree) + 64) * 8);   // P^T r, yc, cpart
        }
        CCM_HIP(c, hipGetLastError());
    }
    CCM_RESERVE(c, S.Y, std::max<size_t>(18 * (size_t)E * 8, 16)); CCM_RESERVE(c, S.db, std::max<size_t>(3 * (size_t)L * 8, 16));
    CCM_RESERVE(c, S.ce, std::max<size_t>(6 * (size_t)E * 8, 16));
    D.Z = S.Y.as<double>(); D.db = S.db.as<double>(); D.ce = S.ce.as<double>();
    Hb = S.Hb.as<double>();
    D.bs = nfree > 0 ? Hb + 36 * (size_t)nb : nullptr;
    res->schur_blocks = nb; res->schur_pairs = NP;
    return CCM_OK;
}

// which solver, which preconditioner levels, which iteration
int BaCall::select_solver()
{
    // dense solve for small systems (exact, and cheaper than PCG start-up), PCG on the packed blocks otherwise
    use_pcg = n > env.dense_max;
    // (a system small enough for k_dense_small_solve gets its damping there)
    small_solve = !use_pcg && n <= dense_small_max();
    // second preconditioner level (ba_pcg_precond.hip): on for systems with at least 64 coarse unknowns
    nc = nfree > 0 ? pcg_coarse_dim(nfree) : 0; ncp = nfree > 0 ? pcg_coarse_pitch(nfree) : 0;
    if (use_pcg && env.want_coarse && nc >= 64 && nc <= 2304) {      // beyond: the cubic inversion would outlast an LM trial (more than 24 576 free keyframes)
        if (!S.side) {
            // the context's low-priority auxiliary stream: the inversion has a whole LM trial to finish, the PCG kernels it shares the GPU
            // with are the critical path
            if (!(S.side = ccm_aux_stream(c, 0))) return ccm_fail(c, CCM_E_DEVICE, "hipStreamCreate failed");
            CCM_HIP(c, hipEventCreateWithFlags(&S.ev_hb, hipEventDisableTiming));
            CCM_HIP(c, hipEventCreateWithFlags(&S.ev_inv, hipEventDisableTiming));
            CCM_HIP(c, hipEventCreateWithFlags(&S.ev_copy, hipEventDisableTiming));
        }
        PC.Aci = S.pcg_aci.as<double>();
        PC.rc = S.pcg_coarse.as<double>();
        PC.yc = PC.rc + pcg_coarse_rpart_doubles(nfree);
        PC.cpart = PC.yc + nc;
        PC.svec = S.pcg_svec.as<double>();
        PC.cen = PC.svec + 3 * (size_t)nfree;
    }
    // Which iteration: the pipelined one (two kernels per iteration, ba_ppcg.hip) for the tolerances a BA asks for; its recurrences
    // stall near a relative residual of 1e-9, so a caller that wants more than 1e-7 gets the classic four-kernel iteration.
    pcg_tol = env.pcg_tol > 0 ? env.pcg_tol : (opt->pcg_tol > 0 ? opt->pcg_tol : 1e-7);   // relative residual (default: see ccm_hot.h)
    pipelined = use_pcg && nfree > 0 && ppcg_supported(nfree) && pcg_tol >= 1e-7;
    if (pipelined) {
        CCM_RESERVE(c, S.pcg_hf, 36 * 2 * (size_t)nb * 8 + 64); CCM_RESERVE(c, S.pcg_ecol, 2 * (size_t)nb * 4 + 64);
        CCM_RESERVE(c, S.pcg_ca, ppcg_ca_doubles(nfree) * 8 + 64);
        PB.Hf = S.pcg_hf.as<double>(); PB.ecol = S.pcg_ecol.as<int>(); PB.CA = S.pcg_ca.as<double>();
    }
    res->pcg_pipelined = pipelined ? 1 : 0;
    lap("block structure (pairs, sort)");
    return CCM_OK;
}

// The PCG inner loop is three or four small dependent kernels per iteration and is launch-bound when issued one by
// one: capture a chunk of iterations (+ the scalar publication) into a HIP graph and replay it (chunk lengths: pcg_len).
// A graph that cannot be captured is no error: its launches are issued one by one.
void BaCall::capture_graphs()
{
    // (Captured on the context's second auxiliary stream, which is idle, while the main stream is still sorting the pair lists: the 0.3 ms
    //  of host time the capture takes used to be idle time of the GPU.)
    hipStream_t cap_st = (use_pcg && nfree > 0) ? ccm_aux_stream(c, 1) : nullptr;
    if (cap_st) {
        for (int gi = 0; gi < (PC.Aci ? 4 : 2); gi++) {
            const PcgCoarse& pc = (gi >> 1) ? PC : PC0;
            if (hipStreamBeginCapture(cap_st, hipStreamCaptureModeRelaxed) == hipSuccess) {
                for (int k = 0; k < pcg_len[gi & 1]; k++) {
                    if (pipelined) ppcg_launch_iter(cap_st, S.Minv.as<double>(), S.row_ptr.as<int>(), nfree, S.pcg_w.as<double>(), S.pcg_part.as<double>(), S.pcg_sc.as<double>(), pc, PB);
                    else pcg_launch_iter(cap_st, Hb, S.row_ptr.as<int>(), S.ent_key2.as<unsigned>(), S.ent_val2.as<unsigned>(), S.Minv.as<double>(),
                                         nfree, S.pcg_w.as<double>(), S.pcg_pap.as<double>(), S.pcg_part.as<double>(), S.pcg_sc.as<double>(), k & 1, pc);
                }
                hipError_t e1 = hipStreamEndCapture(cap_st, &pcg_graph[gi]);
                hipError_t e2 = e1 == hipSuccess ? hipGraphInstantiate(&pcg_exec[gi], pcg_graph[gi], nullptr, nullptr, 0) : e1;
                if (e2 != hipSuccess) {
                    pcg_exec[gi] = nullptr;                     // fall back to plain launches
                    if (debug) fprintf(stderr, "[ccm] PCG graph capture failed: %s / %s\n", hipGetErrorString(e1), hipGetErrorString(e2));
                    (void)hipGetLastError();
                }
            } else { if (debug) fprintf(stderr, "[ccm] hipStreamBeginCapture failed\n"); (void)hipGetLastError(); }
            if (debug) fprintf(stderr, "[ccm] PCG graph %d %s\n", gi, pcg_exec[gi] ? "ready" : "not used");
        }
    }
    // The coarse inversion is 75 small launches (0.2 ms of host time per LM trial, during which the host does not answer the PCG's round
    // trips): captured once, replayed with one call.
    if (PC.Aci && use_pcg) {
        double* Aw = S.pcg_acw.as<double>();
        if (hipStreamBeginCapture(S.side, hipStreamCaptureModeRelaxed) == hipSuccess) {
            dense_launch_invert(S.side, Aw, ncp, Aw + (size_t)ncp * ncp, info_dev + INFO_COARSE);
            pcg_launch_coarse_mirror(S.side, Aw, ncp);
            hipError_t e1 = hipStreamEndCapture(S.side, &inv_graph);
            hipError_t e2 = e1 == hipSuccess ? hipGraphInstantiate(&inv_exec, inv_graph, nullptr, nullptr, 0) : e1;
            if (e2 != hipSuccess) { inv_exec = nullptr; (void)hipGetLastError(); }
        } else (void)hipGetLastError();
    }
}

// the aggregate pairs that hold a block (the grid of the coarse matrix's assembly): fixed for the call
int BaCall::list_coarse_pairs()
{
    if (PC.Aci) {
        std::vector<int> coarse_pairs;                         // (I, J), I <= J
        const int nagg = pcg_coarse_aggregates(nfree);
        CCM_RESERVE(c, S.pcg_aggmap, (size_t)nagg * nagg + 16);
        CCM_HIP(c, hipMemsetAsync(S.pcg_aggmap.p, 0, (size_t)nagg * nagg, st));
        pcg_launch_coarse_mark(st, S.blk_row.as<int>(), S.blk_col.as<int>(), nb, nfree, S.pcg_aggmap.as<uint8_t>());
        std::vector<uint8_t> am((size_t)nagg * nagg);
        CCM_HIP(c, hipMemcpyAsync(am.data(), S.pcg_aggmap.p, am.size(), hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        for (int I = 0; I < nagg; I++)
            for (int J = I; J < nagg; J++) if (am[(size_t)I * nagg + J]) { coarse_pairs.push_back(I); coarse_pairs.push_back(J); }
        CCM_RESERVE(c, S.pcg_pairs, coarse_pairs.size() * 4 + 16);
        CCM_HIP(c, hipMemcpyAsync(S.pcg_pairs.p, coarse_pairs.data(), coarse_pairs.size() * 4, hipMemcpyHostToDevice, st));
        CCM_HIP(c, hipStreamSynchronize(st));                  // coarse_pairs is a local
        n_coarse_pairs = (int)(coarse_pairs.size() / 2);
    }
    lap("PCG graph capture");
    return CCM_OK;
}

// *pbStopFlag (sparse_optimizer.cpp:376, optimization_algorithm_levenberg.cpp:149).  With several ranks the decision must be
// the same everywhere or a rank would leave the loop while the others wait in the next all-reduce: every rank's sample of
// its own flag rides on the chi2 all-reduce (a sum: non-zero = some rank saw it), and the loop tests that collective value
// (stop_requested).  sync_stop: a dedicated exchange where no chi2 evaluation precedes the test.
int BaCall::sync_stop()
{
    if (ranks <= 1) return CCM_OK;
    S.pinned[PIN_STOP_LOCAL] = stop_flag_set() ? 1.0 : 0.0;
    CCM_HIP(c, hipMemcpyAsync(scal + SCAL_STOP, S.pinned + PIN_STOP_LOCAL, 8, hipMemcpyHostToDevice, st));
    int r = comm_allreduce_f64(c, scal + SCAL_STOP, 1, false);
    if (r) return r;
    CCM_HIP(c, hipMemcpyAsync(S.pinned + PIN_STOP, scal + SCAL_STOP, 8, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipStreamSynchronize(st));
    stop_collective = S.pinned[PIN_STOP] > 0.0;
    return CCM_OK;
}

// chi2 (+ optionally scale) of the current state, summed over ranks
// Look-ahead of the LM loop (one rank): a trial is nearly always accepted, and the keyframes' side of the next linearisation (Hpp, bp)
// depends on nothing but the state the trial has just produced -- so it is enqueued right behind the trial's chi2, into a second pair
// of buffers, and runs while the host waits for the chi2 (an event, not the stream), decides and launches the landmark side.  An accepted
// trial's iteration swaps the buffers in and launches the landmarks alone; a rejected one never looks at them.  Same kernel on the same
// state: the values are those the iteration would have computed itself.
int BaCall::eval_chi2(double hd, bool with_scale, double lambda, double* chi, double* scale, bool rt_current, bool look_ahead)
{
    static_assert(SCAL_SCALE == SCAL_CHI2 + 1 && SCAL_STOP == SCAL_CHI2 + 2 && PIN_SCALE == PIN_CHI2 + 1 && PIN_STOP == PIN_CHI2 + 2, "one copy brings all three");
    if (!rt_current) ba_launch_pose_rt(st, D);                             // (k_ba_update leaves the matrices of the poses it moved)
    if (with_scale) ba_launch_errors_scale(st, D, hd, lambda, rank == 0 ? 1 : 0, partial, scal + SCAL_CHI2);
    else if (E > 0) ba_launch_errors(st, D, hd, partial, scal + SCAL_CHI2);
    else CCM_HIP(c, hipMemsetAsync(scal + SCAL_CHI2, 0, 8, st));
    if (ranks > 1) {
        if (!with_scale) CCM_HIP(c, hipMemsetAsync(scal + SCAL_SCALE, 0, 8, st));
        S.pinned[PIN_STOP_LOCAL] = stop_flag_set() ? 1.0 : 0.0;
        CCM_HIP(c, hipMemcpyAsync(scal + SCAL_STOP, S.pinned + PIN_STOP_LOCAL, 8, hipMemcpyHostToDevice, st));
        int r = comm_allreduce_f64(c, scal + SCAL_CHI2, 3, false);
        if (r) return r;
        CCM_HIP(c, hipMemcpyAsync(S.pinned + PIN_CHI2, scal + SCAL_CHI2, 24, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        stop_collective = S.pinned[PIN_STOP] > 0.0;
    } else {
        CCM_HIP(c, hipMemcpyAsync(S.pinned + PIN_CHI2, scal + SCAL_CHI2, with_scale ? 16 : 8, hipMemcpyDeviceToHost, st));
        if (look_ahead) {
            CCM_HIP(c, hipEventRecord(S.ev_chi, st));
            BaDev D2 = D;
            D2.Hpp = Hpp_alt; D2.bp = bp_alt;
            { ProfScope ps(c, CCM_PROF_BA_LINEARIZE); ba_launch_lin_pose(st, D2, hd); }
            CCM_HIP(c, hipEventSynchronize(S.ev_chi));             // (polling the event or the page-locked slots instead measured the same)
        } else CCM_HIP(c, hipStreamSynchronize(st));
    }
    *chi = S.pinned[PIN_CHI2]; if (scale) *scale = S.pinned[PIN_SCALE];
    return CCM_OK;
}

// computeLambdaInit
int BaCall::compute_lambda_init(BaLm& lm)
{
    int rc;
    ba_launch_diag(st, D, S.tmp_ll.as<double>(), S.pp_diag.as<double>(), scal + SCAL_HLL_MAX);
    if (L == 0) CCM_HIP(c, hipMemsetAsync(scal + SCAL_HLL_MAX, 0, 8, st));
    if ((rc = comm_allreduce_f64(c, scal + SCAL_HLL_MAX, 1, true))) return rc;
    if ((rc = comm_allreduce_f64(c, S.pp_diag.as<double>(), (size_t)n, false))) return rc;
    std::vector<double> dg((size_t)n + 1);
    CCM_HIP(c, hipMemcpyAsync(dg.data(), S.pp_diag.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipMemcpyAsync(&dg[n], scal + SCAL_HLL_MAX, 8, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipStreamSynchronize(st));
    double md = 0;
    for (double v : dg) md = std::max(md, std::fabs(v));
    lm.lambda = 1e-5 * md; lm.ni = 2;
    return CCM_OK;
}

// the reduced camera system of one trial: landmark inverses (unless the linearisation has made them), Schur blocks, right-hand side,
// the sum over the ranks, damping
int BaCall::schur_step(BaLm& lm)
{
    int rc;
    if (!lm.landmark_share_ready) {
        ProfScope ps(c, CCM_PROF_BA_DINV_Y);
        if (!lm.hpl_valid) {
            // a rejected trial of an iteration linearised without Hpl: the state is the linearisation point again (pop),
            // the pose matrices are the rejected trial's
            ba_launch_pose_rt(st, D);
            ba_launch_linearize(st, D, lm.huber, 0.0, true, true);
            lm.hpl_valid = true;
        }
        sp_launch_dinv(st, D, lm.lambda);
    }
    lm.landmark_share_ready = false;                          // a repeated trial has another lambda
    { ProfScope ps(c, CCM_PROF_BA_SCHUR_BLOCKS);
      sp_launch_schur_blocks(st, D, S.Y.as<double>(), S.sp_val2.as<unsigned long long>(), S.seg_start.as<int>(), S.seg_end.as<int>(),
                             S.blk_row.as<int>(), S.blk_col.as<int>(), nb, Hb); }
    { ProfScope ps(c, CCM_PROF_BA_BSCHUR); sp_launch_bschur(st, D, D.bs); }
    if ((rc = comm_allreduce_f64(c, Hb, 36 * (size_t)nb + (size_t)n, false))) return rc;
    if (!small_solve) sp_launch_add_lambda(st, S.diag_id.as<int>(), nfree, lm.lambda, Hb);
    return CCM_OK;
}

// The next inversion (assembly of Ac from this trial's system, block Gauss-Jordan: 68 small launches, 0.2 ms
// of host time) goes to the side stream right after this trial's first chunk of PCG iterations has been
// launched, so the host enqueues it while the GPU is already iterating.
int BaCall::start_inversion(PcgTrial& t)
{
    auto ti0 = clk::now();
    double* Aw = S.pcg_acw.as<double>();
    if (copy_recorded) CCM_HIP(c, hipStreamWaitEvent(S.side, S.ev_copy, 0));
    CCM_HIP(c, hipMemsetAsync(info_dev + INFO_COARSE, 0, 4, S.side));
    CCM_HIP(c, pcg_launch_coarse_build(S.side, Hb, S.sp_map.as<uint8_t>(), S.sp_id.as<int>(), nfree, PC.svec, PC.cen, S.pcg_pairs.as<int>(),
                                       n_coarse_pairs, Aw));
    CCM_HIP(c, hipEventRecord(S.ev_hb, S.side));                 // awaited before the next trial overwrites Hb
    hb_in_use = true;
    if (inv_exec) CCM_HIP(c, hipGraphLaunch(inv_exec, S.side));
    else {
        dense_launch_invert(S.side, Aw, ncp, Aw + (size_t)ncp * ncp, info_dev + INFO_COARSE);
        pcg_launch_coarse_mirror(S.side, Aw, ncp);
    }
    CCM_HIP(c, hipEventRecord(S.ev_inv, S.side));
    CCM_HIP(c, hipGetLastError());
    coarse_pending = true; t.side_todo = false;
    t.inv_host_ms = secs(ti0, clk::now()) * 1e3;
    return CCM_OK;
}

// One run of the iteration (pip: the pipelined one).  Returns a CCM code; *status is set when that is CCM_OK.
int BaCall::pcg_run(PcgTrial& t, bool pip, PcgStatus* status)
{
    int rc;
    volatile double* sc = S.pinned + PIN_PCG_SC;
    const volatile int& badh = pinned_int(PIN_PCG_BAD);
    const PcgCoarse& pcu = coarse_ready ? PC : PC0;
    const int glv = coarse_ready ? 2 : 0;
    if (pip) CCM_HIP(c, ppcg_launch_init(st, D.bs, S.Minv.as<double>(), S.row_ptr.as<int>(), nfree, S.pcg_w.as<double>(), S.pcg_part.as<double>(),
                                         S.pcg_sc.as<double>(), pcu, PB));
    else pcg_launch_init(st, D.bs, S.Minv.as<double>(), nfree, S.pcg_w.as<double>(), S.pcg_part.as<double>(), S.pcg_sc.as<double>(), pcu);
    int last_len = 0;
    double rr_prev = 0;
    for (;;) {
        CCM_HIP(c, hipMemcpyAsync(S.pinned + PIN_PCG_SC, S.pcg_sc.p, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        if (t.coarse_unverified) { t.coarse_unverified = false; if (pinned_int(PIN_COARSE_INFO) != 0) { *status = PcgStatus::stale_coarse; return CCM_OK; } }
        if (badh || !std::isfinite(sc[2])) { *status = PcgStatus::not_positive_definite; return CCM_OK; }
        // Convergence is looked at before the smallest p.Ap: the host looks once per chunk, and a system that converges within a few
        // iterations (one cluster: the preconditioner is the exact inverse) spends the rest of the chunk at rounding level, where the
        // residual underflows to zero (p = 0, p.Ap = 0) or the pipelined recurrences cancel.  While p.Ap <= 0 the classic kernels
        // take no step (alpha = 0) and the pipelined ones one of 1e-300 p, and |r|^2 follows every step that is taken, so it still
        // is the residual of x as far as the iteration knows it: a p.Ap <= 0 seen on the way is no verdict on the matrix then.
        // (In the pipelined solve sc[2] is the recurrence's |r|^2 -- see the TODO below -- so a breakdown of the recurrences with a
        // small recurrence residual is accepted as converged here, exactly as a run without breakdown is.)
        if (sc[2] <= t.tol2 * sc[1]) { *status = PcgStatus::converged; return CCM_OK; }
        if (!(sc[3] > 0.0)) { *status = PcgStatus::not_positive_definite; return CCM_OK; }
        // TODO (deferred: changes numerical behaviour): "At exit of a pipelined solve, at least once per trial or under CCM_DEBUG and in
        // tests, compute the true residual with one k_ppcg_row-style mat-vec."  sc[2] is the recurrence's |r|^2, which drifts.
        if (t.itc >= t.max_it) { *status = PcgStatus::no_convergence; return CCM_OK; }
        // iterations still needed if |r|^2 keeps contracting as over the last round trip; without an estimate
        // (first round trip, stagnation): 16, or 32 while there is no coarse level
        const double rr = sc[2], target = t.tol2 * sc[1];
        int need = coarse_ready ? 16 : 32;
        if (last_len > 0 && rr_prev > 0 && rr < rr_prev) {
            const double est = std::log(rr / target) / (std::log(rr_prev / rr) / last_len);
            need = (int)std::min(16.0, std::max(2.0, std::ceil(est)));       // (CG speeds up as it goes: a longer forecast overshoots)
        }
        const int n8 = need / pcg_len[0], n2 = (need - n8 * pcg_len[0] + pcg_len[1] - 1) / pcg_len[1];
        rr_prev = rr; last_len = n8 * pcg_len[0] + n2 * pcg_len[1];
        for (int which = 0; which < 2; which++) {
            hipGraphExec_t gexec = pip == pipelined ? pcg_exec[glv + which] : nullptr;     // the graphs hold the iteration chosen for this call
            for (int rpt = 0; rpt < (which ? n2 : n8); rpt++) {
                if (gexec) CCM_HIP(c, hipGraphLaunch(gexec, st));
                else
                    for (int k = 0; k < pcg_len[which]; k++) {
                        if (pip) ppcg_launch_iter(st, S.Minv.as<double>(), S.row_ptr.as<int>(), nfree, S.pcg_w.as<double>(), S.pcg_part.as<double>(), S.pcg_sc.as<double>(), pcu, PB);
                        else pcg_launch_iter(st, Hb, S.row_ptr.as<int>(), S.ent_key2.as<unsigned>(), S.ent_val2.as<unsigned>(), S.Minv.as<double>(),
                                             nfree, S.pcg_w.as<double>(), S.pcg_pap.as<double>(), S.pcg_part.as<double>(), S.pcg_sc.as<double>(), k & 1, pcu);
                    }
            }
        }
        // |r|^2 of the iterate the chunk ended on (the classic kernels publish it with every direction, one update late:
        // k_pcg_scalars brings sc[2], sc[3] up to date as well)
        if (pip) ppcg_launch_publish(st, S.pcg_part.as<double>(), nfree, S.pcg_sc.as<double>());
        else pcg_launch_publish(st, nfree, S.pcg_part.as<double>(), S.pcg_sc.as<double>(), pcu);
        t.itc += last_len;
        if (t.side_todo && (rc = start_inversion(t))) return rc;
    }
}

// One trial's reduced solve by PCG.  *solved stays false when the iteration did not converge: the dense solve takes over.
int BaCall::solve_pcg(const BaLm& lm, clk::time_point t2, int* ok2, bool* solved)
{
    int rc;
    int* bad = info_dev + INFO_MINV;
    CCM_HIP(c, hipMemsetAsync(bad, 0, 4, st));
    CCM_HIP(c, pcg_launch_minv(st, Hb, S.blk_row.as<int>(), S.blk_col.as<int>(), nb, nfree, S.Minv.as<double>(), bad));
    // Coarse level, pipelined: the inverse this trial uses was computed from the PREVIOUS trial's system on
    // the side stream while that trial's PCG ran (a preconditioner may be stale: lambda differs by the LM
    // factor, H by one relinearisation); this trial's system starts the next inversion.  Which inverse a
    // trial uses depends only on the trial number, never on timing, so all ranks do the same.
    PcgTrial t;
    if (PC.Aci && coarse_pending) {
        // No host round trip: the main stream waits for the inversion (normally over for milliseconds), copies the
        // inverse, and the verdict of the inversion is read together with the first scalars of this trial's PCG.
        CCM_HIP(c, hipStreamWaitEvent(st, S.ev_inv, 0));
        CCM_HIP(c, hipMemcpyAsync(PC.Aci, S.pcg_acw.p, (size_t)ncp * ncp * 8, hipMemcpyDeviceToDevice, st));
        CCM_HIP(c, hipMemcpyAsync(S.pinned + PIN_COARSE_INFO, info_dev + INFO_COARSE, 4, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipEventRecord(S.ev_copy, st));                   // the next inversion overwrites the work matrix: it waits for this copy
        coarse_pending = false; coarse_ready = true; t.coarse_unverified = true; copy_recorded = true;
    }
    const bool more_trials_planned = lm.it + 1 < lm.iterations || (lm.stage == 0 && opt->iterations2 > 0);
    t.side_todo = PC.Aci && more_trials_planned;
    t.max_it = 40 * 8 + (int)std::min<long long>(n, 4000);
    t.tol2 = pcg_tol * pcg_tol;
    volatile int& badh = pinned_int(PIN_PCG_BAD);                   // page-locked: a copy to the stack would stall the host until it is done
    badh = 0;
    CCM_HIP(c, hipMemcpyAsync(S.pinned + PIN_PCG_BAD, bad, 4, hipMemcpyDeviceToHost, st));
    if (pipelined) ppcg_launch_expand(st, Hb, S.ent_key2.as<unsigned>(), S.ent_val2.as<unsigned>(), 2 * nb, nfree, PB.Hf, PB.ecol);
    PcgStatus status;
    if ((rc = pcg_run(t, pipelined, &status))) return rc;
    if (status == PcgStatus::stale_coarse) { coarse_ready = false; if ((rc = pcg_run(t, pipelined, &status))) return rc; }
    if (status == PcgStatus::not_positive_definite && pipelined && !badh) {     // a breakdown of the recurrences is not a verdict on the matrix: ask the classic iteration
        res->pcg_fallbacks++;
        // TODO (deferred: changes numerical behaviour): "itc is not reset between the status-3 rerun and the classic fallback, so the
        // fallback starts with the iteration budget partly spent.  Reset itc, or keep a per-run counter, for the rerun and the fallback."
        if ((rc = pcg_run(t, false, &status))) return rc;
    }
    if (status == PcgStatus::not_positive_definite) { *ok2 = 0; *solved = true; }
    else if (status == PcgStatus::converged) *solved = true;
    if (t.side_todo && (rc = start_inversion(t))) return rc;
    res->pcg_iterations += t.itc;
    if (debug) {
        volatile double* sc = S.pinned + PIN_PCG_SC;
        fprintf(stderr, "[ccm] PCG trial: %d iterations, %.3f ms (host time of the side-stream enqueue %.3f), rel.res %.2e, |b| %.4e, lambda %.3e\n", t.itc, secs(t2, clk::now()) * 1e3, t.inv_host_ms, std::sqrt(sc[2] / std::max((double)sc[1], 1e-300)), std::sqrt((double)sc[1]), lm.lambda);
    }
    if (*solved && *ok2) CCM_HIP(c, hipMemcpyAsync(D.x, S.pcg_w.p, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    if (!*solved) res->pcg_fallbacks++;
    return CCM_OK;
}

// dense solve by the in-house block Gauss-Jordan (see dense_launch_solve for why not rocSOLVER)
// The dense solve's verdict ("not positive definite") of a small, single-rank problem is read together with the
// trial's chi2 instead of in a round trip of its own (a local BA is launch- and round-trip-bound: three host syncs
// per trial were a fifth of the call): the trial's update is applied as if the solve had succeeded and, if it had
// not, discarded exactly like a rejected step (the saved poses and points come back).
int BaCall::solve_dense(double lambda, int* ok2, bool* dense_info_pending)
{
    if (small_solve) {
        // a local BA's system: factored and solved by one workgroup in LDS, one launch (see k_dense_small_solve)
        if (dense_launch_small_solve(st, Hb, S.blk_row.as<int>(), S.blk_col.as<int>(), nb, (int)n, D.bs, D.x, info_dev + INFO_DENSE, lambda))
            return ccm_fail(c, CCM_E_DEVICE, "k_dense_small_solve: LDS request refused");
    } else {
        CCM_HIP(c, hipMemsetAsync(info_dev + INFO_DENSE, 0, 4, st));
        const size_t npd = (size_t)dense_pitch(n);
        CCM_RESERVE(c, S.Hs, (npd * npd + 48 * 48 + 8) * 8);
        double* Hs = S.Hs.as<double>();
        CCM_HIP(c, hipMemsetAsync(Hs, 0, npd * npd * 8, st));
        sp_launch_to_dense(st, Hb, S.blk_row.as<int>(), S.blk_col.as<int>(), nb, (long long)npd, Hs);   // row-major upper block triangle, pitch npd
        dense_launch_solve(st, Hs, (int)n, (int)npd, D.bs, D.x, info_dev + INFO_DENSE);
    }
    CCM_HIP(c, hipMemcpyAsync(S.pinned + PIN_DENSE_INFO, info_dev + INFO_DENSE, 4, hipMemcpyDeviceToHost, st));
    if (ranks == 1 && !fine_timers) *dense_info_pending = true;
    else { CCM_HIP(c, hipStreamSynchronize(st)); *ok2 = pinned_int(PIN_DENSE_INFO) == 0; }
    return CCM_OK;
}

// Every rank has solved the same reduced system.  Rank 0's increment -- and its verdict on positive
// definiteness -- is the one all ranks apply, so their poses stay bit-identical whatever a rank's solver
// did: the others contribute zeros to a sum all-reduce (x + 0 is exact).
int BaCall::share_increment(int* ok2)
{
    int rc;
    double* flag = scal + SCAL_X_OK;
    S.pinned[PIN_X_OK] = (rank == 0 && *ok2) ? 1.0 : 0.0;
    CCM_HIP(c, hipMemcpyAsync(flag, S.pinned + PIN_X_OK, 8, hipMemcpyHostToDevice, st));
    if (rank != 0 || !*ok2) CCM_HIP(c, hipMemsetAsync(D.x, 0, (size_t)n * 8, st));
    if ((rc = comm_allreduce_f64(c, D.x, (size_t)n, false))) return rc;
    if ((rc = comm_allreduce_f64(c, flag, 1, false))) return rc;
    CCM_HIP(c, hipMemcpyAsync(S.pinned + PIN_X_OK, flag, 8, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipStreamSynchronize(st));
    *ok2 = S.pinned[PIN_X_OK] != 0.0;
    return CCM_OK;
}

// one LM trial: Schur step, reduced solve, update, chi2 of the new state, accept or reject (sets lm.rho)
int BaCall::lm_trial(BaLm& lm)
{
    int rc;
    auto t1 = clk::now();
    RoctxRange trial_("ba:trial (schur + solve + update)");
    // (push: k_ba_update saves the state it is about to change; the fixed keyframes' poses were copied once, in lm_loop)
    int ok2 = 1;
    bool updated = false, looked_ahead = false;
    bool dense_info_pending = false;                       // see solve_dense
    auto t2 = t1;
    if (nfree > 0) {
        if ((rc = schur_step(lm))) return rc;
        tick(1);
        t2 = clk::now();
        if (!fine_timers) res->t_schur += secs(t1, t2);
        bool solved = false;
        if (use_pcg && (rc = solve_pcg(lm, t2, &ok2, &solved))) return rc;
        if (!solved && (rc = solve_dense(lm.lambda, &ok2, &dense_info_pending))) return rc;
    } else {
        // no free keyframe: only the landmark inverse is needed for the back-substitution
        sp_launch_dinv(st, D, lm.lambda);
        CCM_HIP(c, hipStreamSynchronize(st));
        tick(1);
        t2 = clk::now();
        if (!fine_timers) res->t_schur += secs(t1, t2);
    }
    if (hb_in_use) { CCM_HIP(c, hipEventSynchronize(S.ev_hb)); hb_in_use = false; }     // long over: the assembly is the side stream's first 0.2 ms
    if (ranks > 1 && nfree > 0 && (rc = share_increment(&ok2))) return rc;
    tick(2);
    auto t3 = clk::now();
    if (!fine_timers) res->t_solve += secs(t2, t3);
    res->trials++;
    double tempChi = DBL_MAX, scale = 0;
    if (ok2) {
        if (L > 0) { ProfScope ps(c, CCM_PROF_BA_BACKSUB); ba_launch_backsub(st, D, lm.lambda); }
        ba_launch_update(st, D, S.save_poses.as<double>(), S.save_points.as<double>());
        updated = true;
        looked_ahead = ranks == 1 && nfree > 0 && !env.no_ahead && lm.it + 1 < lm.iterations;
        if ((rc = eval_chi2(lm.huber, true, lm.lambda, &tempChi, &scale, true, looked_ahead))) return rc;     // synchronises the stream (or, looking ahead, waits for the chi2 alone)
        if (dense_info_pending && pinned_int(PIN_DENSE_INFO) != 0) { ok2 = 0; tempChi = DBL_MAX; scale = 0; }
    }
    scale += 1e-3;
    lm.rho = ok2 ? (lm.currentChi - tempChi) / scale : -1.0;
    // test switch: the first trial of iteration N is treated as rejected (the repeated-trial path -- pop, another lambda,
    // Hpl rebuilt -- on graphs whose trials are all accepted)
    if (lm.it == env.reject_at && lm.qmax == 0) lm.rho = -1.0;
    if (lm.rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow((2 * lm.rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        lm.lambda *= std::max(1. / 3., alpha);
        lm.ni = 2; lm.currentChi = tempChi;                             // discardTop
        lm.ahead_ready = looked_ahead;
    } else {
        lm.lambda *= lm.ni; lm.ni *= 2;
        if (updated) {                                                  // pop (a trial whose solve failed has not moved anything)
            CCM_HIP(c, hipMemcpyAsync(D.poses, S.save_poses.p, 7 * (size_t)P * 8, hipMemcpyDeviceToDevice, st));
            if (L) CCM_HIP(c, hipMemcpyAsync(D.points, S.save_points.p, 3 * (size_t)L * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    lm.qmax++;
    tick(3);
    if (!fine_timers) res->t_update += secs(t3, clk::now());
    return CCM_OK;
}

// the iterations of one stage (lm.stage, lm.iterations)
int BaCall::lm_stage(BaLm& lm)
{
    int rc;
    lm.lambda = 0; lm.ni = 2;
    int nBad = 0;
    if ((rc = sync_stop())) return rc;
    // computeActiveErrors + activeRobustChi2 at the top of an iteration (optimization_algorithm_levenberg.cpp:75-80) evaluate the state the
    // last ACCEPTED trial left, which that trial has just evaluated -- same kernels, same state, same sums: the value, the errors
    // and the pose matrices are carried over instead of computed again (one host round trip and three launches per iteration; a
    // local BA is bound by exactly those).  After a rejected last trial (state restored) and with several ranks (the stop flag
    // rides on this evaluation's all-reduce) the evaluation runs as before.
    bool chi_carried = false;
    double carried_chi = 0;
    lm.ahead_ready = false;
    for (lm.it = 0; lm.it < lm.iterations; lm.it++) {
        if (stop_requested()) { res->stopped = 1; break; }                    // !terminate(), sparse_optimizer.cpp:376
        auto t0 = clk::now();
        RoctxRange lin_("ba:linearize");
        lm.currentChi = 0;
        if (chi_carried && ranks == 1) lm.currentChi = carried_chi;
        else if ((rc = eval_chi2(lm.huber, false, 0, &lm.currentChi, nullptr))) return rc;
        chi_carried = false;
        const double iniChi = lm.currentChi;
        if (lm.first_eval) { res->chi2_initial = lm.currentChi; lm.first_eval = false; }
        // buildSystem.  From the second iteration on lambda is known here, and the landmarks' share of the first trial's Schur step
        // (Dinv, db, Z, ce) is computed by the same kernel
        const bool fused_schur = lm.it > 0 && nfree > 0 && lm.lambda > 0;
        // (and without Hpl, which only a repeated trial reads: see k_ba_lin_landmark MODE 2)
        const bool use_ahead = lm.ahead_ready;
        lm.ahead_ready = false;
        if (use_ahead) { std::swap(D.Hpp, Hpp_alt); std::swap(D.bp, bp_alt); }
        { ProfScope ps(c, CCM_PROF_BA_LINEARIZE); ba_launch_linearize(st, D, lm.huber, fused_schur ? lm.lambda : 0.0, env.keep_hpl, use_ahead); }
        lm.landmark_share_ready = fused_schur;
        lm.hpl_valid = !fused_schur || env.keep_hpl;
        if (lm.it == 0) { if ((rc = compute_lambda_init(lm))) return rc; nBad = 0; }
        tick(0);
        lin_.end();
        if (!fine_timers) res->t_linearize += secs(t0, clk::now());
        lm.rho = 0;
        lm.qmax = 0;
        do {
            if ((rc = lm_trial(lm))) return rc;
        } while (lm.rho < 0 && lm.qmax < 10 && !stop_requested());
        if (lm.rho > 0 && std::isfinite(lm.currentChi)) { chi_carried = true; carried_chi = lm.currentChi; }      // the last trial was accepted: currentChi is its chi2
        res->iterations_done++;
        res->chi2_final = lm.currentChi; res->lambda_final = lm.lambda;
        if (lm.qmax == 10 || lm.rho == 0) break;                                 // Terminate
        if ((iniChi - lm.currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;      // stop criterion :154-161
        if (nBad >= 3) break;
    }
    return CCM_OK;
}

// the two stages of a call: opt->iterations robust iterations, then opt->iterations2 plain ones without the outliers
int BaCall::lm_loop()
{
    int rc;
    if (split_up) CCM_HIP(c, hipStreamWaitEvent(st, S.ev_up, 0));          // observations, information values, points have arrived
    if (!S.ev_chi) CCM_HIP(c, hipEventCreateWithFlags(&S.ev_chi, hipEventDisableTiming));
    BaLm lm;
    lm.huber = opt->huber_delta > 0 ? opt->huber_delta : 0.0;
    CCM_HIP(c, hipMemcpyAsync(S.save_poses.p, D.poses, 7 * (size_t)P * 8, hipMemcpyDeviceToDevice, st));     // the fixed keyframes' entries of the saved state
    tick(-1);
    for (lm.stage = 0; lm.stage < 2 && !res->stopped; lm.stage++) {
        lm.iterations = lm.stage == 0 ? opt->iterations : opt->iterations2;
        if (lm.iterations <= 0) { if (lm.stage == 0) continue; else break; }
        if (lm.stage == 1) {
            // src/Optimizer.cpp:546-563: chi2 > th or non-positive depth -> level 1; every kernel dropped
            ba_launch_pose_rt(st, D);
            if (E > 0) { ba_launch_outliers(st, D, opt->outlier_chi2, S.flags.as<uint8_t>()); ba_launch_deactivate(st, D, S.flags.as<uint8_t>()); }
            lm.huber = 0.0;
        }
        if ((rc = lm_stage(lm))) return rc;
    }
    if (S.side) CCM_HIP(c, hipStreamSynchronize(S.side));
    return CCM_OK;
}

int BaCall::read_phase_timers()
{
    if (fine_timers && clock_phase.size() > 1) {
        CCM_HIP(c, hipStreamSynchronize(st));
        double* tp[4] = { &res->t_linearize, &res->t_schur, &res->t_solve, &res->t_update };
        for (size_t i = 1; i < clock_phase.size(); i++) {
            float ms = 0.f;
            if (clock_phase[i] >= 0 && hipEventElapsedTime(&ms, S.clock_ev[i - 1], S.clock_ev[i]) == hipSuccess) *tp[clock_phase[i]] += 1e-3 * (double)ms;
        }
    }
    lap("LM loop");
    return CCM_OK;
}

// ---- results: poses, points (gathered over the ranks), outlier flags in the caller's edge order
int BaCall::download()
{
    int rc;
    if (route) return publish();
    CCM_HIP(c, hipMemcpyAsync(pb->poses, D.poses, 7 * (size_t)P * 8, hipMemcpyDeviceToHost, st));
    if (ranks == 1) {
        // (a page-locked landing area + a threaded copy for pageable destinations was measured: 1.19 against 0.75 ms for config 5's 4.8 MB --
        //  the first touch of a freshly allocated destination costs the same either way, and the threads cost their creation)
        if (L) CCM_HIP(c, hipMemcpyAsync(pb->points, D.points, 3 * (size_t)L * 8, hipMemcpyDeviceToHost, st));
    } else {
        // every rank fills its landmark range of a zeroed full-size buffer; a sum all-reduce is the all-gather
        CCM_RESERVE(c, S.gather, std::max<size_t>(3 * (size_t)Lall * 8, 16));
        CCM_HIP(c, hipMemsetAsync(S.gather.p, 0, 3 * (size_t)Lall * 8, st));
        if (L) CCM_HIP(c, hipMemcpyAsync(S.gather.as<double>() + 3 * (size_t)l0, D.points, 3 * (size_t)L * 8, hipMemcpyDeviceToDevice, st));
        if ((rc = comm_allreduce_f64(c, S.gather.as<double>(), 3 * (size_t)Lall, false))) return rc;
        CCM_HIP(c, hipMemcpyAsync(pb->points, S.gather.p, 3 * (size_t)Lall * 8, hipMemcpyDeviceToHost, st));
    }
    if (outlier_out) {
        ba_launch_pose_rt(st, D);
        const bool straight = ranks == 1 && ix.direct;            // the caller's array is in the device's edge order
        std::vector<uint8_t> fl(straight ? 1 : std::max(E, 1));
        if (E > 0) {
            ba_launch_outliers(st, D, opt->outlier_chi2, S.flags.as<uint8_t>());
            CCM_HIP(c, hipMemcpyAsync(straight ? outlier_out : fl.data(), S.flags.p, E, hipMemcpyDeviceToHost, st));
        }
        CCM_HIP(c, hipStreamSynchronize(st));
        if (straight) {
            // (downloaded in place)
        } else if (ranks == 1) {
            for (int k = 0; k < E; k++) outlier_out[ix.perm[k]] = fl[k];
        } else {
            // flags of the other ranks' edges: exchange as doubles through the same collective
            std::vector<double> full(Eall, 0.0);
            for (int k = 0; k < E; k++) full[ix.edge_id(k)] = fl[k];
            CCM_RESERVE(c, S.gather, std::max<size_t>((size_t)Eall * 8, 16));
            CCM_HIP(c, hipMemcpyAsync(S.gather.p, full.data(), (size_t)Eall * 8, hipMemcpyHostToDevice, st));
            if ((rc = comm_allreduce_f64(c, S.gather.as<double>(), Eall, false))) return rc;
            CCM_HIP(c, hipMemcpyAsync(full.data(), S.gather.p, (size_t)Eall * 8, hipMemcpyDeviceToHost, st));
            CCM_HIP(c, hipStreamSynchronize(st));
            for (int e = 0; e < Eall; e++) outlier_out[e] = full[e] != 0.0;
        }
    }
    CCM_HIP(c, hipStreamSynchronize(st));
    CCM_HIP(c, hipGetLastError());
    lap("download results");
    return CCM_OK;
}

// The table route's download: the points narrowed into the table and the published poses into their handles (k_ba_publish_table),
// unless the stop flag ended the call before its first iteration (src/Optimizer.cpp:531-533 returns before writing anything); then
// one download of poses, outlier flags and the positions as the table holds them.
int BaCall::publish()
{
    int rc;
    Staging& G = *route->G;
    BaTableArgs& A = route->A;
    route->wrote = !(res->stopped && res->iterations_done == 0);
    A.poses = D.poses; A.points = D.points; A.scatter = route->wrote ? 1 : 0;
    ba_launch_publish_table(st, A);
    CCM_HIP(c, hipMemcpyAsync(G.dev<double>(route->o_pose_out), D.poses, 7 * (size_t)P * 8, hipMemcpyDeviceToDevice, st));
    if (outlier_out && E > 0) {
        ba_launch_pose_rt(st, D);
        ba_launch_outliers(st, D, opt->outlier_chi2, G.dev<uint8_t>(route->o_outl));
    }
    CCM_HIP(c, hipGetLastError());
    if ((rc = G.download(c, 0, route->res_end)) || (rc = G.wait(c))) return rc;
    std::memcpy(pb->poses, G.host<double>(route->o_pose_out), 7 * (size_t)P * 8);
    if (outlier_out) { const uint8_t* fl = G.host<uint8_t>(route->o_outl); for (int k = 0; k < E; k++) outlier_out[ix.edge_id(k)] = fl[k]; }
    G.get(route->pos_out, route->o_pos, 3 * (size_t)L * 4);
    lap("publish + download results");
    return CCM_OK;
}

// The stages of one call.  Every stage returns a CCM code (0 or negative) and nothing else: ccm_ba_solve cannot return a positive value.
int ba_solve_impl(ccm_ctx* c, ccm_ba_problem* pb, const ccm_ba_options* opt, ccm_ba_result* res, BaTableRoute* route)
{
    RoctxRange roctx_(route ? "ccm_ba_solve_table_frames" : "ccm_ba_solve");
    int rc;
    if ((rc = ba_begin(c, pb, opt, route != nullptr))) return rc;
    BaCall k(c, pb, opt, res, route);
    if ((rc = k.vertex_maps_and_shard())) return rc;
    if ((rc = k.index_on_device())) return rc;
    if ((rc = k.index_on_host())) return rc;
    if ((rc = k.upload_problem())) return rc;
    if ((rc = k.reserve_workspace())) return rc;
    if ((rc = k.build_block_structure())) return rc;
    if ((rc = k.select_solver())) return rc;
    k.capture_graphs();
    if ((rc = k.list_coarse_pairs())) return rc;
    if ((rc = k.lm_loop())) return rc;
    if ((rc = k.read_phase_timers())) return rc;
    return k.download();
}
}  // namespace

int ba_solve_table(ccm_ctx* c, ccm_ba_problem* pb, const ccm_ba_options* opt, ccm_ba_result* res, BaTableRoute* route)
{
    return ba_solve_impl(c, pb, opt, res, route);
}

extern "C" int ccm_ba_solve(ccm_ctx* c, ccm_ba_problem* pb, const ccm_ba_options* opt, ccm_ba_result* res)
{
    return ccm_guard(c, "ccm_ba_solve", [&] { return ba_solve_impl(c, pb, opt, res, nullptr); });
}
