// cslam_sim3solver.cpp -- drop-in body of cslam::Sim3Solver (src/Sim3Solver.cpp): the constructor's map-side loop (:5-92) fills the
// flat arrays of ccm_sim3_ransac_problem, the random draws of the sampling loop (:146-161) come from DUtils::Random::RandomInt as in
// the reference, and iterate / find / GetEstimated* forward to the C ABI.  The reference's header (include/cslam/Sim3Solver.h) stays
// untouched, so the state the class has no member for -- the flat arrays and the ccm_sim3_solver handle -- lives in a side table
// keyed on the object.  The header declares no destructor (LoopFinder and MapMatcher never delete their solvers either); an entry
// is reused when a new solver is constructed at the address of an old one, and ccm_shim::sim3_solver_release(this) drops it for a
// caller that does delete.
//
// The RANSAC parameters are part of ccm_sim3_solver_create (every hypothesis is evaluated there, in one launch), so the batch is
// created lazily at the first iterate / find after the last SetRansacParameters.  One Sim3Solver object is a batch of one; a caller
// that owns the candidate loop (src/LoopFinder.cpp:251-282) gets all candidates into one launch by filling one
// ccm_sim3_ransac_problem itself.  ccm_shim::search_by_bow_candidates below is the step in front of that batch: the
// SearchByBoW(mpCurrentKF, pKF, ...) calls of the same loop (src/LoopFinder.cpp:265, src/MapMatcher.cpp:271) as one
// ccm_search_by_bow_frames call over all candidates; ccm_shim::search_by_sim3_on_table and search_by_projection_on_table are the two
// matchers behind the solver (SearchBySim3 for all candidates in one call, SearchByProjection(pKF, Scw, ...)) on keyframe handles and
// the map-point table, sim3_solvers_on_table the solver batch with its constructor's loop on the device, and
// compute_sim3_candidates_on_table SearchBySim3 and OptimizeSim3 of one pass in one call.  They take the calling thread's handle on the table (map_table_here: on LoopFinder's and MapMatcher's threads a
// view of the rows the tracking thread's table holds), as Fuse on the table does; without one they decline and the caller's ORBmatcher
// call takes the array route.
#include <cslam/Sim3Solver.h>
#include <cslam/KeyFrame.h>
#include <cslam/MapPoint.h>
#include <cslam/ORBmatcher.h>
#include <cmath>
#include <map>
#include <mutex>
#include "ccm_shim.h"
#include "fuse_steps.h"

namespace ccm_shim {

struct Sim3SolverSide {
    std::vector<float> X1, X2, max_err1, max_err2;
    std::vector<int32_t> indices1;
    float K1[4], K2[4];
    int32_t n1 = 0, fix_scale = 0, best_inliers = 0;
    double probability = 0.99; int min_inliers = 6, max_iterations = 300;
    ccm_sim3_solver* solver = nullptr;
    bool have_estimate = false; float R[9], t[3], s = 1.0f;       // the running best carried over a SetRansacParameters
    ~Sim3SolverSide() { ccm_sim3_solver_destroy(solver); }
};

static std::mutex g_side_mutex;
static std::map<const void*, Sim3SolverSide>& side_table()
{
    static std::map<const void*, Sim3SolverSide> t;
    return t;
}
static Sim3SolverSide& side_of(const void* self, bool fresh = false)
{
    std::lock_guard<std::mutex> lock(g_side_mutex);
    if (fresh) side_table().erase(self);
    return side_table()[self];
}
void sim3_solver_release(const void* self)
{
    std::lock_guard<std::mutex> lock(g_side_mutex);
    side_table().erase(self);
}

// the solver of the current parameters, created on first use (one upload, one launch, one download)
static ccm_sim3_solver* ensure(Sim3SolverSide& S)
{
    if (S.solver) return S.solver;
    const int N = (int)S.indices1.size();
    const int32_t first[2] = { 0, N };
    std::vector<int32_t> draws((size_t)S.max_iterations * 3, 0);
    if (N >= 3)
        for (int h = 0; h < S.max_iterations; h++)
            for (int i = 0; i < 3; i++) draws[3 * h + i] = DUtils::Random::RandomInt(0, N - 1 - i);       // :151
    ccm_sim3_ransac_problem pb{};
    pb.n_solvers = 1; pb.first = first; pb.n1 = &S.n1; pb.fix_scale = &S.fix_scale; pb.K1 = S.K1; pb.K2 = S.K2;
    pb.X1 = S.X1.data(); pb.X2 = S.X2.data(); pb.max_err1 = S.max_err1.data(); pb.max_err2 = S.max_err2.data(); pb.indices1 = S.indices1.data();
    pb.probability = S.probability; pb.min_inliers = S.min_inliers; pb.max_iterations = S.max_iterations;
    pb.draws = draws.data(); pb.best_inliers = &S.best_inliers;
    if (ccm_sim3_solver_create(ctx(), &pb, &S.solver)) throw estd::infrastructure_ex();
    return S.solver;
}

// A keyframe as a handle in the calling thread's context, with the node directory of its mFeatVec; nullptr on failure.
static ccm_frame* candidate_handle(const cslam::Sim3Solver::kfptr& pKF)
{
    const int n = (int)pKF->mvKeysUn.size();
    std::vector<float> kx(n), ky(n), angle(n); std::vector<int32_t> oct(n);
    for (int i = 0; i < n; i++) { kx[i] = pKF->mvKeysUn[i].pt.x; ky[i] = pKF->mvKeysUn[i].pt.y; oct[i] = pKF->mvKeysUn[i].octave; angle[i] = pKF->mvKeysUn[i].angle; }
    const cv::Mat desc = pKF->mDescriptors.isContinuous() ? pKF->mDescriptors : pKF->mDescriptors.clone();
    const ccm_frame_grid g{n, kx.data(), ky.data(), oct.data(), desc.data, (float)pKF->mnMinX, (float)pKF->mnMinY, pKF->mfGridElementWidthInv,
                           pKF->mfGridElementHeightInv, pKF->mnGridCols, pKF->mnGridRows};
    const std::vector<int32_t> node = nodes_of(pKF->mFeatVec, n);
    ccm_frame* f = nullptr;
    if (ccm_frame_create(ctx(), &g, angle.data(), &f) || ccm_frame_set_bow(f, node.data())) { ccm_frame_destroy(f); return nullptr; }
    return f;
}

// The first loop of LoopFinder::ComputeSim3 (src/LoopFinder.cpp:251-282) and of MapMatcher (src/MapMatcher.cpp:258-290) in one call:
// matcher.SearchByBoW(pKF1, candidates[i], vvpMatches12[i]) for every candidate (ORBmatcher(0.75, true) there), returning nmatches per
// candidate.  The caller keeps its own tests around it (isBad candidates are passed with skip[i] != 0 and get 0 matches) and builds
// the Sim3Solver batch from the result.  The handles are made for this call in the calling thread's context and recycled through its
// pool; a caller that meets the same keyframes again may keep them instead.
std::vector<int> search_by_bow_candidates(const cslam::Sim3Solver::kfptr& pKF1, const std::vector<cslam::Sim3Solver::kfptr>& candidates,
                                          const std::vector<uint8_t>& skip, float nnratio, bool check_ori,
                                          std::vector<std::vector<cslam::Sim3Solver::mpptr>>& vvpMatches12)
{
    typedef cslam::Sim3Solver::mpptr mpptr;
    const int K = (int)candidates.size();
    std::vector<int> result(K, 0);
    const std::vector<mpptr> mps1 = pKF1->GetMapPointMatches();
    const int n1 = (int)mps1.size();
    vvpMatches12.assign(K, std::vector<mpptr>(n1));
    std::vector<int> live;                                                     // candidates that take part
    for (int i = 0; i < K; i++) if (skip.empty() || !skip[i]) live.push_back(i);
    if (live.empty()) return result;
    struct Handles {
        std::vector<ccm_frame*> v;
        ~Handles() { for (ccm_frame* f : v) ccm_frame_destroy(f); }
    } H;
    H.v.push_back(candidate_handle(pKF1));
    std::vector<std::vector<mpptr>> mps2(live.size());
    std::vector<int32_t> first2(live.size() + 1, 0);
    std::vector<uint8_t> valid1(std::max(n1, 1), 0), valid2;
    for (int i = 0; i < n1; i++) valid1[i] = mps1[i] && !mps1[i]->isBad();
    for (size_t j = 0; j < live.size(); j++) {
        H.v.push_back(candidate_handle(candidates[live[j]]));
        mps2[j] = candidates[live[j]]->GetMapPointMatches();
        for (const mpptr& p : mps2[j]) valid2.push_back(p && !p->isBad());
        first2[j + 1] = (int32_t)valid2.size();
    }
    for (ccm_frame* f : H.v) if (!f) throw estd::infrastructure_ex();
    if (valid2.empty()) valid2.push_back(0);
    const ccm_bow_options o{nnratio, check_ori ? 1 : 0, 50, /*strict_th=*/1};  // TH_LOW; :629 compares with <
    std::vector<int32_t> m12(live.size() * (size_t)std::max(n1, 1), -1), nm(live.size(), 0);
    if (ccm_search_by_bow_frames(ctx(), H.v[0], (int)live.size(), H.v.data() + 1, &o, valid1.data(), first2.data(), valid2.data(), m12.data(), nm.data()))
        throw estd::infrastructure_ex();
    for (size_t j = 0; j < live.size(); j++) {
        result[live[j]] = nm[j];
        for (int i = 0; i < n1; i++) {
            const int32_t m = m12[j * (size_t)n1 + i];
            if (m >= 0) vvpMatches12[live[j]][i] = mps2[j][m];
        }
    }
    return result;
}

static void rows_of(const cv::Mat& R, const cv::Mat& t, float out[12])
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) out[4 * r + c] = R.at<float>(r, c);
        out[4 * r + 3] = t.at<float>(r);
    }
}

// Link 3 of ComputeSim3 (src/LoopFinder.cpp:300-330, src/MapMatcher.cpp:307-337): matcher.SearchBySim3(pKF1, candidates[i],
// vvpMatches12[i], s12[i], R12[i], t12[i], th) for every candidate the caller hands over, in ONE ccm_search_by_sim3_table_frames.  The
// keyframes travel as handles whose map-point ids are table slots (handle_of), the points are read from the table; only the entry
// marks go up, 8 bytes a feature of pKF1.  The intrinsics are pKF1's for both directions, as in the reference (:1127-1130).
bool search_by_sim3_on_table(const ORBmatcher::kfptr& pKF1, const std::vector<ORBmatcher::kfptr>& candidates,
                             std::vector<std::vector<ORBmatcher::mpptr>>& vvpMatches12, const std::vector<float>& s12, const std::vector<cv::Mat>& R12,
                             const std::vector<cv::Mat>& t12, float th, KeyframeHandleOf handle_of, std::vector<int>& found)
{
    typedef ORBmatcher::mpptr mpptr;
    const int K = (int)candidates.size();
    if (vvpMatches12.size() != candidates.size() || s12.size() != candidates.size() || R12.size() != candidates.size() || t12.size() != candidates.size())
        return false;
    ccm_map_table* table = map_table_here();
    if (!table) return false;
    ccm_frame* h1 = handle_of(pKF1);
    if (!h1) return false;
    const int n1 = (int)pKF1->GetMapPointMatches().size();
    std::vector<ccm_sim3_search_pair> pairs(K);
    std::vector<std::vector<int32_t>> m12(K), mi2(K);
    std::vector<std::vector<mpptr>> mps2(K);
    const cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
    for (int k = 0; k < K; k++) {
        const ORBmatcher::kfptr& pKF2 = candidates[k];
        ccm_sim3_search_pair& P = pairs[k];
        P.kf1 = h1;
        if (!(P.kf2 = handle_of(pKF2)) || (int)vvpMatches12[k].size() != n1) return false;
        mps2[k] = pKF2->GetMapPointMatches();
        const cv::Mat sR12 = s12[k] * R12[k], sR21 = (1.0 / s12[k]) * R12[k].t(), t21 = -sR21 * t12[k];    // :1141-1143
        rows_of(R1w, t1w, P.T1w); rows_of(pKF2->GetRotation(), pKF2->GetTranslation(), P.T2w);
        rows_of(sR21, t21, P.S21); rows_of(sR12, t12[k], P.S12);
        P.fx = pKF1->fx; P.fy = pKF1->fy; P.cx = pKF1->cx; P.cy = pKF1->cy;
        P.bounds1[0] = pKF1->mnMinX; P.bounds1[1] = pKF1->mnMaxX; P.bounds1[2] = pKF1->mnMinY; P.bounds1[3] = pKF1->mnMaxY;
        P.bounds2[0] = pKF2->mnMinX; P.bounds2[1] = pKF2->mnMaxX; P.bounds2[2] = pKF2->mnMinY; P.bounds2[3] = pKF2->mnMaxY;
        m12[k].assign(std::max(n1, 1), -1); mi2[k].assign(std::max(n1, 1), -1);
        for (int i = 0; i < n1; i++) {                                         // :1154-1164
            const mpptr& pMP = vvpMatches12[k][i];
            if (!pMP) continue;
            const int s = map_slot_of(pMP);
            m12[k][i] = s >= 0 ? s : 0;                                        // only "there is a point" is read
            mi2[k][i] = pMP->GetIndexInKeyFrame(pKF2);
        }
        P.matched12 = m12[k].data(); P.matched_idx2 = mi2[k].data();
    }
    std::vector<int32_t> match12((size_t)K * std::max(n1, 1), -1), n_found(std::max(K, 1), 0);
    if (K > 0) {
        const ORBmatcher::kfptr& pKF2 = candidates[0];                         // one client's keyframes share the extractor's scale tables
        const ccm_sim3_search_problem p{K, pairs.data(), th, pKF1->mfLogScaleFactor, (int32_t)pKF1->mvScaleFactors.size(), pKF1->mvScaleFactors.data(),
                                        pKF2->mfLogScaleFactor, (int32_t)pKF2->mvScaleFactors.size(), pKF2->mvScaleFactors.data()};
        ccm_sim3_search_result r{};
        r.match12 = match12.data(); r.n_found = n_found.data();
        if (ccm_search_by_sim3_table_frames(ctx(), table, &p, &r) < 0) return false;
    }
    found.assign(K, 0);
    for (int k = 0; k < K; k++) {
        found[k] = n_found[k];
        for (int i = 0; i < n1; i++) {                                         // :1337-1342
            const int32_t i2 = match12[(size_t)k * n1 + i];
            if (i2 >= 0) vvpMatches12[k][i] = mps2[k][i2];
        }
    }
    return true;
}

// Link 5 (src/LoopFinder.cpp:372, src/MapMatcher.cpp:380): matcher.SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints,
// mvpCurrentMatchedPoints, 10) in ONE ccm_search_by_projection_table_frames.  Nothing is projected on the host; the loop points travel
// as slots and vpMatched as one slot per feature.  The remap of an accepted point the keyframe already observes (:414-435) is made
// here from best_idx and observed, in list order as the reference does.
bool search_by_projection_on_table(const ORBmatcher::kfptr& pKF, const cv::Mat& Scw, const std::vector<ORBmatcher::mpptr>& vpPoints,
                                   std::vector<ORBmatcher::mpptr>& vpMatched, int th, KeyframeHandleOf handle_of, int& nmatches)
{
    typedef ORBmatcher::mpptr mpptr;
    ccm_map_table* table = map_table_here();
    ccm_frame* h = table ? handle_of(pKF) : nullptr;
    if (!table || !h) return false;
    const int n = (int)vpPoints.size(), N = (int)vpMatched.size();
    std::vector<int32_t> slot(std::max(n, 1), -1), ms(std::max(N, 1), -1);
    std::map<int, int> seen;
    for (int i = 0; i < n; i++) {
        const int s = vpPoints[i] ? map_slot_of(vpPoints[i]) : -1;
        if (s < 0 || !seen.emplace(s, i).second) return false;                 // a point without a slot, or listed twice: the array route
        slot[i] = s;
    }
    for (int i = 0; i < N; i++)
        if (vpMatched[i]) { const int s = map_slot_of(vpMatched[i]); if (s < 0) return false; ms[i] = s; }
    ccm_loop_view V{};
    V.view.kf = h;
    cv::Mat sRcw = Scw.rowRange(0, 3).colRange(0, 3);                           // :317-321
    const float scw = sqrt(sRcw.row(0).dot(sRcw.row(0)));
    cv::Mat Rcw = sRcw / scw, tcw = Scw.rowRange(0, 3).col(3) / scw, Ow = -Rcw.t() * tcw;
    rows_of(Rcw, tcw, V.view.Tcw);
    for (int r = 0; r < 3; r++) V.view.Ow[r] = Ow.at<float>(r);
    V.view.fx = pKF->fx; V.view.fy = pKF->fy; V.view.cx = pKF->cx; V.view.cy = pKF->cy;
    V.view.min_x = pKF->mnMinX; V.view.max_x = pKF->mnMaxX; V.view.min_y = pKF->mnMinY; V.view.max_y = pKF->mnMaxY;
    V.matched_slot = ms.data();
    const ccm_loop_projection_problem p{1, &V, n, slot.data(), pKF->mfLogScaleFactor, (int32_t)pKF->mvScaleFactors.size(), pKF->mvScaleFactors.data(), (float)th};
    std::vector<int32_t> best(std::max(n, 1), -1), ms_out(std::max(N, 1), -1);
    std::vector<uint8_t> observed(std::max(n, 1), 0);
    int32_t nm = 0;
    ccm_loop_projection_result r{};
    r.best_idx = best.data(); r.observed = observed.data(); r.matched_slot = ms_out.data(); r.n_matches = &nm;
    if (ccm_search_by_projection_table_frames(ctx(), table, &p, &r) < 0) return false;
    for (int i = 0; i < n; i++) {
        if (best[i] < 0) continue;
        const mpptr& pMP = vpPoints[i];
        if (!observed[i]) { vpMatched[best[i]] = pMP; continue; }               // :439
        const int existing_idx = pMP->GetIndexInKeyFrame(pKF);                  // :415-434
        if (existing_idx == -1) continue;
        // :420-429 recomputes DescriptorDistance(dMP, row bestIdx), which is bestDist itself, and asks whether it is smaller than
        // bestDist: bDoNotReplace stays false
        pKF->RemapMapPointMatch(pMP, existing_idx, best[i]);
    }
    nmatches = nm;
    return true;
}

// mvnMaxError per level as the constructor leaves it (:67-68 into a std::vector<size_t>), and the two poses of a pair
static std::vector<float> max_err_levels(const ORBmatcher::kfptr& pKF)
{
    std::vector<float> out(pKF->mvLevelSigma2.size());
    for (size_t l = 0; l < out.size(); l++) out[l] = (float)(size_t)(9.210 * pKF->mvLevelSigma2[l]);
    return out;
}
static void intrinsics_of(const ORBmatcher::kfptr& pKF, float K[4]) { K[0] = pKF->fx; K[1] = pKF->fy; K[2] = pKF->cx; K[3] = pKF->cy; }

// Link 2 on handles.  The filter "set and not bad" (:32-59) stays here: the caller sizes its draws by N.  A correspondence is (i1,
// GetIndexInKeyFrame(pKF2)): the kernel reads the two points at those features of the handles, which are pMP1 and pMP2 as long as
// mObservations and mvpMapPoints agree.
bool sim3_solvers_on_table(const ORBmatcher::kfptr& pKF1, const std::vector<ORBmatcher::kfptr>& candidates,
                           const std::vector<std::vector<ORBmatcher::mpptr>>& vvpMatches12, bool fix_scale, double probability, int min_inliers,
                           int max_iterations, const std::vector<int32_t>& draws, KeyframeHandleOf handle_of, std::vector<int>& n, ccm_sim3_solver** out)
{
    typedef ORBmatcher::mpptr mpptr;
    const int K = (int)candidates.size();
    if (vvpMatches12.size() != candidates.size() || !out) return false;
    ccm_map_table* table = map_table_here();
    ccm_frame* h1 = table ? handle_of(pKF1) : nullptr;
    if (!table || !h1 || K == 0) return false;
    const std::vector<mpptr> mps1 = pKF1->GetMapPointMatches();
    std::vector<ccm_sim3_frames_pair> pairs(K);
    std::vector<int32_t> first(K + 1, 0), fix(K, fix_scale ? 1 : 0), f1, f2;
    const cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
    for (int k = 0; k < K; k++) {
        const ORBmatcher::kfptr& pKF2 = candidates[k];
        ccm_sim3_frames_pair& P = pairs[k];
        P.kf1 = h1;
        if (!(P.kf2 = handle_of(pKF2)) || vvpMatches12[k].size() != mps1.size()) return false;
        rows_of(R1w, t1w, P.T1w); rows_of(pKF2->GetRotation(), pKF2->GetTranslation(), P.T2w);
        intrinsics_of(pKF1, P.K1); intrinsics_of(pKF2, P.K2);
        for (size_t i1 = 0; i1 < mps1.size(); i1++) {                          // :30-59
            const mpptr& pMP1 = mps1[i1]; const mpptr& pMP2 = vvpMatches12[k][i1];
            if (!pMP2 || !pMP1 || pMP1->isBad() || pMP2->isBad()) continue;
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (pMP1->GetIndexInKeyFrame(pKF1) < 0 || i2 < 0) continue;
            if (map_slot_of(pMP1) < 0 || map_slot_of(pMP2) < 0) return false;  // a point without a slot: the array route
            f1.push_back((int32_t)i1); f2.push_back(i2);
        }
        first[k + 1] = (int32_t)f1.size();
    }
    if ((int)draws.size() < K * max_iterations * 3) return false;
    const std::vector<float> e1 = max_err_levels(pKF1), e2 = max_err_levels(candidates[0]);
    ccm_sim3_solver_frames_problem p{};
    p.n_solvers = K; p.pairs = pairs.data(); p.first = first.data(); p.fix_scale = fix.data(); p.feature1 = f1.data(); p.feature2 = f2.data();
    p.n_levels1 = (int32_t)e1.size(); p.max_err_level1 = e1.data(); p.n_levels2 = (int32_t)e2.size(); p.max_err_level2 = e2.data();
    p.probability = probability; p.min_inliers = min_inliers; p.max_iterations = max_iterations; p.draws = draws.data();
    ccm_sim3_solver* s = nullptr;
    if (ccm_sim3_solver_create_frames(ctx(), table, &p, &s)) return false;
    n.assign(K, 0);
    for (int k = 0; k < K; k++) n[k] = first[k + 1] - first[k];
    *out = s;
    return true;
}

// Links 3 and 4 in one call.  Nothing of a map point is projected or uploaded here; the entry marks go up as for
// search_by_sim3_on_table, and vpMatches1[i] = NULL comes back as `pruned`.
bool compute_sim3_candidates_on_table(const ORBmatcher::kfptr& pKF1, const std::vector<ORBmatcher::kfptr>& candidates,
                                      std::vector<std::vector<ORBmatcher::mpptr>>& vvpMatches12, const std::vector<float>& s12,
                                      const std::vector<cv::Mat>& R12, const std::vector<cv::Mat>& t12, float th, float th2, bool fix_scale,
                                      KeyframeHandleOf handle_of, std::vector<double>& sim3, std::vector<int>& n_inliers)
{
    typedef ORBmatcher::mpptr mpptr;
    const int K = (int)candidates.size();
    if (vvpMatches12.size() != candidates.size() || s12.size() != candidates.size() || R12.size() != candidates.size() || t12.size() != candidates.size() ||
        sim3.size() != 8 * candidates.size() || K == 0)
        return false;
    ccm_map_table* table = map_table_here();
    ccm_frame* h1 = table ? handle_of(pKF1) : nullptr;
    if (!table || !h1) return false;
    const int n1 = (int)pKF1->GetMapPointMatches().size();
    std::vector<ccm_compute_sim3_pair> pairs(K);
    std::vector<std::vector<int32_t>> m12(K), mi2(K);
    std::vector<std::vector<mpptr>> mps2(K);
    const cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
    for (int k = 0; k < K; k++) {
        const ORBmatcher::kfptr& pKF2 = candidates[k];
        ccm_compute_sim3_pair& C = pairs[k];
        ccm_sim3_search_pair& P = C.search;
        P.kf1 = h1;
        if (!(P.kf2 = handle_of(pKF2)) || (int)vvpMatches12[k].size() != n1) return false;
        mps2[k] = pKF2->GetMapPointMatches();
        const cv::Mat sR12 = s12[k] * R12[k], sR21 = (1.0 / s12[k]) * R12[k].t(), t21 = -sR21 * t12[k];    // src/ORBmatcher.cpp:1141-1143
        rows_of(R1w, t1w, P.T1w); rows_of(pKF2->GetRotation(), pKF2->GetTranslation(), P.T2w);
        rows_of(sR21, t21, P.S21); rows_of(sR12, t12[k], P.S12);
        P.fx = pKF1->fx; P.fy = pKF1->fy; P.cx = pKF1->cx; P.cy = pKF1->cy;
        P.bounds1[0] = pKF1->mnMinX; P.bounds1[1] = pKF1->mnMaxX; P.bounds1[2] = pKF1->mnMinY; P.bounds1[3] = pKF1->mnMaxY;
        P.bounds2[0] = pKF2->mnMinX; P.bounds2[1] = pKF2->mnMaxX; P.bounds2[2] = pKF2->mnMinY; P.bounds2[3] = pKF2->mnMaxY;
        m12[k].assign(std::max(n1, 1), -1); mi2[k].assign(std::max(n1, 1), -1);
        for (int i = 0; i < n1; i++) {
            const mpptr& pMP = vvpMatches12[k][i];
            if (!pMP) continue;
            const int s = map_slot_of(pMP);
            if (s < 0) return false;                                           // a point without a slot: the array route
            m12[k][i] = s;
            mi2[k][i] = pMP->GetIndexInKeyFrame(pKF2);
        }
        P.matched12 = m12[k].data(); P.matched_idx2 = mi2[k].data();
        intrinsics_of(pKF2, C.K2);
        for (int i = 0; i < 8; i++) C.sim3[i] = sim3[8 * (size_t)k + i];
        C.fix_scale = fix_scale ? 1 : 0; C.th2 = th2;
    }
    const ORBmatcher::kfptr& pKF2 = candidates[0];                             // one client's keyframes share the extractor's scale tables
    ccm_compute_sim3_problem p{};
    p.n_pairs = K; p.pairs = pairs.data(); p.th = th;
    p.log_scale_factor1 = pKF1->mfLogScaleFactor; p.n_levels1 = (int32_t)pKF1->mvScaleFactors.size(); p.scale_factors1 = pKF1->mvScaleFactors.data();
    p.inv_level_sigma2_1 = pKF1->mvInvLevelSigma2.data();
    p.log_scale_factor2 = pKF2->mfLogScaleFactor; p.n_levels2 = (int32_t)pKF2->mvScaleFactors.size(); p.scale_factors2 = pKF2->mvScaleFactors.data();
    p.inv_level_sigma2_2 = pKF2->mvInvLevelSigma2.data();
    std::vector<int32_t> match12((size_t)K * std::max(n1, 1), -1), n_found(K, 0), n_corr(K, 0), n_in(K, 0);
    std::vector<uint8_t> pruned((size_t)K * std::max(n1, 1), 0);
    std::vector<double> s3(8 * (size_t)K, 0.0);
    ccm_compute_sim3_result r{};
    r.search.match12 = match12.data(); r.search.n_found = n_found.data();
    r.pruned = pruned.data(); r.n_correspondences = n_corr.data(); r.n_inliers = n_in.data(); r.sim3 = s3.data();
    if (ccm_compute_sim3_table_frames(ctx(), table, &p, &r) < 0) return false;
    n_inliers.assign(K, 0);
    for (int k = 0; k < K; k++) {
        n_inliers[k] = n_in[k];
        for (int i = 0; i < n1; i++) {
            const int32_t i2 = match12[(size_t)k * n1 + i];
            if (i2 >= 0) vvpMatches12[k][i] = mps2[k][i2];                     // src/ORBmatcher.cpp:1337-1342
            if (pruned[(size_t)k * n1 + i]) vvpMatches12[k][i] = static_cast<mpptr>(NULL);       // src/Optimizer.cpp:1017, :1051
        }
    }
    sim3 = s3;
    return true;
}

}  // namespace ccm_shim

namespace cslam {

Sim3Solver::Sim3Solver(kfptr pKF1, kfptr pKF2, const vector<mpptr> &vpMatched12, const bool bFixScale):
    mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale)
{
    ccm_shim::Sim3SolverSide& S = ccm_shim::side_of(this, true);
    mpKF1 = pKF1;
    mpKF2 = pKF2;
    const vector<mpptr> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = vpMatched12.size();
    mvpMatches12 = vpMatched12;
    const cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
    size_t idx = 0;
    for (int i1 = 0; i1 < mN1; i1++) {                                        // :30-83
        if (!vpMatched12[i1]) continue;
        mpptr pMP1 = vpKeyFrameMP1[i1];
        mpptr pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
        const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        const cv::KeyPoint &kp1 = pKF1->mvKeysUn[indexKF1];
        const cv::KeyPoint &kp2 = pKF2->mvKeysUn[indexKF2];
        const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
        const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
        // mvnMaxError1/2 are std::vector<size_t> in the header (include/cslam/Sim3Solver.h:74-75): the push_back of :67-68 drops the
        // fraction, and CheckInliers compares the float error with that integer.  The same value goes to the library as a float.
        mvnMaxError1.push_back(9.210 * sigmaSquare1);
        mvnMaxError2.push_back(9.210 * sigmaSquare2);
        S.max_err1.push_back((float)mvnMaxError1.back());
        S.max_err2.push_back((float)mvnMaxError2.back());
        mvpMapPoints1.push_back(pMP1);
        mvpMapPoints2.push_back(pMP2);
        mvnIndices1.push_back(i1);
        S.indices1.push_back(i1);
        const cv::Mat X1c = Rcw1 * pMP1->GetWorldPos() + tcw1, X2c = Rcw2 * pMP2->GetWorldPos() + tcw2;       // :74-78
        mvX3Dc1.push_back(X1c);
        mvX3Dc2.push_back(X2c);
        for (int k = 0; k < 3; k++) { S.X1.push_back(X1c.at<float>(k)); S.X2.push_back(X2c.at<float>(k)); }
        mvAllIndices.push_back(idx);
        idx++;
    }
    mK1 = pKF1->mK;
    mK2 = pKF2->mK;
    S.K1[0] = mK1.at<float>(0, 0); S.K1[1] = mK1.at<float>(1, 1); S.K1[2] = mK1.at<float>(0, 2); S.K1[3] = mK1.at<float>(1, 2);
    S.K2[0] = mK2.at<float>(0, 0); S.K2[1] = mK2.at<float>(1, 1); S.K2[2] = mK2.at<float>(0, 2); S.K2[3] = mK2.at<float>(1, 2);
    S.n1 = mN1; S.fix_scale = bFixScale ? 1 : 0;
    SetRansacParameters();                                                    // :91; mvP1im1 / mvP2im2 (:88-89) are formed by the library
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{
    ccm_shim::Sim3SolverSide& S = ccm_shim::side_of(this);
    if (S.solver) {                                                           // mnBestInliers and the best estimate survive (:94-118)
        int32_t best = 0;
        ccm_sim3_solver_state(S.solver, 0, nullptr, &best, nullptr, nullptr);
        S.best_inliers = best;
        if (ccm_sim3_solver_estimate(S.solver, 0, S.R, S.t, &S.s) == CCM_OK) S.have_estimate = true;
        ccm_sim3_solver_destroy(S.solver);
        S.solver = nullptr;
    }
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    N = mvpMapPoints1.size();
    mRansacMaxIts = ccm_sim3_ransac_iterations(N, probability, minInliers, maxIterations);     // :104-115
    mnIterations = 0;
    S.probability = probability; S.min_inliers = minInliers; S.max_iterations = maxIterations < 1 ? 1 : maxIterations;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    ccm_shim::Sim3SolverSide& S = ccm_shim::side_of(this);
    ccm_sim3_solver* solver = ccm_shim::ensure(S);
    std::vector<uint8_t> inl(mN1 > 0 ? mN1 : 1, 0);
    int32_t found = 0, no_more = 0, n = 0;
    cv::Mat T12(4, 4, CV_32F);
    if (ccm_sim3_solver_iterate(solver, 0, nIterations, &found, &no_more, inl.data(), &n, T12.ptr<float>())) throw estd::infrastructure_ex();
    int32_t its = 0, best = 0;
    ccm_sim3_solver_state(solver, 0, &its, &best, nullptr, nullptr);
    mnIterations = its; mnBestInliers = best;
    bNoMore = no_more != 0;
    vbInliers = vector<bool>(mN1, false);
    for (int i = 0; i < mN1; i++) vbInliers[i] = inl[i] != 0;
    nInliers = n;
    return found ? T12 : cv::Mat();
}

cv::Mat Sim3Solver::find(vector<bool> &vbInliers12, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);              // :193-197
}

cv::Mat Sim3Solver::GetEstimatedRotation()
{
    ccm_shim::Sim3SolverSide& S = ccm_shim::side_of(this);
    cv::Mat R(3, 3, CV_32F);
    if (S.solver && ccm_sim3_solver_estimate(S.solver, 0, R.ptr<float>(), nullptr, nullptr) == CCM_OK) return R;
    if (!S.have_estimate) return cv::Mat();                                   // mBestRotation before any hypothesis
    for (int k = 0; k < 9; k++) R.ptr<float>()[k] = S.R[k];
    return R;
}

cv::Mat Sim3Solver::GetEstimatedTranslation()
{
    ccm_shim::Sim3SolverSide& S = ccm_shim::side_of(this);
    cv::Mat t(3, 1, CV_32F);
    if (S.solver && ccm_sim3_solver_estimate(S.solver, 0, nullptr, t.ptr<float>(), nullptr) == CCM_OK) return t;
    if (!S.have_estimate) return cv::Mat();
    for (int k = 0; k < 3; k++) t.ptr<float>()[k] = S.t[k];
    return t;
}

float Sim3Solver::GetEstimatedScale()
{
    ccm_shim::Sim3SolverSide& S = ccm_shim::side_of(this);
    float s = S.s;
    if (S.solver) ccm_sim3_solver_estimate(S.solver, 0, nullptr, nullptr, &s);
    return s;
}

}  // namespace cslam
