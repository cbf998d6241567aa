// cslam_pnpsolver.cpp -- drop-in body of cslam::PnPsolver (src/PnPSolver.cpp): the constructor's loop (:57-100) fills the flat arrays
// of ccm_pnp_ransac_problem, the random draws of the sampling loop (:178-192) come from DUtils::Random::RandomInt as in the
// reference, and iterate / find forward to the C ABI.  The reference's header (include/cslam/PnPSolver.h) stays untouched, so the
// state the class has no member for -- the flat arrays, the draws and the ccm_pnp_solver handle -- lives in a side table keyed on the
// object; the destructor drops the entry.
//
// The RANSAC parameters are part of ccm_pnp_solver_create (every hypothesis is evaluated there), so the batch is created lazily at
// the first iterate / find after the last SetRansacParameters.  iterate's loop condition (:172) lets a call run past mRansacMaxIts,
// so the batch stores a reserve of hypotheses behind them: RESERVE_CALLS calls' worth of the first call's nIterations.  A call that
// would need more (a caller that keeps rejecting poses returned past mRansacMaxIts) gets CCM_E_STATE from the library and is
// answered with bNoMore = true: as far as this solver's stored hypotheses go, there are no more.  Unlike the reference,
// SetRansacParameters starts again from mnBestInliers = 0 (ccm_hot.h "PnPsolver").
//
// One PnPsolver object is a batch of one.  A caller that owns the candidate loop (ORB-SLAM's Tracking::Relocalization) gets the
// solvers of all candidates into one create through ccm_shim::pnp_candidates below (INTEGRATION.md "Relocalisation").
#include <cslam/PnPSolver.h>
#include <cslam/Frame.h>
#include <cslam/MapPoint.h>
#include <map>
#include <memory>
#include <mutex>
#include "ccm_shim.h"
#include "fuse_steps.h"

namespace ccm_shim {

static const int RESERVE_CALLS = 8;

struct PnpParams {
    double probability = 0.99; int min_inliers = 8, max_iterations = 300, min_set = 4; float epsilon = 0.4f, th2 = 5.991f;
};

// The constructor data of one solver (:57-100), appended to the flat arrays of a batch
struct PnpFlat {
    std::vector<int32_t> first{ 0 }, n1, kp_index;
    std::vector<int32_t> slot;           // with_slots: the point's slot in the map-point table beside every kp_index entry, -1 without one
    std::vector<float> K, P2D, P3Dw, sigma2;
    void add(const cslam::Frame& F, const std::vector<cslam::PnPsolver::mpptr>& vpMapPointMatches, bool with_slots = false)
    {
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            const cslam::PnPsolver::mpptr pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;                                   // :73-75
            const cv::KeyPoint& kp = F.mvKeysUn[i];
            P2D.push_back(kp.pt.x); P2D.push_back(kp.pt.y);
            sigma2.push_back(F.mvLevelSigma2[kp.octave]);
            const cv::Mat Pos = pMP->GetWorldPos();
            for (int k = 0; k < 3; k++) P3Dw.push_back(Pos.at<float>(k));
            kp_index.push_back((int32_t)i);
            if (with_slots) slot.push_back(map_slot_of(pMP));
        }
        first.push_back((int32_t)kp_index.size());
        n1.push_back((int32_t)vpMapPointMatches.size());
        K.push_back(F.fx); K.push_back(F.fy); K.push_back(F.cx); K.push_back(F.cy);        // :94-97
    }
    int solvers() const { return (int)n1.size(); }
    int size(int k) const { return first[k + 1] - first[k]; }
};

// Raw RandomInt results for rows hypotheses of every solver, in the reference's order of calls per solver (:183)
static std::vector<int32_t> draw(const PnpFlat& flat, int rows, int min_set)
{
    std::vector<int32_t> d((size_t)flat.solvers() * rows * min_set, 0);
    for (int k = 0; k < flat.solvers(); k++) {
        const int N = flat.size(k);
        if (N < min_set) continue;
        for (int h = 0; h < rows; h++)
            for (int i = 0; i < min_set; i++) d[((size_t)k * rows + h) * min_set + i] = DUtils::Random::RandomInt(0, N - 1 - i);
    }
    return d;
}

static ccm_pnp_solver* create(const PnpFlat& flat, const PnpParams& p, int reserve)
{
    const int max_its = p.max_iterations < 1 ? 1 : p.max_iterations;
    const std::vector<int32_t> draws = draw(flat, max_its + reserve, p.min_set);
    ccm_pnp_ransac_problem pb{};
    pb.n_solvers = flat.solvers(); pb.first = flat.first.data(); pb.n1 = flat.n1.data(); pb.K = flat.K.data();
    pb.P2D = flat.P2D.data(); pb.P3Dw = flat.P3Dw.data(); pb.sigma2 = flat.sigma2.data(); pb.kp_index = flat.kp_index.data();
    pb.probability = p.probability; pb.min_inliers = p.min_inliers; pb.max_iterations = max_its; pb.min_set = p.min_set;
    pb.epsilon = p.epsilon; pb.th2 = p.th2; pb.reserve = reserve; pb.draws = draws.data(); pb.flags = 0;
    ccm_pnp_solver* s = nullptr;
    if (ccm_pnp_solver_create(ctx(), &pb, &s)) throw estd::infrastructure_ex();
    return s;
}

// The same batch through ccm_pnp_solver_create_frames: the keypoints and octaves come from the frame's handle, the positions from the
// map-point table, and 8 bytes per correspondence go up in the place of 24.  flat was filled with_slots, so feature (kp_index) and slot
// of a correspondence were taken from the same point in the same pass.  nullptr = this route is not available (no handle of F in the
// cache, no table on this thread, a point without a slot, or match vectors that are not as long as the frame): the caller takes the
// array route, with draws of its own.
static ccm_pnp_solver* create_frames(const cslam::Frame& F, const PnpFlat& flat, const PnpParams& p, int reserve)
{
    if (flat.slot.size() != flat.kp_index.size()) return nullptr;
    for (int32_t s : flat.slot) if (s < 0) return nullptr;
    for (int32_t n : flat.n1) if (n != F.N) return nullptr;                          // iterate's vbInliers has the handle's N entries
    ccm_frame* cur = frame_handle(F);
    ccm_map_table* table = cur ? map_table_here() : nullptr;
    if (!cur || !table) return nullptr;
    const int max_its = p.max_iterations < 1 ? 1 : p.max_iterations;
    const std::vector<int32_t> draws = draw(flat, max_its + reserve, p.min_set);
    ccm_pnp_frames_problem fp{};
    fp.n_solvers = flat.solvers(); fp.first = flat.first.data(); fp.K = flat.K.data(); fp.feature = flat.kp_index.data(); fp.slot = flat.slot.data();
    fp.level_sigma2 = F.mvLevelSigma2.data(); fp.n_levels = (int32_t)F.mvLevelSigma2.size();
    fp.probability = p.probability; fp.min_inliers = p.min_inliers; fp.max_iterations = max_its; fp.min_set = p.min_set;
    fp.epsilon = p.epsilon; fp.th2 = p.th2; fp.reserve = reserve; fp.draws = draws.data(); fp.flags = 0;
    ccm_pnp_solver* s = nullptr;
    if (ccm_pnp_solver_create_frames(ctx(), cur, table, &fp, &s)) throw estd::infrastructure_ex();
    return s;
}

// PnPsolver::iterate of solver k of a batch, in the reference's types
static cv::Mat iterate(ccm_pnp_solver* s, int k, int n1, int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
{
    std::vector<uint8_t> inl(n1 > 0 ? n1 : 1, 0);
    int32_t found = 0, no_more = 0, n = 0;
    cv::Mat Tcw(4, 4, CV_32F);
    const int rc = ccm_pnp_solver_iterate(s, k, nIterations, &found, &no_more, inl.data(), &n, Tcw.ptr<float>());
    vbInliers.clear(); nInliers = 0;
    if (rc == CCM_E_STATE) { bNoMore = true; return cv::Mat(); }                  // beyond the reserve (see the head of this file)
    if (rc) throw estd::infrastructure_ex();
    bNoMore = no_more != 0;
    if (!found) return cv::Mat();
    vbInliers = std::vector<bool>(n1, false);
    for (int i = 0; i < n1; i++) vbInliers[i] = inl[i] != 0;
    nInliers = n;
    return Tcw;
}

// ---- all relocalisation candidates of one frame in one create.
// ORB-SLAM's Tracking::Relocalization builds one PnPsolver per candidate from SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i])
// and then calls iterate(5) on them in turn.  pnp_candidates takes the match vectors of all candidates (skip[i] != 0: discarded,
// no solver), flattens them with the constructor's rule, draws max_iterations + reserve minimal sets per solver and evaluates
// everything in one ccm_pnp_solver_create.  reserve: see ccm_hot.h; 5 * RESERVE_CALLS suits iterate(5).
class PnpBatch {
public:
    PnpBatch(ccm_pnp_solver* s, std::vector<int> slot, std::vector<int32_t> n1) : s_(s), slot_(std::move(slot)), n1_(std::move(n1)) {}
    ~PnpBatch() { ccm_pnp_solver_destroy(s_); }
    PnpBatch(const PnpBatch&) = delete; PnpBatch& operator=(const PnpBatch&) = delete;
    // iterate of candidate i (its index in the vector given to pnp_candidates); a skipped candidate reports bNoMore
    cv::Mat iterate(int i, int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        if (slot_[i] < 0) { bNoMore = true; vbInliers.clear(); nInliers = 0; return cv::Mat(); }
        return ccm_shim::iterate(s_, slot_[i], n1_[slot_[i]], nIterations, bNoMore, vbInliers, nInliers);
    }
private:
    ccm_pnp_solver* s_; std::vector<int> slot_; std::vector<int32_t> n1_;
};

std::unique_ptr<PnpBatch> pnp_candidates(const cslam::Frame& F, const std::vector<std::vector<cslam::PnPsolver::mpptr>>& vvpMapPointMatches,
                                         const std::vector<uint8_t>& skip, int reserve, double probability, int minInliers, int maxIterations,
                                         int minSet, float epsilon, float th2)
{
    PnpFlat flat;
    std::vector<int> slot(vvpMapPointMatches.size(), -1);
    for (size_t i = 0; i < vvpMapPointMatches.size(); i++) {
        if (!skip.empty() && skip[i]) continue;
        slot[i] = flat.solvers();
        flat.add(F, vvpMapPointMatches[i], /*with_slots=*/true);
    }
    PnpParams p;
    p.probability = probability; p.min_inliers = minInliers; p.max_iterations = maxIterations; p.min_set = minSet; p.epsilon = epsilon; p.th2 = th2;
    ccm_pnp_solver* s = create_frames(F, flat, p, reserve < 0 ? 0 : reserve);       // nullptr: no handle, or a point without a slot
    if (!s) s = create(flat, p, reserve < 0 ? 0 : reserve);
    return std::unique_ptr<PnpBatch>(new PnpBatch(s, slot, flat.n1));
}

// ---- the side table of the drop-in class
struct PnpSolverSide {
    PnpFlat flat;
    PnpParams params;
    ccm_pnp_solver* solver = nullptr;
    ~PnpSolverSide() { ccm_pnp_solver_destroy(solver); }
};
static std::mutex g_pnp_mutex;
static std::map<const void*, PnpSolverSide>& pnp_table()
{
    static std::map<const void*, PnpSolverSide> t;
    return t;
}
static PnpSolverSide& pnp_side_of(const void* self, bool fresh = false)
{
    std::lock_guard<std::mutex> lock(g_pnp_mutex);
    if (fresh) pnp_table().erase(self);
    return pnp_table()[self];
}
void pnp_solver_release(const void* self)
{
    std::lock_guard<std::mutex> lock(g_pnp_mutex);
    pnp_table().erase(self);
}

}  // namespace ccm_shim

namespace cslam {

PnPsolver::PnPsolver(const Frame &F, const vector<mpptr> &vpMapPointMatches):
    pws(0), us(0), alphas(0), pcs(0), maximum_number_of_correspondences(0), number_of_correspondences(0), mnInliersi(0),
    mnIterations(0), mnBestInliers(0), N(0)
{
    ccm_shim::PnpSolverSide& S = ccm_shim::pnp_side_of(this, /*fresh=*/true);
    mvpMapPointMatches = vpMapPointMatches;
    S.flat.add(F, vpMapPointMatches);
    fu = F.fx; fv = F.fy; uc = F.cx; vc = F.cy;
    SetRansacParameters();                                                    // :99
}

PnPsolver::~PnPsolver()
{
    ccm_shim::pnp_solver_release(this);
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2)
{
    ccm_shim::PnpSolverSide& S = ccm_shim::pnp_side_of(this);
    ccm_pnp_solver_destroy(S.solver);                                         // the next iterate evaluates the batch anew
    S.solver = nullptr;
    S.params.probability = probability; S.params.min_inliers = minInliers; S.params.max_iterations = maxIterations;
    S.params.min_set = minSet; S.params.epsilon = epsilon; S.params.th2 = th2;
    N = S.flat.size(0);
    int32_t mi = 0, its = 1; float eps = epsilon;
    ccm_pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mi, &its, &eps);       // :119-142
    mRansacProb = probability; mRansacMinInliers = mi; mRansacMaxIts = its; mRansacEpsilon = eps; mRansacMinSet = minSet;
    mnIterations = 0; mnBestInliers = 0;
}

cv::Mat PnPsolver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    ccm_shim::PnpSolverSide& S = ccm_shim::pnp_side_of(this);
    if (!S.solver) S.solver = ccm_shim::create(S.flat, S.params, ccm_shim::RESERVE_CALLS * (nIterations > 5 ? nIterations : 5));
    const cv::Mat Tcw = ccm_shim::iterate(S.solver, 0, S.flat.n1[0], nIterations, bNoMore, vbInliers, nInliers);
    int32_t its = 0, best = 0;
    ccm_pnp_solver_state(S.solver, 0, &its, &best, nullptr, nullptr, nullptr);
    mnIterations = its; mnBestInliers = best;
    return Tcw;
}

cv::Mat PnPsolver::find(vector<bool> &vbInliers, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);                // :149-153
}

}  // namespace cslam
