/* ccm_hot.h -- C ABI of the MI355X hot path for CCM-SLAM
 * (ORB extraction, Hamming matching, reprojection bundle adjustment).
 *
 * This is the drop-in boundary: plain pointers and sizes,
 * caller-allocated HOST buffers unless a name says `_dev`, int return 0 = OK or a
 * negative CCM_E_* code, nothing throws.  One ccm_ctx per calling thread: it
 * owns a HIP stream, device workspaces and (optionally) an RCCL communicator,
 * so concurrent callers never share device state.
 *
 * All file:line citations are relative to the reference tree
 * (taiyaki-go/motioncheck_ccm_slam).  INTEGRATION.md shows the C++ shim a
 * maintainer adds on the reference side to forward the original classes here.
 */
#ifndef CCM_HOT_H
#define CCM_HOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an existing struct, enum count or prototype changes (3: ccm_ba_result.pcg_pipelined; round 2 had already changed
 * ccm_essential_graph, CCM_PROF_COUNT and removed ccm_comm_init_shm under version 1).  New entry points and new types are additions
 * and do not bump it (the frame handles, ccm_frame_*, came under version 3).  A caller compiled against another version
 * must not call further: ccm_abi_version() returns the library's value, compare it with this macro (the Python mirror and
 * shim/ccm_shim.h do). */
#define CCM_ABI_VERSION 3

enum {
    CCM_OK = 0,
    CCM_E_ARG = -1,       /* bad argument (null pointer, size <= 0, unsupported parameter) */
    CCM_E_DEVICE = -2,    /* HIP runtime error; ccm_last_error() has the text */
    CCM_E_NOMEM = -3,     /* host or device allocation failed */
    CCM_E_CAPACITY = -4,  /* caller buffer too small (max_per_image, topk ...) */
    CCM_E_NUMERIC = -5,   /* reduced system not positive definite in every LM trial */
    CCM_E_COMM = -6,      /* RCCL error */
    CCM_E_STATE = -7      /* call order violated (e.g. debug fetch before extract) */
};

typedef struct ccm_ctx ccm_ctx;

/* ------------------------------------------------------------------ context */
int ccm_abi_version(void);
/* device = HIP device ordinal.  flags: reserved, pass 0. */
ccm_ctx* ccm_create(int device, int flags);
void ccm_destroy(ccm_ctx*);
const char* ccm_last_error(const ccm_ctx*);
/* Blocks until everything queued on the context's stream has finished. */
int ccm_sync(ccm_ctx*);
/* The hipStream_t the context launches on (for callers that time with HIP events). */
void* ccm_stream(ccm_ctx*);

/* Per-kernel timing with HIP events on the context's stream (bench.py's roofline figures).
 * While enabled, every launch group is bracketed by two events.  ccm_profile_read synchronises,
 * returns for each label the summed milliseconds and the number of launches since the last read,
 * and resets the sums.  Labels: see CCM_PROF_*. */
enum { CCM_PROF_RESIZE = 0, CCM_PROF_FAST_SCORE, CCM_PROF_CELL_NMS, CCM_PROF_OCTREE, CCM_PROF_ORIENT_DESC,
       CCM_PROF_HAMMING_BF,
       /* bundle adjustment: linearisation (k_ba_lin_landmark + k_ba_lin_pose), landmark inverse and Y = Hpl Dinv
        * (k_sp_dinv + k_sp_edge_y), the Schur block GEMM (k_sp_schur_blocks), bschur, back-substitution */
       CCM_PROF_BA_LINEARIZE, CCM_PROF_BA_DINV_Y, CCM_PROF_BA_SCHUR_BLOCKS, CCM_PROF_BA_BSCHUR, CCM_PROF_BA_BACKSUB,
       CCM_PROF_COUNT };
/* Page-lock a host buffer the caller keeps (a frame pool, the cv::Mat a camera driver fills): uploads from it and downloads
 * into it then go by DMA at the full PCIe rate instead of through the runtime's staging of pageable memory.  Thin wrappers over
 * hipHostRegister / hipHostUnregister; optional -- every entry point accepts pageable pointers. */
int ccm_host_register(ccm_ctx*, void* ptr, size_t bytes);
int ccm_host_unregister(ccm_ctx*, void* ptr);

int ccm_profile_enable(ccm_ctx*, int on);
int ccm_profile_read(ccm_ctx*, float ms[CCM_PROF_COUNT], int32_t launches[CCM_PROF_COUNT]);

/* ---------------------------------------------------------------- extractor
 * Replaces ORBextractor::ORBextractor (cslam/src/ORBextractor.cpp:579-639) and
 * ORBextractor::operator() (:1216-1278) with its callees ComputePyramid
 * (:1280-1304), ComputeKeyPointsOctTree (:933-1024), DistributeOctTree
 * (:707-931), IC_Angle (:68-95), GaussianBlur 7x7 sigma 2 (:1259) and
 * computeOrbDescriptor (:100-316).                                           */
typedef struct {
    int   nfeatures;     /* ORBextractor.nFeatures   (cslam/conf/config.yaml:38-51) */
    float scale_factor;  /* ORBextractor.scaleFactor */
    int   nlevels;       /* ORBextractor.nLevels, 1..CCM_MAX_LEVELS */
    int   ini_th_fast;   /* ORBextractor.iniThFAST */
    int   min_th_fast;   /* ORBextractor.minThFAST */
} ccm_orb_params;

#define CCM_MAX_LEVELS 16

/* Layout-identical to cv::KeyPoint (pt.x, pt.y, size, angle, response, octave,
 * class_id): a std::vector<cv::KeyPoint>'s storage can be passed directly. */
typedef struct {
    float x, y;
    float size;
    float angle;     /* degrees [0,360) */
    float response;  /* FAST score */
    int32_t octave;
    int32_t class_id; /* always -1 */
} ccm_keypoint;

/* Constructor tables (getters GetScaleFactors / GetInverseScaleFactors /
 * GetScaleSigmaSquares / GetInverseScaleSigmaSquares, include/cslam/ORBextractor.h:120-150).
 * Each output may be NULL; arrays hold nlevels entries (umax: 16). Host only, no GPU. */
int ccm_orb_tables(const ccm_orb_params*, float* scale, float* inv_scale, float* sigma2,
                   float* inv_sigma2, int32_t* features_per_level, int32_t* umax);
/* Pyramid level sizes for a w x h input (ORBextractor.cpp:1284-1285). Host only. */
int ccm_orb_level_sizes(const ccm_orb_params*, int w, int h, int32_t* level_w, int32_t* level_h);

/* Batched operator(): n_images 8-bit images of w x h (row stride `stride` bytes,
 * image i starts at img + i*image_stride) -> per image up to max_per_image
 * keypoints and 32-byte descriptors, rows in the reference's order (level-major,
 * then DistributeOctTree list order).  kps: [n_images][max_per_image],
 * desc: [n_images][max_per_image][32], counts: [n_images].
 * Rows past counts[i] are zero.
 * n_images == 0 or w*h == 0 -> CCM_OK with nothing written (the reference
 * returns silently on an empty image, ORBextractor.cpp:1219-1220).
 * Returns CCM_E_CAPACITY if an image yields more than max_per_image keypoints
 * (never happens with max_per_image >= nfeatures). */
int ccm_orb_extract(ccm_ctx*, const ccm_orb_params*, const uint8_t* img, int w, int h, int stride,
                    size_t image_stride, int n_images, ccm_keypoint* kps, uint8_t* desc,
                    int32_t* counts, int max_per_image);

/* Device-resident variant: img_dev is a device pointer; results stay on the
 * device (fetch with ccm_orb_fetch) so that ccm_hamming_match_dev can consume
 * the descriptors without a PCIe round trip.  The call is asynchronous and
 * ordered on the context's stream: it starts after everything queued there
 * before it, and whatever is queued there after it sees the whole batch.
 * Inside the call a large batch is extracted in chunks of frames that alternate
 * between the context's stream and one auxiliary stream of the context (forked
 * from and joined back to the context's stream before the call returns, also
 * when it fails), so that one chunk's quadtree kernel runs beside the other
 * chunk's FAST or descriptor kernel.  Small batches, a single frame among them,
 * and every call while ccm_profile_enable is on run as one chunk on the
 * context's stream.  An image with more than max_per_image keypoints is
 * reported by the next ccm_orb_fetch, which returns CCM_E_CAPACITY and copies
 * nothing; counts_dev (ccm_orb_result_dev) then holds the counts clamped to
 * max_per_image.  */
int ccm_orb_extract_dev(ccm_ctx*, const ccm_orb_params*, const uint8_t* img_dev, int w, int h,
                        int stride, size_t image_stride, int n_images, int max_per_image);
/* Copy the last ccm_orb_extract_dev results to host (any pointer may be NULL). */
int ccm_orb_fetch(ccm_ctx*, ccm_keypoint* kps, uint8_t* desc, int32_t* counts);
/* Device pointers of the last extract: desc_dev [n_images][max_per_image][32],
 * counts_dev [n_images] (int32).  Valid until the next extract on this ctx. */
int ccm_orb_result_dev(ccm_ctx*, const uint8_t** desc_dev, const int32_t** counts_dev,
                       int* max_per_image);

/* Test/debug taps of the last extract (host copies; synchronise internally):
 * pyramid level pixels (mvImagePyramid, include/cslam/ORBextractor.h:152) ... */
int ccm_orb_debug_level(ccm_ctx*, int image, int level, uint8_t* out, int out_stride);
/* ... and the per-level FAST candidates before DistributeOctTree, in the order
 * vToDistributeKeys is filled (ORBextractor.cpp:957-998): xy[2*i], xy[2*i+1]
 * relative to minBorderX/Y as there, score[i].  Returns the count (>= 0) or an error. */
int ccm_orb_debug_candidates(ccm_ctx*, int image, int level, int32_t* xy, int32_t* score, int max);
/* The chunks ccm_orb_extract_dev splits a batch of n_images frames into (host only, no GPU): chunk i is frames
 * [frame0[i], frame0[i] + nrun[i]) on lane[i] (0 = the context's stream, 1 = the auxiliary stream).  out_per_frame is the
 * geometry's number of keypoint slots per frame, lane_frames the configured frames per chunk (CCM_ORB_LANE_FRAMES; 0 = one
 * chunk).  Writes at most max entries (any array may be NULL) and returns the number of chunks, or an error. */
int ccm_orb_debug_lane_plan(int n_images, int out_per_frame, int lane_frames, int32_t* frame0, int32_t* nrun, int32_t* lane, int max);
/* The FAST-9/16 score as the fused kernel computes it, on the CPU (host only, no GPU).  vr: n rows of 17 bytes, the centre
 * pixel and its 16 ring pixels in ring order.  full[i] = the score by its definition (both polarities); split[i] = what the
 * kernel stores at thresholds min(iniThFAST, minThFAST) = t_lo -- one polarity per pass, chosen by the four compass pixels --
 * which is full[i] where full[i] >= t_lo and full[i] > 0, else -1 (nothing stored). */
int ccm_debug_fast_score(const uint8_t* vr /* n x 17: v, ring */, int n, int t_lo, int32_t* full, int32_t* split);
/* The items of the fused kernel's rejection test -- one dword (four pixels) of a band's LDS tile each -- in the order its waves
 * take them, produced on the CPU by the code the kernel runs (host only, no GPU).  The band: LDS pitch in bytes (a multiple of 4,
 * 16..256), bh rows (0..65), detection dwords dw_lo..dw_hi of a row (1 <= dw_lo, dw_hi <= pitch / 4 - 2; dw_hi < dw_lo = none).
 * Writes at most max rows of six int32 -- run, wave, lane, row, dword, pos0 (tile offset of the item's first pixel) -- run by
 * run, and returns the number of items (>= 0, it may exceed max) or an error. */
int ccm_debug_fc_items(int pitch, int bh, int dw_lo, int dw_hi, int32_t* out /* max x 6 */, int max);
/* Test tap of the descriptor kernel's orientation and steering: for each of n moment pairs (m01, m10) of IC_Angle, one wave runs the
 * device functions the kernel runs and writes the angle in degrees (cv::fastAtan2), (a, b) = (cos, sin) of it as the kernel steers
 * with them, and the rounded offsets (dx, dy) of the pattern's 512 sample points in pattern order (ORBextractor.cpp:104-110).
 * Synchronises internally. */
int ccm_debug_od_steer(ccm_ctx*, const int32_t* m01, const int32_t* m10, int n,
                       float* angle_deg, float* ab /* n x 2 */, int8_t* offs /* n x 512 x 2 */);

/* ------------------------------------------------------------------ matcher
 * ORBmatcher::DescriptorDistance (cslam/src/ORBmatcher.cpp:1653-1669): host helper. */
int ccm_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Brute-force best / second-best Hamming search, n_pairs independent problems
 * (the inner loop of SearchByBoW, ORBmatcher.cpp:224-245, over one vocabulary
 * node holding every feature).  q: [n_pairs][nq][32], t: [n_pairs][nt][32].
 * Optional per-pair live counts nq_n/nt_n (NULL = all nq/nt rows live).
 * Outputs per query: best_idx (lowest index wins ties, -1 if nt == 0),
 * best_dist and second_dist (256 when absent), exactly the running
 * (bestDist1,bestIdx,bestDist2) of the reference with strict `<`. */
int ccm_hamming_match(ccm_ctx*, const uint8_t* q, int nq, const uint8_t* t, int nt, int n_pairs,
                      const int32_t* nq_n, const int32_t* nt_n,
                      int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
/* Test tap of the matcher's FP4 matrix-core tile: a and b are 32 descriptors (32 x 32 bytes) each, out[32 * i + j] =
 * row_c[i] - 4096 * (number of bits a[i] and b[j] have in common), computed by the expansion to e2m1 operands and the
 * block-scaled matrix instructions the brute-force kernel uses.  Synchronises internally. */
int ccm_debug_fp4_tile(ccm_ctx*, const uint8_t* a, const uint8_t* b, const float* row_c, float* out);
/* Same on device pointers (descriptor strides in rows), asynchronous.  q_dev and t_dev must be 16-byte aligned and
 * nt <= 65535 (CCM_E_ARG otherwise). */
int ccm_hamming_match_dev(ccm_ctx*, const uint8_t* q_dev, int nq, size_t q_pair_stride,
                          const uint8_t* t_dev, int nt, size_t t_pair_stride, int n_pairs,
                          const int32_t* nq_n_dev, const int32_t* nt_n_dev,
                          int32_t* best_idx_dev, int32_t* best_dist_dev, int32_t* second_dist_dev);

/* Acceptance test applied by the callers (ORBmatcher.cpp:247-249): host helper.
 * strict = 0 -> best <= th (Frame variant), 1 -> best < th (KF-KF variant, :641). */
int ccm_ratio_test(int best_dist, int second_dist, float nnratio, int th, int strict);

/* ORBmatcher::SearchByBoW, both overloads (ORBmatcher.cpp:178-306, 565-698), for one pair.
 * Side 1 = the keyframe whose features drive the outer loop, side 2 = the
 * frame/keyframe searched.  node1/node2: vocabulary node id of every feature
 * (the FeatureVector, as one id per feature; features with the same id are
 * visited in ascending feature index, as DBoW2 fills them).  valid1: feature
 * has a good MapPoint (pMP && !isBad).  valid2: NULL for the Frame overload
 * (every frame feature is a candidate), else the KF-KF validity mask.
 * angle1/angle2: keypoint angles (degrees) for the rotation histogram.
 * Output match12[n1]: index into side 2 or -1 -- the KF-KF overload's
 * vpMatches12; for the Frame overload the reference fills
 * vpMapPointMatches[idx2] = MP(idx1), the shim inverts it.  Returns the number
 * of matches (>= 0) or an error. */
typedef struct {
    float nnratio;        /* mfNNratio */
    int   check_ori;      /* mbCheckOrientation */
    int   th;             /* TH_LOW = 50 */
    int   strict_th;      /* 0: best <= th (Frame overload), 1: best < th (KF-KF) */
} ccm_bow_options;
int ccm_match_bow(ccm_ctx*, const ccm_bow_options*,
                  const uint8_t* desc1, const int32_t* node1, const uint8_t* valid1,
                  const float* angle1, int n1,
                  const uint8_t* desc2, const int32_t* node2, const uint8_t* valid2,
                  const float* angle2, int n2, int32_t* match12);

/* Windowed matchers.  A frame's undistorted keypoints with its 75x48 feature grid
 * (Frame::AssignFeaturesToGrid, src/Frame.cpp:103-118; FRAME_GRID_COLS/ROWS include/cslam/Frame.h:51-52). */
typedef struct {
    int n;                         /* Frame::N */
    const float* kp_x; const float* kp_y; const int32_t* kp_octave;   /* mvKeysUn */
    const uint8_t* desc;           /* mDescriptors [n][32] */
    float min_x, min_y;            /* mnMinX, mnMinY */
    float inv_w, inv_h;            /* mfGridElementWidthInv, mfGridElementHeightInv */
    int grid_cols, grid_rows;      /* 75, 48 */
} ccm_frame_grid;
/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cpp:200-253) for nq queries at once, with the
 * Hamming distance of each returned feature to the query's descriptor.  Per query up to `cap` entries, in
 * the order the reference returns them; cand_n[q] is the true count (CCM_E_CAPACITY if any exceeds cap).
 * r < 0 skips a query. */
int ccm_window_candidates(ccm_ctx*, const ccm_frame_grid*, int nq, const float* qx, const float* qy, const float* qr,
                          const int32_t* min_level, const int32_t* max_level, const uint8_t* qdesc, int cap,
                          int32_t* cand_idx, int32_t* cand_dist, int32_t* cand_n);
/* ORBmatcher::SearchByProjection(Frame&, const vector<mpptr>&, th) (cslam/src/ORBmatcher.cpp:71-148), the matcher
 * of TrackLocalMap.  Per map point: in_view = mbTrackInView && !isBad, level = mnTrackScaleLevel, view_cos =
 * mTrackViewCos, proj = mTrackProjX/Y, its descriptor, has_obs = Observations() > 0.  occupied[i] (in/out): feature i
 * already holds a map point with observations.  match[i] = index of the map point newly assigned to feature i or
 * -1.  Returns nmatches. */
int ccm_search_by_projection(ccm_ctx*, const ccm_frame_grid*, const float* scale_factors, int n_mp, const uint8_t* in_view,
                             const int32_t* level, const float* view_cos, const float* proj_x, const float* proj_y,
                             const uint8_t* mp_desc, const uint8_t* mp_has_obs, uint8_t* occupied, float th, float nnratio,
                             int32_t* match);

/* ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th) (ORBmatcher.cpp:1350-1476), the matcher of
 * TrackWithMotionModel.  Per last-frame feature: valid = has a map point, not an outlier, and its projection (u,v)
 * into the current frame (computed by the caller in float as :1382-1393) has positive depth and lies inside the
 * frame bounds; last_octave, last_angle = LastFrame.mvKeys[i].octave / mvKeysUn[i].angle.  match[i2] = last-frame
 * feature whose map point is assigned to current feature i2, or -1.  Returns nmatches.  orb_dist = TH_HIGH (100) here.
 * The relocalisation overload SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1478-1605) is the same
 * loop over the keyframe's map points: valid = not bad, not in sAlreadyFound and projected inside the frame and the
 * distance range (:1502-1531), last_octave = nPredictedLevel, last_angle = pKF->mvKeysUn[i].angle, mp_has_obs all 1
 * (any assigned feature is skipped, :1547), occupied = mvpMapPoints[i2] != null, orb_dist = ORBdist. */
int ccm_search_by_projection_frame(ccm_ctx*, const ccm_frame_grid* current, const float* cur_angle, const float* scale_factors,
                                   int n_last, const uint8_t* valid, const float* u, const float* v, const int32_t* last_octave,
                                   const float* last_angle, const uint8_t* mp_desc, const uint8_t* mp_has_obs, uint8_t* occupied,
                                   float th, int check_ori, int orb_dist, int32_t* match);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cpp:448-563).
 * prev_matched_xy [n1][2] is vbPrevMatched (updated for matched features as :556-558); matches12[i1] = index into
 * F2 or -1.  Returns nmatches. */
int ccm_search_for_initialization(ccm_ctx*, int n1, const int32_t* oct1, const uint8_t* desc1, const float* angle1,
                                  const ccm_frame_grid* f2, const float* angle2, float* prev_matched_xy, int window,
                                  float nnratio, int check_ori, int32_t* matches12);

/* Selection loop of ORBmatcher::Fuse, both overloads (ORBmatcher.cpp:914-955 with the chi2 gate, :1072-1100 without):
 * per map point that passed the caller's geometric checks (valid, projection u,v, predicted level) the most similar
 * keyframe feature in the window th * scaleFactor[level] at level-1..level.  best_idx[m] = feature or -1 (bestDist
 * > accept_th = TH_LOW); the caller applies Replace / AddObservation in map-point order as :958-990 / :1103-1118. */
int ccm_fuse_select(ccm_ctx*, const ccm_frame_grid* kf, const float* scale_factors, const float* inv_level_sigma2, int n_mp,
                    const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* mp_desc, float th,
                    int chi2_check, int accept_th, int32_t* best_idx, int32_t* best_dist);

/* ccm_fuse_select for n_kf keyframes in ONE launch -- the server's fuse loops call Fuse once per keyframe (src/Mapping.cpp:515-546:
 * the current keyframe's map points into every neighbour; src/MapMerger.cpp:576-586: the loop map points into every corrected
 * keyframe).  Map points projected into keyframe k are rows mp_first[k] .. mp_first[k+1]-1 (mp_first[0] = 0) of valid / u / v /
 * level / mp_desc / best_idx / best_dist; best_idx is an index into keyframe k's own features.  Returns what n_kf sequential
 * ccm_fuse_select calls return: the selection reads projections, descriptors and features only; a point that an earlier
 * keyframe's Replace has made bad is skipped by the caller when it applies the results in keyframe order (ORBmatcher.cpp:884-886). */
int ccm_fuse_select_batch(ccm_ctx*, int n_kf, const ccm_frame_grid* kfs, const float* scale_factors, const float* inv_level_sigma2,
                          const int32_t* mp_first, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                          const uint8_t* mp_desc, float th, int chi2_check, int accept_th, int32_t* best_idx, int32_t* best_dist);

/* ORBmatcher::SearchBySim3 (ORBmatcher.cpp:1124-1348).  The caller projects every map point of KF1 into KF2 with the
 * Sim3 (valid1/u1/v1/level1 per feature of KF1, :1170-1208; mp_desc1 = GetDescriptor()) and vice versa; both
 * directions select the most similar feature (<= TH_HIGH) and match12[i1] = i2 where they agree (:1330-1345), else -1.
 * Returns nFound. */
int ccm_search_by_sim3(ccm_ctx*, const ccm_frame_grid* kf1, const float* scale_factors1, const ccm_frame_grid* kf2, const float* scale_factors2,
                       const uint8_t* valid1, const float* u1, const float* v1, const int32_t* level1, const uint8_t* mp_desc1,
                       const uint8_t* valid2, const float* u2, const float* v2, const int32_t* level2, const uint8_t* mp_desc2,
                       float th, int32_t* match12);

/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cpp:308-446), loop closing.  valid/u/v/
 * level = the caller's projection checks (:333-377); matched[idx] (in/out) = vpMatched[idx] != null; observed[m] = the
 * point already is an observation of pKF (GetIndexInKeyFrame != -1, :414: the caller re-maps it, vpMatched is not
 * touched).  best_idx[m] = chosen feature or -1.  Returns nmatches. */
int ccm_search_by_projection_sim3(ccm_ctx*, const ccm_frame_grid* kf, const float* scale_factors, int n_mp, const uint8_t* valid,
                                  const float* u, const float* v, const int32_t* level, const uint8_t* mp_desc, const uint8_t* observed,
                                  uint8_t* matched, float th, int32_t* best_idx);
/* ccm_search_by_projection_sim3 for n_kf keyframes in ONE launch per kernel -- the loop closer projects the loop's map points into
 * every keyframe connected to the current one (src/LoopFinder.cpp, src/MapMatcher.cpp: one SearchByProjection(pKF, Scw, vpPoints,
 * vpMatched, th) per keyframe).  Keyframe k's map points are rows mp_first[k] .. mp_first[k+1]-1 (mp_first[0] = 0) of valid / u / v /
 * level / mp_desc / observed / best_idx; its vpMatched flags are bytes F_k .. F_k + kfs[k].n - 1 of `matched` with F_k = kfs[0].n + ...
 * + kfs[k-1].n (in/out); best_idx is an index into keyframe k's own features; n_matches[k] = what the single call returns for
 * keyframe k.  Returns the sum, i.e. exactly what n_kf sequential calls return and write. */
int ccm_search_by_projection_sim3_batch(ccm_ctx*, int n_kf, const ccm_frame_grid* kfs, const float* scale_factors, const int32_t* mp_first,
                                        const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* mp_desc,
                                        const uint8_t* observed, uint8_t* matched, float th, int32_t* best_idx, int32_t* n_matches);

/* ORBmatcher::SearchForTriangulation (ORBmatcher.cpp:700-852): per feature of KF1 without a map point, the most
 * similar (<= TH_LOW, last one among equals) feature of KF2 in the same vocabulary node that has no map point, is
 * not near the epipole (ex, ey) (:775-777) and fulfils the epipolar constraint of F12 (row-major 3x3 float,
 * CheckDistEpipolarLine :159-176); rotation-histogram filter when check_ori.  match12[i1] = i2 or -1 (the caller
 * lists the pairs in i1 order, :843-849).  Returns nmatches. */
int ccm_search_for_triangulation(ccm_ctx*, const uint8_t* desc1, const int32_t* node1, const uint8_t* has_mp1, const float* x1, const float* y1,
                                 const float* angle1, int n1, const uint8_t* desc2, const int32_t* node2, const uint8_t* has_mp2,
                                 const float* x2, const float* y2, const float* angle2, const int32_t* octave2, int n2, const float* F12,
                                 float ex, float ey, const float* scale_factors2, const float* level_sigma2_2, int check_ori, int32_t* match12);

/* ---------------------------------------------------------------- vocabulary tree
 * DBoW2::TemplatedVocabulary (cslam/thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h).  A vocabulary is handed over as
 * the arrays loadFromTextFile (:1338-1423) fills: node 0 = root, parent[i] < i, descriptors [n_nodes][32], weights
 * [n_nodes]; children keep node-id order, a node without children is a word, words are numbered in node order.
 * The tree lives on the context's device until ccm_voc_destroy. */
typedef struct ccm_vocabulary ccm_vocabulary;
int  ccm_voc_create(ccm_ctx*, int k, int L, int n_nodes, const int32_t* parent, const uint8_t* descriptors, const double* weights,
                    ccm_vocabulary** out);
void ccm_voc_destroy(ccm_vocabulary*);
int  ccm_voc_words(const ccm_vocabulary*);

/* transform(feature, word_id, weight, nid, levelsup) (:1217-1258) for n features: the L-level k-way Hamming descent.
 * node_id = the node at level L - levelsup (0 = root when that is <= 0 or the branch ends above it).  The _dev form
 * takes descriptors resident on the device (ccm_orb_result_dev); results are host arrays.  Its features_dev must be
 * 16-byte aligned (CCM_E_ARG otherwise), as for ccm_hamming_match_dev, and is read on the vocabulary's context's stream. */
int ccm_voc_transform(ccm_vocabulary*, const uint8_t* features, int n, int levelsup, int32_t* word_id, double* weight, int32_t* node_id);
int ccm_voc_transform_dev(ccm_vocabulary*, const uint8_t* features_dev, int n, int levelsup, int32_t* word_id, double* weight,
                          int32_t* node_id);

/* transform(features, BowVector&, FeatureVector&, levelsup) (:1125-1193) from the per-feature results: out_id/out_val
 * (room for n entries) = the BowVector in key order after the weighting (0 TF_IDF, 1 TF, 2 IDF, 3 BINARY) and the
 * normalisation the scoring type asks for (0 L1_NORM ... 5 DOT_PRODUCT, BowVector.h:36-53); fv_node[i] = FeatureVector
 * node of feature i, -1 when its word is stopped -- the per-feature form ccm_match_bow takes.  Returns the size. */
int ccm_bow_vector(int n, const int32_t* word_id, const double* weight, const int32_t* node_id, int weighting, int scoring,
                   int32_t* out_id, double* out_val, int32_t* fv_node);
/* L1Scoring::score (ScoringObject.cpp:23-68) of two BowVectors in key order */
double ccm_bow_score_l1(int n1, const int32_t* id1, const double* v1, int n2, const int32_t* id2, const double* v2);

/* MapPoint::ComputeDistinctiveDescriptors (cslam/src/MapPoint.cpp:929-994) for n_points map points: the observed
 * descriptors of point p are desc[first[p] .. first[p]+count[p]); best[p] = index (within the point) of the descriptor
 * with the least median distance to the others, first among equals; -1 for count 0. */
int ccm_distinctive_descriptors(ccm_vocabulary*, const uint8_t* desc, const int64_t* first, const int32_t* count, int n_points,
                                int32_t* best);

/* ---------------------------------------------------------------- optimizer
 * The 6-DoF pose / 3-DoF point reprojection BA that Optimizer::BundleAdjustmentClient
 * (src/Optimizer.cpp:32-212), LocalBundleAdjustmentClient (:349-644) and
 * MapFusionGBA (:646-865) hand to g2o: EdgeSE3ProjectXYZ residual/Jacobian
 * (thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:103-147), Huber kernel,
 * BlockSolver_6_3 Schur complement (core/block_solver.hpp:354-486) and the
 * Levenberg loop (core/optimization_algorithm_levenberg.cpp:61-189).          */
typedef struct {
    int      n_poses;
    double*  poses;        /* [n_poses][7]: unit quaternion (x,y,z,w) then t (x,y,z) = SE3Quat of Tcw; in/out */
    const uint8_t* fixed;  /* [n_poses] 1 = setFixed(true) */
    const double*  intr;   /* [n_poses][4] fx,fy,cx,cy */
    int      n_points;
    double*  points;       /* [n_points][3] world xyz; in/out */
    int      n_edges;
    const int32_t* edge_pose;   /* [n_edges] */
    const int32_t* edge_point;  /* [n_edges] */
    const double*  obs;         /* [n_edges][2] u,v */
    const double*  info;        /* [n_edges] invSigma2 (information = info * I2) */
} ccm_ba_problem;

typedef struct {
    int    iterations;     /* optimize(n) */
    double huber_delta;    /* thHuber2D; <= 0 -> no robust kernel */
    /* Local BA's second stage (Optimizer.cpp:546-568): after `iterations`, mark
     * edges with chi2 > outlier_chi2 or non-positive depth as level 1, drop the
     * kernels and run `iterations2` more.  iterations2 <= 0 -> single stage. */
    int    iterations2;
    double outlier_chi2;   /* 5.991 */
    const volatile uint8_t* stop_flag; /* pbStopFlag, polled between LM iterations/trials; may be NULL */
    /* Relative residual |H dx - b| / |b| at which the iterative reduced-camera solve stops; 0 = default 1e-7,
     * the tightest the pipelined iteration takes.
     * The reference solves directly (sparse Cholesky); measured on config 5 the poses after 5 iterations differ from
     * a 1e-13 solve by 6e-13 (1e-11), 6e-11 (1e-9), 6e-9 (1e-7), 5e-7 (1e-5) against the 1e-5 contract; over the
     * reference's optimize(20) (9 iterations, LM corrects earlier inexactness) the final poses differ from the oracle's by
     * 2e-9 (1e-8), 9e-9 (1e-6), 2e-7 (1e-5), 1e-6 (1e-4), with identical iteration and trial counts and chi2 equal to 1e-11.
     * Config 5 would keep three orders of magnitude to the contract at 1e-6, but the error is cond(H) x tolerance x step: on a
     * 257-keyframe arc with one or two fixed keyframes 1e-6 leaves 2.7e-5 after 3 iterations (contract missed), 1e-7 2.8e-6 for
     * a fifth more PCG iterations (tests/test_ba_cases_gpu.py), with the classic and the pipelined iteration alike. */
    double pcg_tol;
} ccm_ba_options;

typedef struct {
    int    iterations_done;   /* LM iterations run, both stages */
    int    trials;            /* linear solves */
    double chi2_initial;      /* activeRobustChi2 before the first iteration */
    double chi2_final;        /* activeRobustChi2 at the last accepted state */
    double lambda_final;
    int    stopped;           /* 1 if stop_flag ended the solve */
    /* per-stage wall seconds, mirroring G2OBatchStatistics (core/batch_stats.h).  They always add up to the LM loop's wall time;
     * below 200,000 edges the stream is not synchronised at every phase boundary (that cost a quarter of a local BA), so a phase's
     * GPU time is booked where the next necessary synchronisation falls (CCM_BA_TIMERS=1 forces exact phases). */
    double t_linearize, t_schur, t_solve, t_update;
    uint8_t* edge_outlier;    /* optional out [n_edges]: chi2 > outlier_chi2 || depth <= 0 at the end (:582) */
    /* structure of the reduced camera system and work of its solver */
    int32_t schur_blocks;     /* non-zero 6x6 blocks (upper triangle) */
    int64_t schur_pairs;      /* (landmark, pose-pair) contributions on this rank */
    int32_t pcg_iterations;   /* conjugate-gradient iterations, all trials (0 on the dense path) */
    int32_t pcg_fallbacks;    /* trials whose first solver gave up (pipelined -> classic PCG, PCG -> dense solve) */
    int32_t pcg_pipelined;    /* 1 = the two-kernel pipelined PCG iteration ran (pcg_tol >= 1e-7), 0 = the classic one or the dense solve */
} ccm_ba_result;

int ccm_ba_solve(ccm_ctx*, ccm_ba_problem*, const ccm_ba_options*, ccm_ba_result*);

/* Optimizer::PoseOptimizationClient (src/Optimizer.cpp:215-347), batched over frames: one free pose per
 * frame, one unary EdgeSE3ProjectXYZOnlyPose per frame feature with a MapPoint, Huber sqrt(5.991), four
 * rounds of optimize(10) restarted from the input pose, chi2 > 5.991 relabels outliers after each round.
 * Correspondences of frame f are rows first[f] .. first[f+1]-1 of points/obs/info.  On return poses holds
 * the optimised Tcw, outlier[] is Frame::mvbOutlier, n_inliers[f] the function's return value
 * (nInitialCorrespondences - nBad; 0 with fewer than 3 correspondences, pose untouched). */
typedef struct {
    int            n_frames;
    double*        poses;      /* [n_frames][7] in/out */
    const double*  intr;       /* [n_frames][4] fx fy cx cy */
    const int32_t* first;      /* [n_frames+1] */
    const double*  points;     /* [first[n_frames]][3] MapPoint world positions */
    const double*  obs;        /* [..][2] undistorted keypoints */
    const double*  info;       /* [..] invSigma2 of the keypoint's octave */
    uint8_t*       outlier;    /* [..] out */
    int32_t*       n_inliers;  /* [n_frames] out */
} ccm_pose_problem;
int ccm_pose_optimize(ccm_ctx*, ccm_pose_problem*);

/* ------------------------------------------------------------------ frame handles
 * One tracked image is matched and posed several times (TrackWithMotionModel, src/Tracking.cpp:571-597: SearchByProjection
 * (Current, Last), maybe again with a wider window, then PoseOptimizationClient; TrackLocalMap, :905-920: SearchByProjection
 * (Frame, local map points), then PoseOptimizationClient again; on the next image it is mLastFrame).  A ccm_frame keeps one
 * Frame's undistorted keypoints (mvKeysUn: x, y, octave, angle), mDescriptors, its feature grid (mGrid, built on the device)
 * and mvpMapPoints (as ids into the caller's map-point table, -1 = none) in device memory for the frame's lifetime, so the
 * per-frame calls below upload only their per-call inputs (one page-locked staging copy) and return with one download.
 * A frame belongs to the context that made it: passing it with another context returns CCM_E_ARG.  Frames should be destroyed
 * before their context; ccm_destroy releases the device memory of frames still alive, which then only accept ccm_frame_destroy
 * (and ccm_frame_size); every other call on them returns CCM_E_STATE.  Creating and destroying one frame per image recycles
 * device memory through a pool on the context: no hipMalloc in steady state. */
typedef struct ccm_frame ccm_frame;
/* Frame constructor's host side (src/Frame.cpp:80-118): the features g describes (g->kp_x/kp_y = mvKeysUn, octave, desc) and
 * their grid geometry; angle[n] = mvKeysUn[i].angle or NULL (the frame then takes no part in an orientation-checked
 * frame-to-frame match: such a call returns CCM_E_ARG).  Uploads once and builds the grid on the device (AssignFeaturesToGrid). */
int ccm_frame_create(ccm_ctx*, const ccm_frame_grid* g, const float* angle, ccm_frame** out);
/* The same from image `image` of the last ccm_orb_extract / ccm_orb_extract_dev on this context: octave, angle and descriptor
 * rows are copied device to device.  kp_x_un / kp_y_un [n]: the caller's undistorted coordinates (Frame::UndistortKeyPoints,
 * src/Frame.cpp:277), or NULL for the extracted ones (the zero-distortion early return).  n = keypoint count, or -1 to read it
 * (synchronises).  The frame owns its copies: a later extract does not touch it.  CCM_E_STATE: no extract on this context yet;
 * CCM_E_ARG: image out of range, n above the extract's max_per_image. */
int ccm_frame_from_extract(ccm_ctx*, int image, int n, const float* kp_x_un, const float* kp_y_un, float min_x, float min_y,
                           float inv_w, float inv_h, int grid_cols, int grid_rows, ccm_frame** out);
/* The camera of a Frame: mK (fx, fy, cx, cy) and mDistCoef (k1, k2, p1, p2 and k3, the fifth coefficient that src/Tracking.cpp:53-58
 * appends only when it is not zero: 0 here when absent), as the float values the reference stores. */
typedef struct {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
} ccm_camera;
/* Frame::mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv (src/Frame.cpp:87-88, :309-337). */
typedef struct {
    float min_x, max_x, min_y, max_y;
    float inv_w, inv_h;
} ccm_frame_bounds;
/* Frame::UndistortKeyPoints (src/Frame.cpp:277-307) on n points; host only, no context, no GPU.  cv::undistortPoints as Frame.cpp:295
 * calls it (R empty, P = mK) in its classic fixed-count form: with the float camera values and the float point widened to double,
 *   x0 = x = (u - cx) * (1 / fx), y0 = y = (v - cy) * (1 / fy); exactly 5 times { r2 = x*x + y*y;
 *   icdist = 1 / (1 + ((k3*r2 + k2)*r2 + k1)*r2); dx = ((2*p1)*x)*y + p2*(r2 + (2*x)*x); dy = p1*(r2 + (2*y)*y) + ((2*p2)*x)*y;
 *   x = (x0 - dx)*icdist; y = (y0 - dy)*icdist }; u' = (float)(fx*x + cx), v' = (float)(fy*y + cy),
 * every operation one IEEE double operation in that order.  Five iterations are not converged (up to 0.56 px from the fixed point for
 * the EuRoC camera): the count is part of the definition.  k1 == 0 copies the input whatever the other coefficients are (the early
 * return of :279-283).  x_un / y_un may be x / y.  CCM_E_ARG: a NULL pointer with n > 0, n < 0, fx == 0 or fy == 0. */
int ccm_undistort_points(const ccm_camera* cam, int n, const float* x, const float* y, float* x_un, float* y_un);
/* Frame::ComputeImageBounds (src/Frame.cpp:309-337) with the grid element sizes of :87-88; host only.  The four corners (0,0),
 * (width,0), (0,height), (width,height) undistorted as above: min_x = min(x0, x2), max_x = max(x1, x3), min_y = min(y0, y1),
 * max_y = max(y2, y3); with k1 == 0 the bounds are 0, width, 0, height.  inv_w = (float)grid_cols / (max_x - min_x) and inv_h likewise,
 * in float.  CCM_E_ARG: a NULL pointer, width, height, grid_cols or grid_rows < 1, a zero focal length. */
int ccm_image_bounds(const ccm_camera* cam, int width, int height, int grid_cols, int grid_rows, ccm_frame_bounds* out);
/* ccm_frame_from_extract with Frame::UndistortKeyPoints (src/Frame.cpp:277-307) done on the device from the extract's own keypoints,
 * in the kernel that builds the handle: nothing is uploaded apart from the kernel arguments, and the handle equals the one
 * ccm_frame_from_extract makes from ccm_undistort_points' output and the same bounds.  cam == NULL or cam->k1 == 0: the extracted
 * coordinates.  b gives min_x, min_y, inv_w, inv_h of the grid (ccm_image_bounds; max_x / max_y are not read).  Errors as
 * ccm_frame_from_extract; CCM_E_ARG also for b == NULL or a zero focal length. */
int ccm_frame_from_extract_camera(ccm_ctx*, int image, int n, const ccm_camera* cam, const ccm_frame_bounds* b, int grid_cols,
                                  int grid_rows, ccm_frame** out);
/* The Frame constructors (src/Frame.cpp:80-118 with :277-307) of n_images consecutive images of the last extract, first_image
 * onwards: one read-back of their counts (synchronises), one staged upload of the per-frame records and one launch, a workgroup per
 * frame.  cam may be NULL (the batched form of ccm_frame_from_extract without coordinate arrays).  All or nothing: on any error every
 * handle made so far is released and out[] is all NULL.  n_images == 0 is CCM_OK.  CCM_E_STATE: no extract on this context yet;
 * CCM_E_ARG: the range leaves the extract's images, b == NULL, a zero focal length. */
int ccm_frames_from_extract_camera(ccm_ctx*, int first_image, int n_images, const ccm_camera* cam, const ccm_frame_bounds* b,
                                   int grid_cols, int grid_rows, ccm_frame** out /* [n_images] */);
/* Frame::mvKeysUn[i].pt (src/Frame.cpp:297-306) read back from the handle: kx, ky [N], either may be NULL.  Synchronises.
 * CCM_E_STATE on a handle that outlived its context. */
int ccm_frame_get_keypoints(ccm_frame*, float* kx, float* ky);
/* NULL is a no-op. */
void ccm_frame_destroy(ccm_frame*);
/* Frame::N, or CCM_E_ARG for NULL. */
int ccm_frame_size(const ccm_frame*);
/* Frame::mvpMapPoints as ids (-1 = none); set(NULL) = all -1, the fill(..., nullptr) of Tracking.cpp:579, :589.  set is also how
 * the caller applies "discard outliers" (:599-618). */
int ccm_frame_set_map_points(ccm_frame*, const int32_t* mp_id);
int ccm_frame_get_map_points(ccm_frame*, int32_t* mp_id);
/* Test tap (host copies, synchronises): cell_first[cols*rows+1], cell_items[cell_first[cols*rows]] with cell k = px*rows + py,
 * features of a cell in ascending index, as ccm_window_candidates builds the grid from host arrays. */
int ccm_frame_debug_grid(ccm_frame*, int32_t* cell_first, int32_t* cell_items);
/* KeyFrame side of a frame handle: what LocalMapping reads of a keyframe beyond the Frame data (CreateNewMapPoints, src/Mapping.cpp:
 * 284-469, with SearchForTriangulation, ORBmatcher.cpp:700-852).  All three are optional, may come in any order and may be repeated;
 * they are asynchronous on the context's stream and in effect for the next call.  A keyframe's features never change, so a handle is
 * made once per keyframe; what changes later is mp_id (ccm_frame_set_map_points) and the pose.  Once bow and camera are both set the
 * device keeps the features that have a node ordered by (node, feature index) -- the order DBoW2 fills a FeatureVector in -- with
 * node-ordered copies of their descriptors (about 52 bytes per feature in a second pooled block).  On an error the handle keeps its
 * previous state; on a handle that outlived its context they return CCM_E_STATE.
 * set_bow: node[n] = FeatureVector node per feature (mFeatVec, KeyFrame::ComputeBoW), -1 = none, < 2^24 as ccm_map_keyframe.node;
 * NULL clears it.  CCM_E_ARG names the feature whose node is >= 2^24, or n when it is above 2^20 - 1.
 * set_camera: fx, fy, cx, cy, mvScaleFactors and mvLevelSigma2 (:292-305).  CCM_E_ARG when a table is NULL or n_levels is below the
 * handle's own n_levels (1 + the largest octave of ccm_frame_create, the extractor's levels of ccm_frame_from_extract) or above 256.
 * set_pose: GetRotation / GetTranslation as the rows of [Rcw | tcw], and GetCameraCenter as the keyframe stores it (:337-349). */
int ccm_frame_set_bow(ccm_frame*, const int32_t* node);
int ccm_frame_set_camera(ccm_frame*, float fx, float fy, float cx, float cy, const float* scale_factors, const float* level_sigma2, int n_levels);
int ccm_frame_set_pose(ccm_frame*, const float* Tcw /* [12] rows of [Rcw|tcw] */, const float* Ow /* [3] */);
/* Test tap (synchronises): order[n_with_node] the features that have a node by (node, index), nodes[n_nodes] the distinct nodes
 * ascending, first[n_nodes+1] their first positions in order; returns n_nodes.  Room for n, n and n + 1 entries always suffices.
 * CCM_E_STATE without a bow. */
int ccm_frame_debug_bow(ccm_frame*, int32_t* order, int32_t* nodes, int32_t* first);
/* ccm_fuse_select_batch (ORBmatcher::Fuse, ORBmatcher.cpp:854-1000, for the first loop of SearchInNeighbors, src/Mapping.cpp:
 * 471-547) with the keyframes taken from handles: their device arrays and device-built grids are used as they are, nothing of a
 * keyframe is uploaded or rebuilt.  Same outputs.  The handles need neither bow, camera nor pose; the same handle may appear more
 * than once.  inv_level_sigma2 (chi2_check) holds at least the largest n_levels among the handles. */
int ccm_fuse_select_batch_frames(ccm_ctx*, int n_kf, ccm_frame* const* kfs, const float* scale_factors, const float* inv_level_sigma2,
                                 const int32_t* mp_first, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                                 const uint8_t* mp_desc, float th, int chi2_check, int accept_th, int32_t* best_idx, int32_t* best_dist);
/* ccm_search_by_projection (ORBmatcher.cpp:71-148) with the frame side taken from the handle; same results.  occupied [N] stays
 * host in/out (the caller computes Observations() > 0).  For every newly matched feature i the handle's mp_id[i] becomes
 * query_mp_id[q], or q when query_mp_id is NULL. */
int ccm_frame_search_by_projection(ccm_ctx*, ccm_frame* f, const float* scale_factors, int n_mp, const uint8_t* in_view,
                                   const int32_t* level, const float* view_cos, const float* proj_x, const float* proj_y,
                                   const uint8_t* mp_desc, const uint8_t* mp_has_obs, const int32_t* query_mp_id,
                                   uint8_t* occupied, float th, float nnratio, int32_t* match);
/* ccm_search_by_projection_frame, both overloads (ORBmatcher.cpp:1350-1476, :1478-1605), cur_angle from `cur`.  last != NULL:
 * n_last must equal its N, and the octaves, the angles and (when query_mp_id is NULL) the map-point ids come from the handle
 * (CurrentFrame.mvpMapPoints[i2] = LastFrame.mvpMapPoints[i], :1442); last_octave / last_angle may then be NULL.  last == NULL:
 * the arrays are used (the relocalisation overload with a keyframe's points) and new ids are query_mp_id[i] or i. */
int ccm_frame_search_by_projection_frame(ccm_ctx*, ccm_frame* cur, const ccm_frame* last, const float* scale_factors, int n_last,
                                         const uint8_t* valid, const float* u, const float* v, const int32_t* last_octave,
                                         const float* last_angle, const uint8_t* mp_desc, const uint8_t* mp_has_obs,
                                         const int32_t* query_mp_id, uint8_t* occupied, float th, int check_ori, int orb_dist,
                                         int32_t* match);
/* Optimizer::PoseOptimizationClient (src/Optimizer.cpp:215-347) for one frame.  Correspondences = the features with
 * mp_id >= 0 in feature order: obs = the handle's undistorted coordinates widened to double, info = inv_level_sigma2[octave],
 * point = mp_xyz[mp_id] ([n_mp][3]).  pose7 in/out, outlier[N] per feature (0 where there is no point), *n_inliers = the
 * function's return value -- the values ccm_pose_optimize gives for the problem shim/cslam_optimizer.cpp assembles.  An mp_id
 * outside [0, n_mp) or an octave outside [0, n_levels) returns CCM_E_ARG with the outputs untouched. */
int ccm_frame_pose_optimize(ccm_ctx*, ccm_frame* f, int n_mp, const double* mp_xyz, const float* inv_level_sigma2, int n_levels,
                            const double intr[4], double pose7[7], uint8_t* outlier, int32_t* n_inliers);
/* Tracking::TrackReferenceKeyFrame (src/Tracking.cpp:514-556) and the front of loop / map matching on handles: the three calls
 * below replace Frame::ComputeBoW, SearchByBoW(KeyFrame, Frame) and the per-candidate SearchByBoW(KeyFrame, KeyFrame) loop for
 * features that already lie in device memory.
 *
 * ccm_frame_compute_bow: Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cpp:268-275).  The vocabulary descent of
 * ccm_voc_transform_dev runs on the handle's own descriptor rows and the node directory of ccm_frame_set_bow is built on the device
 * (frames above 4096 features: on the host): nothing of the frame is uploaded.  A feature whose word has weight <= 0 (a stopped
 * word, TemplatedVocabulary.h:1170-1190) gets node -1, as fv_node of ccm_bow_vector.  Afterwards the handle is in the state
 * ccm_frame_set_bow leaves with the same nodes.  word_id / weight / node [N] are optional (all three or none): the per-feature
 * results of ccm_voc_transform_dev with node = -1 for stopped words, which feed ccm_bow_vector for the caller's mBowVec; without them
 * the call reads back two counters.  An empty vocabulary gives a bow with no feature in it (word 0, weight 0, node -1).
 * CCM_E_ARG, the handle's bow as before: a vocabulary or a handle of another context, a vocabulary of 2^24 nodes or more, N above
 * 2^20 - 1, only some of the three outputs.  CCM_E_STATE: a handle that outlived its context. */
int ccm_frame_compute_bow(ccm_ctx*, ccm_frame* f, ccm_vocabulary* voc, int levelsup, int32_t* word_id, double* weight, int32_t* node);
/* ccm_match_bow's Frame overload (ORBmatcher.cpp:178-306) on two handles that both have a bow (set_bow or compute_bow, in any mix):
 * descriptors, angles and FeatureVector order are the handles', the group list is made on the device.  valid1 [N_kf] or NULL = kf's
 * mp_id >= 0.  match [N_f] = the feature of kf matched to frame feature i, or -1 (vpMapPointMatches[idx2], :251).  Returns nmatches;
 * if and only if that is >= min_matches (Tracking.cpp:526-529) the frame's mp_id is replaced as a whole: kf's mp_id of the matched
 * feature, -1 elsewhere (mCurrentFrame->mvpMapPoints = vpMapPointMatches).  One upload (valid1, when given), one download.
 * Errors leave match and mp_id untouched: CCM_E_ARG for a handle of another context, kf == f, check_ori with a handle created
 * without angles; CCM_E_STATE for a handle without a bow or one that outlived its context. */
int ccm_frame_search_by_bow(ccm_ctx*, const ccm_frame* kf, ccm_frame* f, const ccm_bow_options*,
                            const uint8_t* valid1 /* [N_kf] or NULL: kf's mp_id >= 0 */,
                            int min_matches, int32_t* match /* [N_f]: feature of kf, or -1 */);
/* ccm_match_bow's KeyFrame-KeyFrame overload (ORBmatcher.cpp:565-698; strict_th is taken as 1) for kf1 against n_kf2 candidates in
 * three launches, whatever n_kf2: the loop of LoopFinder::ComputeSim3 (src/LoopFinder.cpp:265) and MapMatcher (src/MapMatcher.cpp:
 * 271) in front of the batched Sim3Solver.  valid1 [N1] or NULL = kf1's mp_id >= 0; valid2 = the candidates' masks concatenated,
 * candidate k at first2[k] .. first2[k+1] (which must span its N), or NULL = each candidate's mp_id >= 0 (first2 may then be NULL).
 * match12 [n_kf2][N1] and nmatches [n_kf2]: per candidate what ccm_match_bow returns for that pair.  The same handle may appear
 * twice; n_kf2 = 0 returns CCM_OK.  Errors as ccm_frame_search_by_bow, naming kfs2[k]; the outputs stay untouched. */
int ccm_search_by_bow_frames(ccm_ctx*, const ccm_frame* kf1, int n_kf2, ccm_frame* const* kfs2, const ccm_bow_options*,
                             const uint8_t* valid1 /* [N1] or NULL */, const int32_t* first2 /* [n_kf2+1] */,
                             const uint8_t* valid2 /* concatenated, or NULL: mp_id >= 0 */,
                             int32_t* match12 /* [n_kf2][N1] */, int32_t* nmatches /* [n_kf2] */);

/* ------------------------------------------------------------------ map-point table
 * The client's map points in device memory, one row per slot; a slot is the id the frame handles carry in mp_id.  The caller
 * assigns slots and sends rows when the map changes (keyframe rate: creation, culling, bundle adjustment); the per-frame calls below
 * (frame rate) then upload nothing of the map.  Columns: pos = mWorldPos, normal = mNormalVector, min_dist / max_dist = the raw
 * mfMinDistance / mfMaxDistance (the factors 0.8 / 1.2 of GetMin/MaxDistanceInvariance, src/MapPoint.cpp, are applied on the
 * device; PredictScale uses the raw maximum), desc = GetDescriptor(), flags = CCM_MP_*.  A fresh table holds zeros (no slot LIVE).
 * The table also keeps one `seen` stamp per slot that only ccm_frame_search_local_points writes.
 * Ownership as for frames: a table handle belongs to the context that made it (another context: CCM_E_ARG); after ccm_destroy it
 * accepts only ccm_map_table_destroy, ccm_map_table_capacity and ccm_map_table_handles, every other call returns CCM_E_STATE.
 *
 * Table views.  The reference runs Tracking, LocalMapping, LoopFinder, MapMatcher and MapMerger on threads of their own, each with a
 * context of its own, and all of them work on one map.  ccm_map_table_attach gives a context a handle of its own (a view) on the
 * ROWS of an existing table; a view is used exactly like a table, with the view's context, by every call that takes a table:
 * ccm_map_table_update, _set_order, _fetch, _refresh, _correct_frames, ccm_frame_search_local_points, ccm_frame_pose_optimize_table,
 * ccm_frame_track_motion_model, ccm_fuse_select_table_frames, ccm_search_by_sim3_table_frames and
 * ccm_search_by_projection_table_frames.  The frame handles and vocabularies such a call names belong to that same context.
 *   Shared between the handles of the same rows: the columns pos, normal, min_dist, max_dist, desc and flags, and the capacity.
 *   Owned by each handle: the `seen` column and its stamp (ccm_map_table_fetch returns the calling handle's), the visiting order
 *   (ccm_map_table_set_order), and the scratch of the Fuse and ComputeSim3 calls.
 *   Visibility: rows written through one handle (ccm_map_table_update, _refresh, _correct_frames) are seen by every call through any
 *   handle that starts after the writing call has returned, also where that call returned without synchronising (_update, and
 *   _refresh without a result): the later call's stream is made to wait for the write.
 *   Concurrency: calls on handles of the same rows may be made from different threads at the same time, each thread with its own
 *   context.  A call that writes rows excludes every other call on those rows for its duration, calls that only read them overlap,
 *   and the outcome equals that of some serial order of the calls.  Two threads still never share one context or one handle.
 *   Lifetime: the rows live until their last handle is destroyed or orphaned.  Destroying the first table leaves its views working;
 *   ccm_destroy of a context orphans that context's handles only.
 * A table nobody attached to behaves and costs as before: it records no event and waits for none. */
enum { CCM_MP_LIVE = 1,      /* the slot is in use */
       CCM_MP_BAD = 2,       /* MapPoint::isBad() */
       CCM_MP_HAS_OBS = 4 }; /* Observations() > 0 */
typedef struct ccm_map_table ccm_map_table;
int  ccm_map_table_create(ccm_ctx*, int capacity, ccm_map_table** out);   /* capacity >= 1 */
void ccm_map_table_destroy(ccm_map_table*);                               /* NULL is a no-op */
int  ccm_map_table_capacity(const ccm_map_table*);                        /* or CCM_E_ARG for NULL */
/* A further handle, owned by context c, on the ROWS of `table` (which may itself be such a handle).  c may be the context of `table`:
 * a second handle with scratch of its own.  Called on c's thread; it touches nothing of the other context (the first attach to a
 * table waits once for the device, so that rows written before it are seen).  CCM_E_ARG: a NULL argument, a context on another
 * device.  CCM_E_STATE: `table` outlived its context.  On any failure *view = NULL.  Destroy a view with ccm_map_table_destroy. */
int  ccm_map_table_attach(ccm_ctx* c, ccm_map_table* table, ccm_map_table** view);
/* Test tap: the number of live handles that share this handle's rows (1 for a table nobody attached to); CCM_E_ARG for NULL, 0 for
 * an orphan. */
int  ccm_map_table_handles(const ccm_map_table*);
/* Rows to write.  A NULL column keeps that column of the listed slots (bundle adjustment moves positions only, culling changes
 * flags only).  A slot listed twice takes its last row. */
typedef struct {
    int32_t        n;
    const int32_t* slot;      /* [n], each in [0, capacity) */
    const float*   pos;       /* [n][3] or NULL */
    const float*   normal;    /* [n][3] or NULL */
    const float*   min_dist;  /* [n] or NULL */
    const float*   max_dist;  /* [n] or NULL */
    const uint8_t* desc;      /* [n][32] or NULL */
    const uint8_t* flags;     /* [n] or NULL */
} ccm_map_update;
/* One page-locked staging copy and one scatter launch, asynchronous on the context's stream.  A slot outside [0, capacity) returns
 * CCM_E_ARG with the table untouched (checked on the host before anything is queued).  n == 0 is OK. */
int ccm_map_table_update(ccm_ctx*, ccm_map_table*, const ccm_map_update*);
/* The order in which ccm_frame_search_local_points visits the map points: slots [n].  The reference iterates mmpMapPoints, a
 * std::map keyed by (id, client id) (Map::GetAllMapPoints, src/Map.cpp), and SearchByProjection depends on the order; the caller
 * sends the list again only when the set of points changes.  slots == NULL: ascending slot over all LIVE slots, what a
 * single-client map gives (the state of a fresh table).  A duplicate or a slot outside [0, capacity) returns CCM_E_ARG and keeps
 * the previous order. */
int ccm_map_table_set_order(ccm_ctx*, ccm_map_table*, int n, const int32_t* slots);
/* Test tap (synchronises): the rows of slots [n] copied to the host; every output may be NULL.  seen [n] = the slot's stamp. */
int ccm_map_table_fetch(ccm_ctx*, ccm_map_table*, int n, const int32_t* slot, float* pos, float* normal, float* min_dist,
                        float* max_dist, uint8_t* desc, uint8_t* flags, int32_t* seen);
/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823) for a list of
 * map points, read from keyframe handles and written into the table: what LocalMapping calls on every point it touched after
 * CreateNewMapPoints, after Fuse (src/Mapping.cpp:471-559) and after a bundle adjustment (src/Optimizer.cpp:203, :636, :851).  The
 * descriptors (ccm_frame_create), the camera centres (ccm_frame_set_pose), the scale factors (ccm_frame_set_camera) and the positions
 * already lie in device memory; the call uploads the index lists only.
 *   Observations: point p owns entries obs_first[p] .. obs_first[p+1] of obs_kf / obs_feat: mObservations in the caller's iteration
 *   order (the reference's std::map is ordered by pointer value, so the caller fixes the order) without the entries whose keyframe
 *   isBad() (:803, :952).  ref_kf / ref_feat = mpRefKF and mObservations[mpRefKF], which the reference reads whether or not that
 *   keyframe is bad; they are ignored for a point without observations.
 *   A point without observations (both functions return early): desc, normal, min_dist and max_dist of its row stay, best = -1;
 *   pos and flags are still written when given.
 *   CCM_MPR_DESCRIPTOR: best[p] = what ccm_distinctive_descriptors returns for the point's descriptors in list order (the least
 *   median of its row of Hamming distances, k = (int)(0.5 * (c - 1)), the first among equal medians), and the row's desc becomes
 *   that observation's 32 bytes.  Without this bit best[p] = -1.
 *   CCM_MPR_NORMAL_DEPTH, in the arithmetic of a float cv::Mat as OpenCV's expression templates evaluate :797-822, with P the row's
 *   pos after the optional write and c the number of observations:
 *     normal = (0, 0, 0);  for each observation in list order, Ow of its keyframe:
 *       d = P - Ow (float);  nrm = sqrt((double)d0*d0 + (double)d1*d1 + (double)d2*d2)  (cv::norm returns a double)
 *       a = (float)(1.0 / nrm);  normal[k] = d[k] * a + normal[k]  (cv::scaleAdd: a float multiply, then a float add, not fused)
 *     normal[k] = normal[k] * (float)(1.0 / (double)c)   (Mat / n multiplies by the reciprocal)
 *     PC = P - Ow_ref (float);  dist = (float)sqrt(sum (double)PC^2);  level = octave_ref[ref_feat]
 *     max_dist = dist * sf_ref[level];  min_dist = max_dist / sf_ref[n_levels_ref - 1]  (float; n_levels of ccm_frame_set_camera)
 *   A point that coincides with a camera centre gives NaN, as in the reference.  An OpenCV built with FMA dispatch may fuse the
 *   multiply-add of scaleAdd; the library's reading is the unfused one.
 *   Columns `what` does not select are left as they are.
 * One page-locked staging copy up (index lists, optional pos / flags, one small view of device pointers per keyframe), one launch on
 * the context's stream, ordered with the other table calls: a ccm_frame_search_local_points issued afterwards sees the new rows.
 * result (optional, each field optional): best [n] as above; normal [n][3], min_dist [n], max_dist [n] = those columns of the listed
 * rows after the call, whether or not this call computed them.  With result == NULL or all four fields NULL the call neither
 * downloads nor synchronises; otherwise there is one download.
 * Errors are found on the host before anything is queued; the table and the outputs are then untouched.  CCM_E_ARG: a NULL required
 * array (slot, kfs, obs_first; obs_kf / obs_feat when there are observations; ref_kf / ref_feat with NORMAL_DEPTH), what == 0 or with
 * unknown bits, a slot out of range or listed twice, obs_first not ascending from 0, a keyframe index outside [0, n_kf), a feature
 * index outside that handle's [0, N) (the message names the point and the entry), a handle or table of another context.
 * CCM_E_STATE: a handle or table that outlived its context; with NORMAL_DEPTH an observed handle without a pose or a reference handle
 * without a pose or a camera (the message says which).  n == 0 returns CCM_OK. */
enum { CCM_MPR_DESCRIPTOR = 1,      /* MapPoint::ComputeDistinctiveDescriptors */
       CCM_MPR_NORMAL_DEPTH = 2 };  /* MapPoint::UpdateNormalAndDepth */
typedef struct {
    int32_t          n;          /* map points */
    const int32_t*   slot;       /* [n], each in [0, capacity), no slot twice */
    const float*     pos;        /* [n][3] written to the table first, or NULL: the table's pos is used */
    const uint8_t*   flags;      /* [n] written to the table, or NULL: kept */
    int32_t          n_kf;
    ccm_frame* const* kfs;       /* [n_kf] the keyframes the observations name; the same handle may appear twice */
    const int32_t*   obs_first;  /* [n+1] ascending, obs_first[0] == 0 */
    const int32_t*   obs_kf;     /* [obs_first[n]] index into kfs */
    const int32_t*   obs_feat;   /* [obs_first[n]] feature index in that keyframe */
    const int32_t*   ref_kf;     /* [n] mpRefKF as an index into kfs   (needed with NORMAL_DEPTH) */
    const int32_t*   ref_feat;   /* [n] observations[pRefKF]           (needed with NORMAL_DEPTH) */
    int32_t          what;       /* CCM_MPR_* or'ed, not 0 */
} ccm_map_refresh;
typedef struct { int32_t* best; float* normal; float* min_dist; float* max_dist; } ccm_map_refresh_result;  /* each [n] / [n][3], each optional */
int ccm_map_table_refresh(ccm_ctx*, ccm_map_table*, const ccm_map_refresh*, ccm_map_refresh_result* /* or NULL */);

/* Loop and merge corrections on the table: the step that moves keyframes and their map points, on keyframe handles and the table.
 *   CCM_MC_SIM3 + CCM_MC_IN_ORDER     LoopFinder::CorrectLoop (src/LoopFinder.cpp:543-613) and MapMerger::MergeMaps
 *                                     (src/MapMerger.cpp:349-392): for every corrected keyframe, in the iteration order of
 *                                     CorrectedSim3, the map points it owns become correctedSwi.map(Siw.map(P)) and
 *                                     UpdateNormalAndDepth runs on each at once; then the keyframe's pose becomes [R | t/s]
 *   CCM_MC_SIM3 + CCM_MC_POSES_FIRST  the tail of OptimizeEssentialGraphLoopClosure / MapFusion (src/Optimizer.cpp:1279-1330): every
 *                                     keyframe takes its pose, then every point moves through its reference keyframe and
 *                                     UpdateNormalAndDepth runs
 *   CCM_MC_RIGID                      the tail of the global BA (src/MapMerger.cpp:637-753 and its twin in LoopFinder): points outside
 *                                     the BA move as Rwc * (Rcw_before * P + tcw_before) + twc
 * Keyframes: kfs[0 .. n_moved) take a new pose, in the caller's iteration order; kfs[n_moved ..) are only read (their camera centres
 * and, as reference keyframes, their octaves and scale factors).  Points: row slot[p] is moved by keyframe owner[p] (an index into
 * the moved keyframes); owner[p] == -1 leaves the row exactly as it is.
 *   Position, CCM_MC_SIM3: pos[slot[p]] = (float)Q, Q = what ccm_correct_map_points gives for the point (double)pos[slot[p]] with
 *   ref_vertex = owner[p] and the same two Sim3 arrays, bit for bit (the widening is Converter::toVector3d, the narrowing
 *   Converter::toCvMat).
 *   Position, CCM_MC_RIGID, with Tb the owner handle's device pose when the call is made, Ta / Oa its Tcw_after / Ow_after:
 *     Xc[r] = (float)(((double)Tb[4r]*P[0] + (double)Tb[4r+1]*P[1] + (double)Tb[4r+2]*P[2]) + (double)Tb[4r+3])
 *     P'[r] = (float)(((double)Ta[r]*Xc[0] + (double)Ta[4+r]*Xc[1] + (double)Ta[8+r]*Xc[2]) + (double)Oa[r])
 *   that is Rwc * Xc + twc of GetPoseInverse (src/KeyFrame.cpp:299-306) as a float cv::Mat expression; nothing is fused.
 *   Poses: every moved keyframe's handle takes the new pose, on the device and in the handle's host copy; a handle without a keyframe
 *   block gets one, as ccm_frame_set_pose would give it.  SIM3: the pose is ccm_pose_to_camera((qx,qy,qz,qw, tx*(1.0/s), ty*(1.0/s),
 *   tz*(1.0/s))) of sim3_after (eigt *= (1./s), then toCvSE3).  RIGID: the given Tcw_after / Ow_after.
 *   Normal and depth (only with obs_first != NULL, the lists of ccm_map_refresh): for every point with owner >= 0 and at least one
 *   observation, exactly the arithmetic of CCM_MPR_NORMAL_DEPTH above on the new position.  The Ow of observing keyframe j and of the
 *   reference keyframe is chosen by `order`:
 *     CCM_MC_POSES_FIRST  the new Ow for every j < n_moved, the handle's Ow for the others
 *     CCM_MC_IN_ORDER     keyframe k's points are refreshed before k's own SetPose and after that of every earlier keyframe: the new
 *                         Ow iff j < owner[p], the handle's (old) Ow for j >= owner[p] and for every unmoved keyframe
 *   A point with owner >= 0 and no observations moves and keeps its normal, min_dist and max_dist.
 *   Untouched bit for bit: flags, desc, the seen stamps, and every row not listed or with owner == -1.
 * The outputs (each optional) report the listed rows as they stand after the call, rows with owner == -1 included.
 * The call is a writer of the table's rows (a view on another thread sees the new rows in any call that starts after this one
 * returns) and is ordered on the context's stream behind earlier ccm_frame_set_* / ccm_map_table_update / _refresh calls.  One
 * page-locked staging copy goes up: the Sim3 pairs or poses, slots, owners, the index lists and one small view of device pointers per
 * keyframe; nothing per point beyond 4-byte indices.  Three launches: the new poses into staging, the points (which read the
 * handles' old poses), the publish into the handles.  One download, and only if an output is given; otherwise the call neither
 * downloads nor synchronises.
 * Errors are found on the host before anything is queued; table, handles and outputs are then untouched.  CCM_E_ARG: a NULL required
 * array for the chosen transform (sim3_before / sim3_after or Tcw_after / Ow_after with n_moved > 0; slot and owner with points;
 * ref_kf / ref_feat with obs_first; obs_kf / obs_feat when there are observations), an unknown transform or order, n_moved outside
 * [0, n_kf], a handle twice, a slot out of range or twice, an owner outside [-1, n_moved), a non-finite Sim3 entry or s <= 0 in
 * sim3_after, the list errors of ccm_map_refresh (the message names the point and the entry), a handle or table of another context.
 * CCM_E_STATE: a handle or table that outlived its context; RIGID with an owner handle that has no pose; with lists, for the points
 * that move, an observed handle without a pose or a reference handle without a pose or a camera.
 * n_points == 0 still publishes the poses; n_moved == 0 with no points is CCM_OK. */
enum { CCM_MC_SIM3 = 0, CCM_MC_RIGID = 1 };          /* transform */
enum { CCM_MC_POSES_FIRST = 0, CCM_MC_IN_ORDER = 1 }; /* order */
typedef struct {
    int32_t           n_kf;
    ccm_frame* const* kfs;          /* [n_kf] every keyframe the call names; no handle twice */
    int32_t           n_moved;      /* kfs[0 .. n_moved) take a new pose, in the caller's iteration order; 0 <= n_moved <= n_kf */
    int32_t           transform;    /* CCM_MC_SIM3 or CCM_MC_RIGID */
    int32_t           order;        /* CCM_MC_POSES_FIRST or CCM_MC_IN_ORDER */
    const double*     sim3_before;  /* SIM3: [n_moved][8] qx,qy,qz,qw,tx,ty,tz,s  (g2oSiw / vScw) */
    const double*     sim3_after;   /* SIM3: [n_moved][8] CorrectedSiw */
    const float*      Tcw_after;    /* RIGID: [n_moved][12], rows of [Rcw|tcw], as ccm_frame_set_pose */
    const float*      Ow_after;     /* RIGID: [n_moved][3] */
    int32_t           n_points;
    const int32_t*    slot;         /* [n_points], each in [0, capacity), no slot twice */
    const int32_t*    owner;        /* [n_points] index into the moved keyframes, or -1: the row is left exactly as it is */
    const int32_t*    obs_first;    /* [n_points+1] the lists of ccm_map_refresh, or NULL: no normal / depth */
    const int32_t*    obs_kf;       /* [obs_first[n_points]] index into kfs */
    const int32_t*    obs_feat;     /* [obs_first[n_points]] feature index in that keyframe */
    const int32_t*    ref_kf;       /* [n_points] mpRefKF as an index into kfs */
    const int32_t*    ref_feat;     /* [n_points] observations[pRefKF] */
    float*            pos_out;      /* optional [n_points][3]: the rows after the call */
    float*            normal_out;   /* optional [n_points][3] */
    float*            min_dist_out; /* optional [n_points] */
    float*            max_dist_out; /* optional [n_points] */
} ccm_map_correct;
int ccm_map_table_correct_frames(ccm_ctx*, ccm_map_table*, const ccm_map_correct*);

/* Tracking::SearchLocalPoints (src/Tracking.cpp:860-922) with Frame::isInFrustum (src/Frame.cpp:139-198), MapPoint::PredictScale
 * (src/MapPoint.cpp:854-869) and ORBmatcher::SearchByProjection(Frame&, map points, th) (ORBmatcher.cpp:71-148) on a frame handle
 * and a table.
 *   First loop (:863-879): a feature whose mp_id names a BAD slot loses it (-1); the other slots the frame holds are stamped as seen
 *   and are not projected again; occupied[i] = HAS_OBS of the slot feature i keeps.  An mp_id outside the table or naming a slot
 *   that is not LIVE returns CCM_E_ARG with the handle's ids as they were.
 *   Second loop (:888-908) over the table's order: entries seen in this call, BAD or not LIVE are skipped; the others are tested as
 *   isInFrustum does, in the arithmetic of a float cv::Mat (products summed in double, stored as float):
 *     Pc[r] = (float)((double)R[r][0] P[0] + (double)R[r][1] P[1] + (double)R[r][2] P[2] + (double)t[r]);  reject PcZ < 0
 *     invz = 1.0f / PcZ;  u = fx * PcX * invz + cx;  v = fy * PcY * invz + cy  (float, left to right)
 *     reject u < min_x || u > max_x, then v < min_y || v > max_y
 *     PO = P - Ow (float);  dist = (float)sqrt(sum (double)PO^2);  reject dist < 0.8f * min_dist || dist > 1.2f * max_dist
 *     viewCos = (float)(sum (double)PO * Pn / (double)dist);  reject viewCos < viewing_cos_limit
 *     level = ceil(((float)log((double)(max_dist / dist))) / log_scale_factor), clamped to [0, n_levels - 1] (a NaN gives 0)
 *   The logarithm is the double one rounded to float -- the reference's log(float) is whichever overload its compiler picks.
 *   The entries in view, in visiting order, become the matcher's queries (radius 2.5 for viewCos > 0.998, else 4.0; times th unless
 *   th == 1; times scale_factors[level]; levels level-1 .. level) and are matched as ccm_frame_search_by_projection matches them.
 * Returns nmatches, or an error.  Nothing of the map is uploaded; the call synchronises twice (the in-view count, the result). */
typedef struct {
    float Tcw[12];             /* mRcw | mtcw, row-major 3x4 */
    float Ow[3];               /* mOw */
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;   /* mnMinX ... mnMaxY */
    float viewing_cos_limit;   /* 0.5 */
    float log_scale_factor;    /* mfLogScaleFactor */
    int32_t n_levels;          /* mnScaleLevels, 1..CCM_MAX_LEVELS */
    const float* scale_factors;/* [n_levels] mvScaleFactors */
    float th;                  /* 1, or 5 right after a relocalisation (:913-918) */
    float nnratio;             /* 0.8 */
} ccm_slp_params;
typedef struct {
    int32_t  n_to_match;       /* out: nToMatch, the number of entries in view */
    int32_t  in_view_cap;      /* in: room in in_view_slot and the taps; fewer than n_to_match: CCM_E_CAPACITY, the handle's ids as they were */
    int32_t* in_view_slot;     /* out [n_to_match]: the slots in view, in visiting order (IncreaseVisible, mbTrackInView) */
    float*   proj_x;           /* optional taps, one value per entry in view: mTrackProjX */
    float*   proj_y;           /*   mTrackProjY */
    int32_t* level;            /*   mnTrackScaleLevel */
    float*   view_cos;         /*   mTrackViewCos */
    int32_t* match;            /* out [N]: the slot newly assigned to feature i, or -1 */
    int32_t* mp_id;            /* out [N]: mvpMapPoints after the call (bad ones cleared, new ones set), as the handle holds them */
    uint8_t* occupied;         /* optional out [N]: feature i holds a map point with observations, after the call */
} ccm_slp_result;
int ccm_frame_search_local_points(ccm_ctx*, ccm_frame* f, ccm_map_table* table, const ccm_slp_params*, ccm_slp_result*);
/* Diagnostic tap: host wall time in milliseconds of the last ccm_frame_search_local_points on this context that reached its first
 * read-back.  ms[0]: from the entry to the read-back (queueing the first loop, the frustum test and the compaction); ms[1]: the
 * read-back of the count and the slot list (the copy and the wait for those kernels); ms[2]: the rest (taps, matcher, second
 * read-back, copies to the caller).  CCM_E_STATE before the first such call. */
int ccm_frame_search_local_points_timing(ccm_ctx*, double ms[3]);
/* ccm_frame_pose_optimize with the points taken from the table: pos is widened to double (Converter::toVector3d of a float cv::Mat
 * is exact), so the results equal ccm_frame_pose_optimize given mp_xyz = (double)pos bit for bit.  An mp_id outside the table or
 * naming a slot that is not LIVE returns CCM_E_ARG with the outputs untouched. */
int ccm_frame_pose_optimize_table(ccm_ctx*, ccm_frame* f, ccm_map_table* table, const float* inv_level_sigma2, int n_levels,
                                  const double intr[4], double pose7[7], uint8_t* outlier, int32_t* n_inliers);

/* Tracking::TrackWithMotionModel (src/Tracking.cpp:569-621) behind UpdateLastFrame and the pose product, in one call on two frame
 * handles and the table: ORBmatcher::SearchByProjection(Current, Last, th) (src/ORBmatcher.cpp:1350-1476, monocular), its repetition
 * with a window twice as wide, PoseOptimizationClient and "discard outliers".  In the reference's order:
 *   Clear (:579): cur's ids all become -1.
 *   Project, once per call: last-frame feature i with id = last's mp_id[i] < 0, or with last_outlier[i] set, is no query.  isBad() is not
 *     asked there, so a BAD slot is projected.  An id outside the table or naming a slot that is not LIVE returns CCM_E_ARG with cur's
 *     ids as they were on entry.  Otherwise, with P the slot's pos, in the arithmetic of a float cv::Mat:
 *       Pc[r] = (float)((double)R[r][0] P[0] + (double)R[r][1] P[1] + (double)R[r][2] P[2] + (double)t[r])
 *       invz = 1.0f / Pc[2];  reject invz < 0
 *       u = fx * PcX * invz + cx;  v = fy * PcY * invz + cy   (float, left to right, each operation rounded: the association of
 *       ccm_frame_search_local_points, one device function for both)
 *       reject u < min_x || u > max_x, then v < min_y || v > max_y   (both ends inside, unlike IsInImage)
 *     One deviation: a u or v that is not finite (Pc[2] == 0 only) is rejected; the reference would pass it to GetFeaturesInArea, where
 *     the cast is undefined.  A query takes the slot's descriptor, HAS_OBS of the slot, octave and angle from `last`; the current
 *     feature it is matched to receives the slot as its id.
 *   Search, per pass: radius = th * scale_factors[octave], levels octave-1 .. octave+1, window selection, the sequential acceptance of
 *     :1411-1448 and the rotation histogram of :1453-1473 exactly as ccm_frame_search_by_projection_frame runs them for a `last` handle
 *     (on the device, or on the host with CCM_WINDOW_HOST_ACCEPT=1 or a frame too large for the acceptance kernel's LDS).
 *   Retry (:587-591): with n_matches < retry_below the ids are cleared again and ONE more pass runs with 2 * th; the projection is
 *     kept, only radius and level window are made again.
 *   No pose (:593-594): with n_matches < min_matches after the last pass, or inv_level_sigma2 == NULL, posed = 0; the handle keeps the
 *     last pass's matches as ids (the reference does not clear them there), pose7 is untouched, outlier is 0 and n_inliers 0.
 *   Pose: as ccm_frame_pose_optimize_table on cur from pose7, bit for bit.
 *   Discard (:599-618): a feature with an id and outlier != 0 loses its id.  n_matches_map counts the features whose id names a slot
 *     with HAS_OBS afterwards (without a pose: of the last pass's matches).  mp_id and the handle agree after the call.
 * Traffic, as the code has it: one page-locked copy up of last_outlier (when given), 16 zero bytes, pose7, intr, inv_level_sigma2 and
 * scale_factors -- 320 bytes (five 64-byte segments) without last_outlier, plus N_last rounded up to 64 with it; nothing per map point.  One read-back
 * and stream synchronisation per search pass (status, match, occupancy flags, the bad-id word: 5 N_cur + 32 bytes and the padding),
 * which the overflow retry of the candidate lists needs, and one more for the rest (counts, pose7, outlier, mp_id; the taps when asked
 * for): 2 synchronisations for a call of one pass, 3 with the retry.  On the host acceptance route the candidate lists and what the
 * loops read of both frames are fetched as well, each fetch synchronising.
 * Errors, found before anything changes the handle.  CCM_E_ARG: a NULL ctx, cur, last, table, params, result, scale_factors, pose7 (with
 * a pose stage), intr (with a pose stage), match or mp_id or outlier (N_cur > 0); only some of u / v / valid; n_levels outside
 * 1..CCM_MAX_LEVELS; cur == last; a handle or table of another context; check_ori with a handle that has no angles; an octave of last
 * that is >= n_levels, or, with a pose stage, an octave of cur that is.  CCM_E_STATE: a handle or table that outlived its context.
 * N_last == 0 or N_cur == 0: CCM_OK with zero matches and posed = 0 (cur's ids cleared).  Returns CCM_OK or an error. */
typedef struct {
    float Tcw[12];                      /* CurrentFrame.mTcw = mVelocity * mLastFrame->mTcw, rows of [Rcw | tcw] */
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;   /* mnMinX .. mnMaxY */
    int32_t n_levels; const float* scale_factors;          /* mvScaleFactors [n_levels], 1..CCM_MAX_LEVELS */
    float th;                           /* 7 */
    int32_t retry_below;                /* 20: fewer matches -> ids cleared, searched again with 2 * th; 0 = never */
    int32_t min_matches;                /* 20, miTrackWithMotionModelInlierThresSearch: fewer after the last pass -> no pose */
    int32_t check_ori; int32_t orb_dist;/* 1, TH_HIGH = 100 */
    const uint8_t* last_outlier;        /* [N_last] LastFrame.mvbOutlier or NULL = none */
    /* pose stage; inv_level_sigma2 == NULL: search only */
    const float* inv_level_sigma2; const double* intr; /* [n_levels], [4] */
} ccm_tmm_params;
typedef struct {
    int32_t n_matches;     /* of the last pass, after the rotation filter: what SearchByProjection returned */
    int32_t passes;        /* 1 or 2 */
    int32_t posed;         /* 1 when the pose stage ran */
    int32_t n_inliers;     /* PoseOptimizationClient's return value */
    int32_t n_matches_map; /* :600-618: features that keep a point with HAS_OBS after the discard */
    double  pose7[7];      /* in: Converter::toSE3Quat(mTcw) (ccm_pose_from_mat4f); out: optimised when posed */
    int32_t* match;        /* [N_cur] last-frame feature assigned to current feature i by the last pass, or -1 */
    int32_t* mp_id;        /* [N_cur] the handle's ids after the call */
    uint8_t* outlier;      /* [N_cur] mvbOutlier as the pose left it, BEFORE the discard (the caller needs it for mbTrackInView / mLastFrameSeen); 0 when not posed */
    float* u; float* v; uint8_t* valid;   /* optional taps [N_last] (all three or none): the projection; u = v = 0 where valid is 0 */
} ccm_tmm_result;
int ccm_frame_track_motion_model(ccm_ctx*, ccm_frame* cur, const ccm_frame* last, ccm_map_table*, const ccm_tmm_params*, ccm_tmm_result*);

/* The relocalisation overload ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cpp:
 * 1478-1605) on the current frame's handle, a keyframe handle whose map-point ids are table slots, and the table; it replaces the
 * route through ccm_frame_search_by_projection_frame on host arrays, where the caller projects every map point of the keyframe and
 * uploads u, v, level, angle and a descriptor per point.  In the reference's order, one thread per keyframe feature (k_reloc_project):
 *   Keyframe feature i with id = kf's mp_id[i] < 0 is no query (:1498).  An id outside the table or naming a slot that is not LIVE
 *     returns CCM_E_ARG with cur's ids as they were on entry.  A BAD slot is skipped: isBad() IS asked here (:1500), unlike Current/Last.
 *     A slot in the found set is skipped (:1500).
 *   Project, with P the slot's pos, in the arithmetic ccm_frame_track_motion_model states (one device function for both):
 *       Pc[r] = (float)((double)R[r][0] P[0] + (double)R[r][1] P[1] + (double)R[r][2] P[2] + (double)t[r])
 *       invz = 1.0f / Pc[2]   (:1508 divides in double and narrows; for one division of two floats that is the same float)
 *       u = fx * PcX * invz + cx;  v = fy * PcY * invz + cy
 *     There is NO depth test in this overload: a point behind the camera whose u, v land inside the bounds is a query.  One deviation,
 *     as in ccm_frame_track_motion_model: a u or v that is not finite (Pc[2] == 0 only) is rejected.
 *       reject u < min_x || u > max_x, then v < min_y || v > max_y   (:1513-1516, both ends inside)
 *   Distance: dist3D = (float)sqrt of the squares of P - Ow summed in double (cv::norm); reject dist3D < 0.8f * min_dist || dist3D >
 *     1.2f * max_dist (:1526 with GetMin/MaxDistanceInvariance, strict on both sides).
 *   Level = PredictScale(dist3D, Frame) (src/MapPoint.cpp:854-869): ratio = max_dist / dist3D, (float)log((double)ratio) /
 *     log_scale_factor, ceilf, clamped to [0, n_levels - 1], a NaN gives 0 -- the device function of ccm_fuse_select_table_frames.
 *   Query: radius = th * scale_factors[level], levels level-1 .. level+1 (:1532-1534), the slot's descriptor, angle kf's angle[i].
 *   Search and acceptance: window selection, the sequential acceptance of :1544-1564 in i order and the rotation histogram of
 *     :1566-1601 exactly as ccm_frame_search_by_projection_frame runs them (on the device, or on the host with
 *     CCM_WINDOW_HOST_ACCEPT=1 or a frame too large for the acceptance kernel's LDS).  A current feature is occupied when its mp_id >=
 *     0, WHATEVER the slot's HAS_OBS says (:1547), and a feature matched in this call is occupied for the later queries; accepted is
 *     bestDist <= orb_dist.  cur's ids are NOT cleared first; the accepted features receive the slot, a feature the rotation filter
 *     removes keeps -1.  n_matches is the count after the rotation filter.
 * The found set (sAlreadyFound): n_found >= 0: the slots found[0 .. n_found); n_found < 0: every id cur holds on entry, derived on
 * the device from cur's mp_id.  Membership is a stamp per table slot in a column of the table handle; nothing is cleared per call.
 * Traffic, as the code has it: the view, th and the scale factors travel as kernel arguments; one page-locked copy up of the found
 * list when it is explicit (4 bytes per entry), nothing per map point.  One read-back and stream synchronisation (status, match,
 * occupancy flags, mp_id, the bad-id word: 9 N_cur + 32 bytes and the padding; the taps with it when asked for), repeated only by the
 * overflow retry of the candidate lists.  On the host acceptance route the candidate lists and what the loops read of both frames
 * are fetched as well, each fetch synchronising.
 * Errors, found before anything changes the handle.  CCM_E_ARG: a NULL ctx, cur, kf, table, view, result, scale_factors, match or
 * mp_id (N_cur > 0), found (n_found > 0); only some of the taps; n_levels outside 1..CCM_MAX_LEVELS; cur == kf; a handle or table of
 * another context; check_ori with a handle that has no angles; a found slot outside the table.  CCM_E_STATE: a handle or table that
 * outlived its context.  N_kf == 0 or N_cur == 0: CCM_OK with zero matches.  Returns CCM_OK or an error. */
typedef struct {
    float Tcw[12];                      /* CurrentFrame.mTcw, rows of [Rcw | tcw] */
    float Ow[3];                        /* -Rcw^T tcw (:1484) */
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;   /* mnMinX .. mnMaxY */
    int32_t n_levels; const float* scale_factors;          /* mvScaleFactors [n_levels], 1..CCM_MAX_LEVELS */
    float log_scale_factor;             /* mfLogScaleFactor */
} ccm_reloc_view;
typedef struct {
    int32_t n_matches;     /* after the rotation filter: what SearchByProjection returned */
    int32_t* match;        /* [N_cur] keyframe feature assigned to current feature i by this call, or -1 */
    int32_t* mp_id;        /* [N_cur] the handle's ids after the call */
    float* u; float* v; int32_t* level; uint8_t* valid;   /* optional taps [N_kf] (all four or none); u = v = 0, level = 0 where valid is 0 */
} ccm_reloc_search_result;
int ccm_frame_search_by_projection_keyframe(ccm_ctx*, ccm_frame* cur, const ccm_frame* kf, ccm_map_table*, const ccm_reloc_view*, float th,
                                            int orb_dist, int check_ori, int n_found, const int32_t* found, ccm_reloc_search_result*);

/* One relocalisation candidate from the PnP pose to the verdict, in one call: the body of the candidate loop of ORB-SLAM's
 * Tracking::Relocalization behind PnPsolver::iterate.  The reference has no such function -- its Tracking stays LOST
 * (src/Tracking.cpp:187-201) -- so the steps are defined here, with ORB-SLAM's nesting and its thresholds as the defaults in brackets:
 *   1. Matches: cur's ids all become -1, then feature[j] receives slot[j] for each of the n_matched PnP inliers (vbInliers of
 *      ccm_pnp_solver_iterate over the candidate's vpMapPointMatches).  found = those slots.  pose7 = ccm_pose_from_mat4f(Tcw).
 *   2. First pose: n_good = the pose optimisation, exactly ccm_frame_pose_optimize_table from pose7.  n_good < min_good [10]: success =
 *      0 and the call stops (the ids stay the inliers).  Otherwise the features with outlier != 0 lose their id; found keeps them.
 *   3. First search, only if n_good < enough [50]: n_add1 = ccm_frame_search_by_projection_keyframe with found, th1 [10] and dist1
 *      [100]; its Tcw / Ow are those of pose7 (the definition of ccm_pose_to_camera, evaluated on the device: the pose is not read
 *      back for it), the rest of the view is `view`.
 *   4. Second pose, only if 3 ran and n_good + n_add1 >= enough: n_good = the pose again from the current pose7.  The outliers keep
 *      their ids.
 *   5. Second search, only if 4 ran and narrow_above [30] < n_good < enough: found = every id cur holds now; n_add2 = the search with
 *      th2 [3] and dist2 [64] at the new pose7.
 *   6. Third pose, only if 5 ran and n_good + n_add2 >= enough: n_good = the pose once more; the outliers lose their id.
 *   7. success = n_good >= enough.  On success the handle's pose is set as ccm_frame_set_pose(cur, ccm_pose_to_camera(pose7)) would.
 * stages has one bit per stage that ran (CCM_RELOC_*); n_add of a search that did not run is 0; outlier is that of the last pose that
 * ran; mp_id and the handle agree after the call.
 * Traffic: one page-locked copy up (pose7, intr, inv_level_sigma2, and 8 bytes per inlier); nothing per map point.  Every stage
 * decides the next, so each ends in ONE read-back and stream synchronisation and nothing is queued between them that is waited for:
 * a pose stage brings n_inliers, the bad-id word, outlier and pose7 (N_cur + 184 bytes and the padding), a search stage what
 * ccm_frame_search_by_projection_keyframe reads back.  "The outliers lose their id" is decided on the device from n_inliers, behind
 * the pose and in front of its read-back.  Synchronisations per path: stop at 2, or success at once: 1; search 1 failing the sum: 2;
 * searches 1 and pose 2 with n_good outside (narrow_above, enough): 3; search 2 failing the sum: 4; all stages: 5.  On the host
 * acceptance route each search fetches the candidate lists and what its loops read as well.
 * Errors leave cur's ids as they were on entry (they are kept aside and put back).  CCM_E_ARG: a NULL ctx, cur, kf, table, params,
 * result, Tcw, intr, inv_level_sigma2, scale_factors, feature or slot (n_matched > 0), mp_id or outlier (N_cur > 0); n_matched < 0;
 * n_levels outside 1..CCM_MAX_LEVELS; cur == kf; a handle or table of another context; check_ori with a handle that has no angles;
 * a feature outside [0, N_cur) or named twice; a slot outside the table or not LIVE; an octave of cur that is >= n_levels; an id of
 * kf outside the table or not LIVE (found by the first search).  CCM_E_STATE: a handle or table that outlived its context. */
enum { CCM_RELOC_POSE1 = 1, CCM_RELOC_SEARCH1 = 2, CCM_RELOC_POSE2 = 4, CCM_RELOC_SEARCH2 = 8, CCM_RELOC_POSE3 = 16 };
typedef struct {
    const float* Tcw;                   /* [16] the 4x4 float of ccm_pnp_solver_iterate */
    int32_t n_matched;                  /* PnP inliers */
    const int32_t* feature;             /* [n_matched] feature of cur, each once */
    const int32_t* slot;                /* [n_matched] its map point's table slot */
    const double* intr;                 /* [4] fx, fy, cx, cy of the pose optimisation */
    const float* inv_level_sigma2;      /* [view.n_levels] */
    ccm_reloc_view view;                /* of the searches; its Tcw and Ow are not read */
    int32_t min_good, enough, narrow_above;             /* 10, 50, 30 */
    float th1; int32_t dist1;           /* 10, 100 */
    float th2; int32_t dist2;           /* 3, 64 */
    int32_t check_ori;                  /* 1 */
} ccm_reloc_params;
typedef struct {
    int32_t success;       /* 7. */
    int32_t n_good;        /* nGood of the last pose that ran */
    int32_t stages;        /* CCM_RELOC_* bits of the stages that ran */
    int32_t n_add1, n_add2;/* what the two searches returned */
    double  pose7[7];      /* ccm_pose_from_mat4f(Tcw), optimised by every pose stage */
    int32_t* mp_id;        /* [N_cur] the handle's ids after the call */
    uint8_t* outlier;      /* [N_cur] mvbOutlier of the last pose that ran */
} ccm_reloc_result;
int ccm_frame_relocalize_candidate(ccm_ctx*, ccm_frame* cur, const ccm_frame* kf, ccm_map_table*, const ccm_reloc_params*, ccm_reloc_result*);

/* ORBmatcher::Fuse, both overloads (src/ORBmatcher.cpp:854-1000 and :1002-1122), up to and including the selection, on keyframe
 * handles and the table: ONE list of map points is projected into EVERY keyframe, as LoopFinder::SearchAndFuse (src/LoopFinder.cpp:
 * 806-831), MapMerger::SearchAndFuse (src/MapMerger.cpp:574-600) and the first loop of LocalMapping::SearchInNeighbors
 * (src/Mapping.cpp:499-521) do.  The two overloads share their arithmetic; they differ in where the pose comes from, in the chi2 test
 * (chi2_check, :929-937) and in the acceptance threshold, which the caller passes as for ccm_fuse_select_batch.  What the reference
 * does with a selection (Replace / AddObservation / vpReplacePoint, :958-990, :1103-1117) stays with the caller.
 *   Pair (k, j) = point slot[j] in keyframe views[k]; the outputs are [n_kf][n_points], pair (k, j) at k * n_points + j.  Gates in the
 *   reference's order, the first that fails names the pair (gate, CCM_FG_*), with P / Pn / min_dist / max_dist the slot's row:
 *     SKIPPED      skip[j] != 0 (a null pointer, mbDoNotReplace :880), or the slot is not LIVE, or it is BAD (isBad(), :877 / :1023)
 *     IN_KEYFRAME  some feature of the handle holds the slot in mp_id (IsInKeyFrame :877, spAlreadyFound :1011 / :1023); an mp_id
 *                  outside [0, capacity) names no slot and is ignored
 *     BEHIND       Pc[r] = (float)((double)R[r][0] P[0] + (double)R[r][1] P[1] + (double)R[r][2] P[2] + (double)t[r]);  Pc[2] < 0
 *     OUTSIDE      invz = 1.0f / Pc[2];  x = Pc[0] * invz;  y = Pc[1] * invz;  u = fx * x + cx;  v = fy * y + cy  (float, each
 *                  operation rounded, not fused -- NOT the association of ccm_frame_search_local_points, which follows
 *                  Frame::isInFrustum);  !(u >= min_x && u < max_x && v >= min_y && v < max_y), KeyFrame::IsInImage
 *                  (src/KeyFrame.cpp:1236): u == max_x is outside, and so is a NaN (Pc = 0).  The second overload writes 1.0 / Pc[2]
 *                  in double and stores a float (:1040): the same value, a quotient of two floats rounds alike both ways.
 *     DISTANCE     PO = P - Ow (float);  dist = (float)sqrt(sum (double)PO^2);  dist < 0.8f * min_dist || dist > 1.2f * max_dist
 *     ANGLE        sum (double)PO[i] * (double)Pn[i] < 0.5 * (double)dist, compared in double (:914, :1063)
 *     EMPTY_KF     the pair passed all of the above and the handle has no features (GetFeaturesInArea would return nothing)
 *     SEARCHED     level = ceil(((float)log((double)(max_dist / dist))) / log_scale_factor) clamped to [0, n_levels - 1], a NaN gives 0
 *                  (MapPoint::PredictScale, src/MapPoint.cpp:837-852, exactly as ccm_frame_search_local_points computes it);
 *                  radius = th * scale_factors[level], features of level - 1 .. level inside the window, with chi2_check those
 *                  whose reprojection error e2 * inv_level_sigma2[octave] is at most 5.99; the nearest descriptor, the first of equal
 *                  ones in GetFeaturesInArea's order.  best_dist = its distance (256: none), best_idx = its index when
 *                  best_dist <= accept_th, else -1 -- per pair what ccm_fuse_select_batch_frames returns for valid = 1, these u / v /
 *                  level and the slot's descriptor.
 *   Every pair that is not SEARCHED has best_idx = -1 and best_dist = 256.  The taps u / v / level (all three or none) hold the values
 *   above where the pair got that far, and 0 before.
 * Traffic: one page-locked staging copy up (the views with the handles' device pointers, the slot list, skip, inv_level_sigma2) --
 * nothing per pair, nothing of a keyframe or a map point; the projection appends the SEARCHED pairs to a query list in device memory
 * and only those run the selection.  One download of the outputs that were asked for.  The call synchronises twice: on the number of
 * queries (16 bytes) behind the projection, and on the download.  It is ordered on the context's stream behind
 * ccm_frame_set_map_points, ccm_map_table_update and ccm_map_table_refresh calls made before it.
 * Errors are found on the host before anything is queued; the outputs are then untouched.  CCM_E_ARG: a NULL required array (views,
 * slot, scale_factors, best_idx, inv_level_sigma2 with chi2_check, a view's kf), only some of u / v / level, n_levels outside
 * 1..CCM_MAX_LEVELS, a slot outside [0, capacity) or listed twice, a handle or table of another context.  CCM_E_STATE: a handle or table
 * that outlived its context.  CCM_E_CAPACITY: more than 65535 keyframes or 2^24 pairs in one call.  Memory: the
 * query list is sized for every pair surviving, 69 bytes of device memory per pair plus 4 to 21 bytes per pair (by the outputs asked
 * for) of page-locked host and device staging, kept by the context at its high-water mark -- about 11 MB + 1.4 MB at 160,000 pairs,
 * 1.1 GB + 0.35 GB at the cap; split a larger problem over the keyframes.  n_kf == 0 or n_points == 0
 * returns CCM_OK with n_searched = 0. */
enum { CCM_FG_SEARCHED = 0, CCM_FG_SKIPPED = 1, CCM_FG_IN_KEYFRAME = 2, CCM_FG_BEHIND = 3, CCM_FG_OUTSIDE = 4, CCM_FG_DISTANCE = 5,
       CCM_FG_ANGLE = 6, CCM_FG_EMPTY_KF = 7 };
typedef struct {
    ccm_frame* kf;                     /* features, grid and mp_id (as table slots) are read; no bow / camera / pose needed */
    float Tcw[12];                     /* rows of [Rcw | tcw]: GetRotation / GetTranslation (:856-857), or the caller's decomposition of Scw (:1004-1007) */
    float Ow[3];                       /* GetCameraCenter (:864), or -Rcw^T tcw as the caller computed it (:1008) */
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;  /* mnMinX .. mnMaxY (KeyFrame::IsInImage, src/KeyFrame.cpp:1236) */
} ccm_fuse_view;
typedef struct {
    int32_t n_kf;  const ccm_fuse_view* views;       /* the same handle may appear twice, with different poses */
    int32_t n_points;  const int32_t* slot;          /* [n_points] table slots; ONE list, projected into every keyframe */
    const uint8_t* skip;                             /* [n_points] or NULL: 1 = never looked at (null pointer, mbDoNotReplace) */
    float log_scale_factor;  int32_t n_levels;       /* mfLogScaleFactor, mnScaleLevels (1..CCM_MAX_LEVELS) */
    const float* scale_factors;                      /* [n_levels] */
    const float* inv_level_sigma2;                   /* [n_levels], needed with chi2_check */
    float th;  int32_t chi2_check;  int32_t accept_th;   /* as ccm_fuse_select_batch */
} ccm_fuse_table_problem;
typedef struct {
    int32_t* best_idx;                 /* [n_kf][n_points] feature of keyframe k selected for point j, or -1 */
    int32_t* best_dist;                /* optional, same shape; 256 where best_idx is -1 for want of a candidate */
    uint8_t* gate;                     /* optional tap, same shape: CCM_FG_* */
    float* u; float* v; int32_t* level;/* optional taps, same shape; meaningful where gate == CCM_FG_SEARCHED */
    int32_t n_searched;                /* out: pairs that passed every gate */
} ccm_fuse_table_result;
int ccm_fuse_select_table_frames(ccm_ctx*, ccm_map_table*, const ccm_fuse_table_problem*, ccm_fuse_table_result*);

/* ---- ComputeSim3 on keyframe handles and the table: links 3 and 5 of LoopFinder::ComputeSim3 (src/LoopFinder.cpp:231-400) and
 * MapMatcher::ComputeSim3 (src/MapMatcher.cpp:238-400), next to ccm_search_by_bow_frames, ccm_sim3_solver_*, ccm_optimize_sim3 and
 * ccm_fuse_select_table_frames.  Both calls read the map points from the table and the features, grids and mp_id (as table slots) from
 * the handles; nothing of a keyframe or of a map point is uploaded.  The table and every handle of a call belong to the calling context
 * (one table serves one context, as for ccm_fuse_select_table_frames): a thread with another context keeps the array entry points
 * ccm_search_by_sim3 and ccm_search_by_projection_sim3_batch.  Float arithmetic is unfused and rounded per operation; a "matrix
 * product" below sums in double and stores a float, Pc[r] = (float)((double)M[r][0] P[0] + (double)M[r][1] P[1] + (double)M[r][2] P[2] +
 * (double)M[r][3]) for a row-major [3][4] M, as for CCM_FG_BEHIND above.
 *
 * ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:1124-1348), complete, for n_pairs >= 0 candidate pairs in one call (the reference calls
 * it once per candidate that survives RANSAC; the round-robin over candidates can hand over all of them).
 *   Direction 1 -> 2, per feature i1 of kf1 with slot = kf1's mp_id[i1]; the first gate that fails names the feature (CCM_SG_*):
 *     NO_POINT   slot < 0, slot >= capacity, or the slot is not LIVE (such an id names no point, as for Fuse)
 *     MATCHED    matched12[i1] >= 0 (vbAlreadyMatched1, :1154-1164)
 *     BAD        the slot is BAD (isBad(), :1177)
 *     BEHIND     Pc1 = T1w P, Pc2 = S21 Pc1 (two matrix products, :1181-1182);  Pc2[2] < 0
 *     OUTSIDE    invz = 1.0f / Pc2[2];  x = Pc2[0] * invz;  y = Pc2[1] * invz;  u = fx * x + cx;  v = fy * y + cy;  KeyFrame::IsInImage with
 *                the bounds of the TARGET keyframe (bounds2 here): !(u >= min_x && u < max_x && v >= min_y && v < max_y); a NaN is outside
 *     DISTANCE   dist3D = (float)sqrt(sum (double)Pc2^2);  dist3D < 0.8f * min_dist || dist3D > 1.2f * max_dist  (:1199-1205)
 *     EMPTY_KF   the target handle has no features
 *     SEARCHED   level = MapPoint::PredictScale on the target side's log_scale_factor / n_levels, the expression of CCM_FG_SEARCHED;
 *                radius = th * scale_factors_target[level], features of level - 1 .. level in the window, the nearest descriptor, the
 *                first of equal ones in GetFeaturesInArea's order, accepted at <= TH_HIGH (100): sel1[i1] = that feature of kf2 or -1
 *   SearchBySim3 has no viewing-angle gate.  Direction 2 -> 1 is the same with T2w, S12, bounds1, side 1's levels, and MATCHED where
 *   some i1 has matched12[i1] >= 0 and matched_idx2[i1] in [0, N2) naming the feature (vbAlreadyMatched2, :1160-1162; an index
 *   outside [0, N2) is ignored).  fx, fy, cx, cy are ONE set used for BOTH directions: the reference reads pKF1's intrinsics for both
 *   (:1127-1130, :1272), also where pKF2 has other ones -- pass pKF1's.
 *   match12[i1] = sel1[i1] where sel2[sel1[i1]] == i1, else -1 (:1330-1345), decided on the device; n_found[p] counts them and the
 *   function returns their sum.  All per-feature arrays of the result are flat over the pairs: pair p's side-1 entries start at
 *   N1(0) + .. + N1(p-1), its side-2 entries at N2(0) + .. + N2(p-1).  The taps hold 0 (sel: -1) where a feature did not get that far.
 * Traffic: one page-locked staging copy up (per pair and direction a 168-byte view with the handles' device pointers, an 80-byte grid
 * record, and the two index lists, 8 bytes per feature of kf1); one download of match12 and of the taps asked for.  Two
 * synchronisations: on the number of queries (16 bytes) behind the projection, and on the download.  Ordered on the context's stream
 * behind earlier ccm_frame_set_map_points / ccm_map_table_update / ccm_map_table_refresh.
 * Errors are found on the host before anything is queued; the outputs are then untouched.  CCM_E_ARG: a NULL required array (pairs,
 * a pair's kf1 / kf2, matched12 / matched_idx2 of a pair with N1 > 0, scale_factors1 / 2, match12 with features on side 1, n_found),
 * only some of u / v / level of a direction, n_levels1 / 2 outside 1..CCM_MAX_LEVELS, a handle or table of another context.
 * CCM_E_STATE: a handle or table that outlived its context.  CCM_E_CAPACITY: more than 32767 pairs or 2^24 features in one call.
 * n_pairs == 0 returns 0.  Memory: the query list is sized for every feature surviving, 72 bytes of device memory per feature of
 * either side, plus 12 to 29 bytes per feature (by the taps asked for) of page-locked host and device staging, kept by the context
 * at its high-water mark: about 0.5 MB for three pairs of 1,000 x 1,000 features. */
enum { CCM_SG_SEARCHED = 0, CCM_SG_NO_POINT = 1, CCM_SG_MATCHED = 2, CCM_SG_BAD = 3, CCM_SG_BEHIND = 4, CCM_SG_OUTSIDE = 5,
       CCM_SG_DISTANCE = 6, CCM_SG_EMPTY_KF = 7 };
typedef struct {
    ccm_frame* kf1; ccm_frame* kf2;    /* features, grid and mp_id (vpMapPoints1 / 2 as table slots) are read; may be the same handle */
    float T1w[12], T2w[12];            /* rows of [R1w | t1w], [R2w | t2w] (:1133-1138) */
    float S21[12], S12[12];            /* rows of [sR21 | t21] and [sR12 | t12], as the caller computed them at :1141-1143 */
    float fx, fy, cx, cy;              /* pKF1's, used for both directions */
    float bounds1[4], bounds2[4];      /* mnMinX, mnMaxX, mnMinY, mnMaxY of kf1 / kf2 */
    const int32_t* matched12;          /* [N1] slot of vpMatches12[i] on entry, or -1 */
    const int32_t* matched_idx2;       /* [N1] GetIndexInKeyFrame(pKF2) of that point, or -1 */
} ccm_sim3_search_pair;
typedef struct {
    int32_t n_pairs;  const ccm_sim3_search_pair* pairs;
    float th;                                                    /* 7.5 in ComputeSim3 */
    float log_scale_factor1;  int32_t n_levels1;  const float* scale_factors1;   /* side 1: kf1 of every pair; [n_levels1] */
    float log_scale_factor2;  int32_t n_levels2;  const float* scale_factors2;   /* side 2 */
} ccm_sim3_search_problem;
typedef struct {
    int32_t* match12;                  /* [sum N1] feature of kf2 matched to feature i1, or -1 */
    int32_t* n_found;                  /* [n_pairs] */
    uint8_t* gate1; float* u1; float* v1; int32_t* level1; int32_t* sel1;   /* optional taps [sum N1]: CCM_SG_*, projection, vnMatch1 */
    uint8_t* gate2; float* u2; float* v2; int32_t* level2; int32_t* sel2;   /* optional taps [sum N2]: direction 2 -> 1, vnMatch2 */
} ccm_sim3_search_result;
int ccm_search_by_sim3_table_frames(ccm_ctx*, ccm_map_table*, const ccm_sim3_search_problem*, ccm_sim3_search_result*);

/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cpp:308-446) up to and including the acceptance:
 * ONE list of table slots projected into n_kf views, each with its own vpMatched (the reference has one view, mpCurrentKF; the batch
 * mirrors ccm_search_by_projection_sim3_batch).  A view is a ccm_fuse_view -- the caller decomposes Scw as at :317-321 -- plus
 * matched_slot [N]: vpMatched on entry, the slot of the point or -1 (any value >= 0 marks the feature as matched; one outside
 * [0, capacity) names no listed point).  Pair (k, j) at k * n_points + j.  Gates in the reference's order (CCM_LG_*):
 *     SKIPPED        the slot is not LIVE, or it is BAD (isBad(), :335)
 *     ALREADY_FOUND  the slot occurs in view k's matched_slot (spAlreadyFound, :324-335)
 *     BEHIND / OUTSIDE / DISTANCE / ANGLE / EMPTY_KF / SEARCHED   exactly the arithmetic of CCM_FG_* above (:342-375 and Fuse's second
 *                    overload are the same text); there is NO IN_KEYFRAME gate
 *   Acceptance, in list order (:388-441): a SEARCHED point takes the nearest feature of level - 1 .. level in its window whose
 *   vpMatched is still empty (:393), strictly nearer wins, so the first of equal ones; accepted at <= TH_LOW (50): best_idx = that
 *   feature.  An accepted point that the keyframe already observes -- observed[k][j]: some feature of the handle holds the slot in
 *   mp_id -- leaves vpMatched alone and is not counted (:414-435; RemapMapPointMatch stays with the caller, who reads observed to tell
 *   which accepted points are remaps); any other accepted point sets matched_slot[best_idx] = its slot and counts in n_matches[k].
 *   `observed` restates GetIndexInKeyFrame(pKF) != -1 (:415) from the handle's mp_id: it rests on mObservations and mvpMapPoints agreeing,
 *   as AddObservation / AddMapPoint keep them.  The function returns the sum of n_matches.
 * The queries stay in list order, one per pair (a gated pair has radius -1); keyframe k is worked by workgroup k of the acceptance
 * kernel of ccm_search_by_projection_sim3_batch.  A handle with more features than that kernel's LDS admits (about 25,000) sends the
 * call through the host acceptance loops, as ccm_frame_search_by_projection does in that case (so does CCM_WINDOW_HOST_ACCEPT=1).
 * Traffic: one staging copy up (per view 112 + 80 + 16 bytes and 4 bytes per feature for matched_slot, the slot list); one download;
 * ONE synchronisation (a second round only when a window holds more than 64 features).  Stream order, error handling and ownership as
 * ccm_fuse_select_table_frames.  CCM_E_ARG: a NULL required array (views, a view's kf, matched_slot of a view with features, slot,
 * scale_factors, best_idx, observed, n_matches, the result's matched_slot), only some of u / v / level, n_levels outside
 * 1..CCM_MAX_LEVELS, a slot outside [0, capacity) or listed twice, a handle or table of another context.  CCM_E_STATE: a handle or table
 * that outlived its context.  CCM_E_CAPACITY: more than 65535 views or 2^24 pairs.  n_kf == 0 or n_points == 0 returns 0 with
 * best_idx = -1, n_matches = 0 and matched_slot copied through.  Memory: 574 bytes of device memory per pair (the candidate lists of 64
 * entries take 512 of them) and 5 per feature, plus 5 to 22 bytes per pair (by the taps asked for) and 8 per feature of page-locked
 * host and device staging, kept by the context at its high-water mark: 2.3 MB + 0.03 MB for 1,000 features x 4,000 points. */
enum { CCM_LG_SEARCHED = 0, CCM_LG_SKIPPED = 1, CCM_LG_ALREADY_FOUND = 2, CCM_LG_BEHIND = 3, CCM_LG_OUTSIDE = 4, CCM_LG_DISTANCE = 5,
       CCM_LG_ANGLE = 6, CCM_LG_EMPTY_KF = 7 };
typedef struct {
    ccm_fuse_view view;                /* handle, [Rcw | tcw], Ow, intrinsics and bounds, as for ccm_fuse_select_table_frames */
    const int32_t* matched_slot;       /* [N] vpMatched on entry */
} ccm_loop_view;
typedef struct {
    int32_t n_kf;  const ccm_loop_view* views;       /* the same handle may appear twice, with different poses */
    int32_t n_points;  const int32_t* slot;          /* [n_points] table slots, visited in this order */
    float log_scale_factor;  int32_t n_levels;       /* mfLogScaleFactor, mnScaleLevels (1..CCM_MAX_LEVELS) */
    const float* scale_factors;                      /* [n_levels] */
    float th;                                        /* 10 in ComputeSim3 */
} ccm_loop_projection_problem;
typedef struct {
    int32_t* best_idx;                 /* [n_kf][n_points] accepted feature of view k for point j, or -1 */
    uint8_t* observed;                 /* [n_kf][n_points] the handle already holds the slot */
    int32_t* matched_slot;             /* views' vpMatched after the call, flat: view k's [N_k] at N_0 + .. + N_(k-1) */
    int32_t* n_matches;                /* [n_kf] */
    uint8_t* gate; float* u; float* v; int32_t* level;   /* optional taps [n_kf][n_points]: CCM_LG_* and the projection */
    int32_t* best_dist;                /* optional tap: descriptor distance to best_idx, 256 where best_idx is -1 */
} ccm_loop_projection_result;
int ccm_search_by_projection_table_frames(ccm_ctx*, ccm_map_table*, const ccm_loop_projection_problem*, ccm_loop_projection_result*);

/* Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cpp:867-1062), next row F4,
 * batched over candidate keyframe pairs: one VertexSim3Expmap, fixed points, EdgeSim3ProjectXYZ +
 * EdgeInverseSim3ProjectXYZ per correspondence with g2o's numeric Jacobians (delta 1e-9) and Huber(sqrt(th2));
 * optimize(5), prune chi2 > th2, optimize(5 or 10), classify.  Correspondence e of problem p (first[p] <= e <
 * first[p+1]) = one non-null vpMatches1[i] that passed :918-943: P1 = R1w*P3D1w + t1w, P2 = R2w*P3D2w + t2w (the
 * caller's float arithmetic, widened), obs1/info1 = pKF1->mvKeysUn[i] / mvInvLevelSigma2, obs2/info2 likewise for
 * i2.  sim3 = g2oS12 as qx,qy,qz,qw, tx,ty,tz, s (in/out; untouched when fewer than 10 correspondences survive the
 * first round, where the reference returns 0); inlier[e] = vpMatches1 entry kept; n_inliers[p] = the return value. */
typedef struct {
    int32_t        n_problems;
    double*        sim3;       /* [n_problems][8] in/out */
    const int32_t* fix_scale;  /* [n_problems] */
    const double*  K1;         /* [n_problems][4] fx, fy, cx, cy of pKF1 */
    const double*  K2;
    const int32_t* first;      /* [n_problems+1] */
    const double*  P1;         /* [..][3] */
    const double*  P2;
    const double*  obs1;       /* [..][2] */
    const double*  obs2;
    const double*  info1;      /* [..] */
    const double*  info2;
    const float*   th2;        /* [n_problems] */
    uint8_t*       inlier;     /* [..] out */
    int32_t*       n_inliers;  /* [n_problems] out */
} ccm_sim3_problem;
int ccm_optimize_sim3(ccm_ctx*, ccm_sim3_problem*);

/* ---------------------------------------------------------------- Sim3Solver (src/Sim3Solver.cpp), batched RANSAC
 * The link in front of OptimizeSim3 in loop closing and map matching (src/LoopFinder.cpp:231-346, src/MapMatcher.cpp:238-350): one
 * Sim3Solver per candidate keyframe, iterate(5) round-robin over the candidates.  The hypotheses of Sim3Solver::iterate (:120-191)
 * do not depend on each other (three sampled correspondences -> ComputeSim3 :210-321 -> CheckInliers :324-348); only "running
 * best, return at the first hypothesis that qualifies" is ordered.  ccm_sim3_solver_create evaluates ALL hypotheses of ALL solvers
 * of a batch in one launch; ccm_sim3_solver_iterate / _find replay the ordered bookkeeping over the stored results on the host, so
 * any calling pattern returns what the sequential code returns for the same random draws.
 *
 * Constructor data (:5-92), flattened by the caller as for ccm_sim3_problem: correspondence e of solver k (first[k] <= e <
 * first[k+1], N = first[k+1] - first[k]) = one vpMatched12[i1] that passed :32-59, in i1 order.  The library computes mvP1im1 /
 * mvP2im2 (FromCameraToImage, :389-407).
 *
 * SetRansacParameters (:94-118) is part of the create call, because the hypotheses are evaluated there: solver k evaluates
 * mRansacMaxIts = ccm_sim3_ransac_iterations(N, probability, min_inliers, max_iterations) hypotheses, or none when N < min_inliers
 * (iterate leaves at :129) or N < 3 (the reference would sample out of range; unreachable behind MatchesThres 20).
 *
 * Sampling (:146-161): the random source stays with the caller (DUtils::Random is not part of this library).  draws holds the raw
 * RandomInt results: draw i of hypothesis h of solver k at draws[(k * max_iterations + h) * 3 + i], in [0, N-1-i].  The library
 * turns them into correspondence indices by the reference's swap-with-last removal on vAvailableIndices = 0..N-1 (position randi
 * takes the last element, :159).  Only the rows of hypotheses that are evaluated are read; one of them outside its range is
 * CCM_E_ARG.
 *
 * ComputeSim3: float storage as in the reference, the 4x4 symmetric eigenproblem by cyclic Jacobi in double.  The rotation is
 * built from the unit quaternion directly (equal to the reference's Rodrigues(2 atan2(|v|, w) v/|v|) for either sign of the
 * eigenvector, and defined at zero rotation); cv::eigen lies outside the reference tree, so the contract is a tolerance against a
 * float64 restatement, not bits.  CheckInliers: err1 = |p1im1 - proj(K1, T12 X2)|^2, err2 = |proj(K2, T21 X1)
 * - p2im2|^2, inlier iff err1 < max_err1 && err2 < max_err2; non-finite errors compare false. */
typedef struct {
    int32_t        n_solvers;
    const int32_t* first;        /* [n_solvers+1], first[0] = 0, non-decreasing */
    const int32_t* n1;           /* [n_solvers] mN1 = vpMatched12.size() */
    const int32_t* fix_scale;    /* [n_solvers] mbFixScale */
    const float*   K1;           /* [n_solvers][4] fx, fy, cx, cy of mK1 */
    const float*   K2;
    const float*   X1;           /* [..][3] mvX3Dc1 = Rcw1 * X3D1w + tcw1 (camera frame of pKF1) */
    const float*   X2;           /* [..][3] mvX3Dc2 */
    const float*   max_err1;     /* [..] mvnMaxError1 = 9.210 * mvLevelSigma2[octave] (:67) */
    const float*   max_err2;
    const int32_t* indices1;     /* [..] mvnIndices1, each in [0, n1[k]) */
    double         probability;  /* SetRansacParameters(probability, minInliers, maxIterations) */
    int32_t        min_inliers;
    int32_t        max_iterations;
    const int32_t* draws;        /* [n_solvers][max_iterations][3] */
    /* mnBestInliers at the start, [n_solvers], or NULL for 0 (the constructor's value).  SetRansacParameters resets mnIterations
     * (:117) but not mnBestInliers: a caller that changes the parameters of a solver it has already iterated creates the new batch
     * with the old solver's best count here and keeps its estimate until a hypothesis reaches that count. */
    const int32_t* best_inliers;
} ccm_sim3_ransac_problem;
typedef struct ccm_sim3_solver ccm_sim3_solver;

/* mRansacMaxIts of SetRansacParameters (:94-118): epsilon = (float)min_inliers / n; nIterations = 1 if min_inliers == n, else
 * ceil(log(1 - probability) / log(1 - pow(epsilon, 3))); max(1, min(nIterations, max_iterations)).  For n < min_inliers (and n ==
 * 0) the reference converts the logarithm of a non-positive number to int, which is undefined; the value is never used (iterate
 * leaves at :129) and is defined as 1 here.  Host only. */
int ccm_sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations);
/* Uploads the batch, evaluates every hypothesis in one launch, downloads the per-hypothesis counts, estimates and inlier masks and
 * synchronises once.  Device memory is the context's (grow-only, reused by the next batch); the solver object holds host memory
 * only.  It belongs to the thread that made it.  On an error *out is untouched. */
int ccm_sim3_solver_create(ccm_ctx*, const ccm_sim3_ransac_problem*, ccm_sim3_solver** out);
/* NULL is a no-op. */
void ccm_sim3_solver_destroy(ccm_sim3_solver*);
/* n_solvers of the batch, or CCM_E_ARG for NULL. */
int ccm_sim3_solver_count(const ccm_sim3_solver*);
/* Sim3Solver::iterate(nIterations, bNoMore, vbInliers, nInliers) (:120-191) of solver k, exactly: N < min_inliers -> *no_more = 1
 * and nothing else; the running best is replaced on mnInliersi >= mnBestInliers; a Sim3 comes back only for mnInliersi >
 * min_inliers (strict); mnIterations and mnBestInliers persist over calls, the per-call counter restarts; *no_more is set only when
 * the loop ends without a return at mnIterations >= mRansacMaxIts.  *found = 1: T12 holds mBestT12 (4x4 row-major), *n_inliers
 * the count and inliers[mvnIndices1[i]] = 1 for every inlier i; otherwise T12 is untouched.  inliers has n1[k] entries and is
 * always cleared first (:123).  inliers and T12 may be NULL. */
int ccm_sim3_solver_iterate(ccm_sim3_solver*, int k, int n_iterations, int32_t* found, int32_t* no_more, uint8_t* inliers,
                            int32_t* n_inliers, float* T12);
/* Sim3Solver::find (:193-197) = iterate(mRansacMaxIts) without bNoMore. */
int ccm_sim3_solver_find(ccm_sim3_solver*, int k, int32_t* found, uint8_t* inliers, int32_t* n_inliers, float* T12);
/* GetEstimatedRotation / Translation / Scale (:351-364): the running best, which hypotheses that did not qualify for a return
 * update as well.  R row-major 3x3.  CCM_E_STATE while no hypothesis has become the best (the reference returns empty matrices). */
int ccm_sim3_solver_estimate(const ccm_sim3_solver*, int k, float* R, float* t, float* s);
/* The RANSAC state of solver k (each output may be NULL): mnIterations, mnBestInliers, the hypothesis behind the running best
 * (-1 = none yet) and mRansacMaxIts. */
int ccm_sim3_solver_state(const ccm_sim3_solver*, int k, int32_t* iterations, int32_t* best_inliers, int32_t* best_hypothesis,
                          int32_t* max_iterations);
/* Test / diagnostic tap: what the launch stored for solver k.  Returns the number of hypotheses H (>= 0) or an error; each
 * output may be NULL: sample [H][3] correspondence indices, count [H], rts [H][13] = R (9), t (3), s, mask [H][ceil(N/64)] with
 * correspondence i at bit i % 64 of word i / 64. */
int ccm_sim3_solver_hypotheses(const ccm_sim3_solver*, int k, int32_t* sample, int32_t* count, float* rts, uint64_t* mask);

/* ---- ComputeSim3 on handles: the solver, OptimizeSim3 and the chain.  Links 2 and 4 of LoopFinder::ComputeSim3 / MapMatcher::ComputeSim3
 * with their correspondences named by features, and links 3 + 4 as one call.  A correspondence is a pair of features, i1 of kf1 and i2
 * of kf2; its two map points are the slots the handles hold at those features in mp_id (ccm_frame_set_map_points; the handles need no
 * bow, camera or pose part).  That is vpKeyFrameMP1[i1] exactly, and vpMatched12[i1] for side 2 as long as mObservations and
 * mvpMapPoints agree -- the assumption `observed` of ccm_search_by_projection_table_frames already rests on.  Eight bytes a
 * correspondence go up and nothing per map point.  Per pair the call carries T1w and T2w (rows of [R | t], as in
 * ccm_sim3_search_pair) and K1, K2 (fx, fy, cx, cy); per side and call a table per pyramid level, which the kernels index by the
 * feature's octave without arithmetic: max_err_level for the solver -- mvnMaxError is a vector of size_t (include/cslam/Sim3Solver.h:
 * 74-75), so the caller passes (float)(size_t)(9.210 * mvLevelSigma2[level]) -- and inv_level_sigma2 for the optimiser.
 * Camera-frame points are Xc = R X + t as the "matrix product" defined under "ComputeSim3 on keyframe handles and the table": the
 * solver reads that float, the optimiser reads it, the keypoint and inv_level_sigma2[octave] widened to double (Converter::toVector3d
 * and the Eigen assignments of src/Optimizer.cpp:938-989).  The gathers therefore store the bits the array routes are given by a
 * caller who forms them so, and everything behind them is the array routes' own kernel. */
typedef struct {
    ccm_frame* kf1; ccm_frame* kf2;    /* features and mp_id (table slots) are read; may be the same handle */
    float T1w[12], T2w[12];            /* rows of [R1w | t1w], [R2w | t2w] */
    float K1[4], K2[4];                /* fx, fy, cx, cy of pKF1 / pKF2 */
} ccm_sim3_frames_pair;

/* ccm_sim3_solver_create with the constructor's loop (src/Sim3Solver.cpp:30-83) on the device: k_sim3_solver_gather, one thread per
 * correspondence, fills the four arrays X1 / X2 / max_err1 / max_err2 in front of k_sim3_ransac.  indices1 = feature1, n1[k] = kf1's N.
 * first, fix_scale, the RANSAC parameters, draws, best_inliers and the solver object (every ccm_sim3_solver_* call) are
 * ccm_sim3_solver_create's.  The caller still filters "set and not bad" (:32-59): it needs N for its draws.  Takes a shared lock on
 * the table's rows, works through a view (ccm_map_table_attach), ordered behind earlier writes of handles and table on the context's
 * stream.  CCM_E_ARG with *out untouched: what ccm_sim3_solver_create refuses, a NULL pair, handle or table, n_levels outside
 * 1..CCM_MAX_LEVELS, and -- found on the device before an address is formed -- a feature outside its handle, an mp_id below 0 or
 * outside the table, a slot that is not LIVE, an octave outside [0, n_levels).  A BAD slot is not an error.  (A batch none of whose
 * solvers evaluates a hypothesis launches nothing, the gather included, as for ccm_pnp_solver_create_frames.) */
typedef struct {
    int32_t        n_solvers;
    const ccm_sim3_frames_pair* pairs;          /* [n_solvers] */
    const int32_t* first;        /* [n_solvers+1] */
    const int32_t* fix_scale;    /* [n_solvers] */
    const int32_t* feature1;     /* [..] feature of kf1 */
    const int32_t* feature2;     /* [..] feature of kf2 */
    int32_t n_levels1;  const float* max_err_level1;    /* [n_levels1] side 1 */
    int32_t n_levels2;  const float* max_err_level2;
    double         probability;
    int32_t        min_inliers;
    int32_t        max_iterations;
    const int32_t* draws;        /* [n_solvers][max_iterations][3] */
    const int32_t* best_inliers; /* [n_solvers] or NULL */
} ccm_sim3_solver_frames_problem;
int ccm_sim3_solver_create_frames(ccm_ctx*, ccm_map_table*, const ccm_sim3_solver_frames_problem*, ccm_sim3_solver** out);

/* ccm_optimize_sim3 for n_problems pairs whose correspondences are (feature1, feature2) lists; the caller has applied
 * src/Optimizer.cpp:922-935.  k_sim3_opt_gather fills P1, P2, obs1, obs2, info1, info2 and the unchanged k_sim3_opt runs: for the same
 * pairs the call stores the bits ccm_optimize_sim3 stores.  sim3 [n_problems][8] is in/out, inlier [first[n_problems]] and n_inliers
 * [n_problems] as there.  Locking, order and the errors of a correspondence as for ccm_sim3_solver_create_frames; on an error the
 * outputs are untouched.  One staging copy up, one download, one synchronisation. */
typedef struct {
    int32_t        n_problems;
    const ccm_sim3_frames_pair* pairs;          /* [n_problems] */
    const int32_t* first;        /* [n_problems+1] */
    const int32_t* fix_scale;    /* [n_problems] */
    const float*   th2;          /* [n_problems] */
    const int32_t* feature1;
    const int32_t* feature2;
    int32_t n_levels1;  const float* inv_level_sigma2_1;    /* [n_levels1] mvInvLevelSigma2 of side 1 */
    int32_t n_levels2;  const float* inv_level_sigma2_2;
} ccm_sim3_opt_frames_problem;
typedef struct {
    double*  sim3;               /* [n_problems][8] in/out */
    uint8_t* inlier;             /* [..] out */
    int32_t* n_inliers;          /* [n_problems] out */
} ccm_sim3_opt_frames_result;
int ccm_optimize_sim3_table_frames(ccm_ctx*, ccm_map_table*, const ccm_sim3_opt_frames_problem*, ccm_sim3_opt_frames_result*);

/* From the RANSAC estimate to OptimizeSim3's verdict (src/LoopFinder.cpp:313-330, src/MapMatcher.cpp:318-333) in one call, for every
 * candidate that returned an Scm in one pass of the round-robin.
 *   a. ccm_search_by_sim3_table_frames on `search` of every pair, unchanged; match12 stays on the device.
 *   b. k_sim3_chain_list: per pair, in ascending i1, feature i1 has a match when matched12[i1] >= 0 (then i2 = matched_idx2[i1]) or
 *      match12[i1] >= 0 (then i2 = match12[i1]).  A match becomes a correspondence when kf1's mp_id[i1] names a LIVE slot that is not
 *      BAD, 0 <= i2 < N2 and kf2's mp_id[i2] names a LIVE slot that is not BAD (src/Optimizer.cpp:933-935).  Any other match is left
 *      alone, as the reference `continue`s with vpMatches1[i] still set: a filtered match is never an error.
 *   c. k_sim3_opt_gather and k_sim3_opt on the list, with sim3 (the gScm the caller made of R, t, s), fix_scale and th2 per pair,
 *      K1 = search.fx .. cy and K2.
 *   d. pruned[i1] = 1 exactly where OptimizeSim3 set vpMatches1[i1] to NULL, the first-round prunes of a problem that then
 *      returned 0 (:1032) included; 0 elsewhere.
 * Result: search.match12 / n_found (and the search call's taps) as ccm_search_by_sim3_table_frames gives them; pruned flat over the
 * side-1 features like match12; n_correspondences, n_inliers and sim3 per pair, sim3 untouched in bits where fewer than 10
 * correspondences survive the first round.  Optional taps: corr, the list as (i1, i2) rows, pair p's rows from n_correspondences[0]
 * + .. + n_correspondences[p-1] on ([sum N1][2] holds any list), and inlier per row ([sum N1]).
 * Traffic: one staging copy up; two synchronisations, on the number of queries and on the result; the downloads of the result.
 * Everything behind the query count is queued without a host round trip.  Locking, stream order and errors as for
 * ccm_search_by_sim3_table_frames: found on the host before anything is queued, the outputs then untouched.  In addition CCM_E_ARG for
 * NULL pruned / n_correspondences / n_inliers / sim3, inv_level_sigma2_1 / 2, or a handle whose octaves reach beyond n_levels1 / 2
 * (the handle knows its highest octave).  The function returns the sum of n_found. */
typedef struct {
    ccm_sim3_search_pair search;       /* matched12 / matched_idx2: the solver's inliers; only matched12 >= 0 is read of it */
    float   K2[4];                     /* fx, fy, cx, cy of pKF2 (search.fx .. cy are pKF1's) */
    double  sim3[8];                   /* gScm: qx, qy, qz, qw, tx, ty, tz, s */
    int32_t fix_scale;
    float   th2;                       /* 10 in LoopFinder, 20 in MapMatcher */
} ccm_compute_sim3_pair;
typedef struct {
    int32_t n_pairs;  const ccm_compute_sim3_pair* pairs;
    float th;                                                    /* the search threshold, 7.5 */
    float log_scale_factor1;  int32_t n_levels1;  const float* scale_factors1;  const float* inv_level_sigma2_1;   /* [n_levels1] */
    float log_scale_factor2;  int32_t n_levels2;  const float* scale_factors2;  const float* inv_level_sigma2_2;
} ccm_compute_sim3_problem;
typedef struct {
    ccm_sim3_search_result search;     /* match12, n_found and the optional taps of the search */
    uint8_t* pruned;                   /* [sum N1] */
    int32_t* n_correspondences;        /* [n_pairs] */
    int32_t* n_inliers;                /* [n_pairs] OptimizeSim3's return value */
    double*  sim3;                     /* [n_pairs][8] */
    int32_t* corr;                     /* optional tap [sum N1][2] */
    uint8_t* inlier;                   /* optional tap [sum N1] */
} ccm_compute_sim3_result;
int ccm_compute_sim3_table_frames(ccm_ctx*, ccm_map_table*, const ccm_compute_sim3_problem*, ccm_compute_sim3_result*);

/* ---------------------------------------------------------------- PnPsolver (src/PnPSolver.cpp), batched EPnP RANSAC
 * The link between SearchByBoW against the relocalisation candidates (ccm_kfdb_query_vector, ccm_search_by_bow_frames) and the
 * relocalisation overload of SearchByProjection: one PnPsolver per candidate keyframe, iterate(5) round-robin as ORB-SLAM's
 * Tracking::Relocalization does.  The minimal-set hypotheses of PnPsolver::iterate (:155-249) do not depend on each other (min_set
 * sampled correspondences -> EPnP compute_pose :468-516 -> CheckInliers :299-330), and Refine (:251-296) depends only on which
 * hypothesis is the running best.  ccm_pnp_solver_create evaluates ALL hypotheses of ALL solvers in one launch and every reachable
 * Refine() in a second one; ccm_pnp_solver_iterate / _find replay the ordered bookkeeping over the stored results on the host, so
 * any calling pattern returns what the sequential code returns for the same random draws and the same per-hypothesis poses.
 *
 * Constructor data (:57-100), flattened by the caller: correspondence e of solver k (first[k] <= e < first[k+1], N = first[k+1] -
 * first[k]) = one vpMapPointMatches[i] that is set and not bad, in i order.
 *
 * SetRansacParameters (:111-147) is part of the create call: solver k gets (mRansacMinInliers, mRansacMaxIts) =
 * ccm_pnp_ransac_parameters(N, ...) and mvMaxError[i] = sigma2[i] * th2 (float).  Carrying mnBestInliers over a later
 * SetRansacParameters (the reference does not reset it) is NOT supported: a batch always starts from mnBestInliers = 0, and a caller
 * that changes the parameters creates a new batch.
 *
 * Which hypotheses are stored: the loop condition is mnIterations < mRansacMaxIts || nCurrentIterations < nIterations (:172), so
 * with its || a call can run past mRansacMaxIts.  Solver k evaluates H_k = mRansacMaxIts_k + reserve hypotheses, or none when N <
 * mRansacMinInliers_k (iterate leaves at :163).  iterate with n_iterations needs at most max(mRansacMaxIts_k, mnIterations +
 * n_iterations) hypotheses; beyond H_k it returns CCM_E_STATE and changes nothing.  reserve = the caller's n_iterations covers every
 * caller that drops a solver at bNoMore or at its first return (the call that crosses mRansacMaxIts starts below it and runs at
 * most n_iterations - 1 past it).  A return at or past mRansacMaxIts does not set bNoMore; a caller that rejects such a pose and
 * resumes the solver draws up to n_iterations more per call, so it reserves n_iterations for each rejection it allows for.
 *
 * Sampling (:178-192): the random source stays with the caller.  draws holds the raw RandomInt results: draw i of hypothesis h of
 * solver k at draws[((k * (max_iterations + reserve)) + h) * min_set + i], in [0, N-1-i]; the library applies the reference's
 * swap-with-last removal (position randi takes the last element, :190).  Only the rows of hypotheses that are evaluated are read;
 * one of them outside its range is CCM_E_ARG.
 *
 * Arithmetic: EPnP in double.  What the reference takes from OpenCV (cvSVD of the 3x3 covariance and of the 12x12 M^T M, cvInvert,
 * cvSolve, the 3x3 cvSVD of estimate_R_and_t) is restated with Jacobi iterations.  With min_set = 4 M^T M has a 4-dimensional null
 * space and "the four smallest right singular vectors" (:755-758) are an ARBITRARY basis of it, on which the resulting pose depends
 * (DESIGN.md "PnPsolver"); so does it on the signs of the PCA axes (:391).  Agreement with the reference per hypothesis is therefore
 * not definable.  The contract: the tapped (control points, basis) satisfy their definitions, and everything behind them agrees with
 * a float64 restatement fed with that pair; CheckInliers follows the reference's mixed float / double types step by step without
 * floating-point contraction, so flags and counts are exact functions of the double pose the library reports.  One deviation:
 * qr_solve (:851-941) returns at eta == 0 with X stale (uninitialised on the first step); here that Gauss-Newton step is zero. */
typedef struct {
    int32_t        n_solvers;
    const int32_t* first;        /* [n_solvers+1], first[0] = 0, non-decreasing */
    const int32_t* n1;           /* [n_solvers] mvpMapPointMatches.size(), the length of vbInliers */
    const float*   K;            /* [n_solvers][4] fx, fy, cx, cy (:94-97) */
    const float*   P2D;          /* [..][2] mvKeysUn[i].pt */
    const float*   P3Dw;         /* [..][3] GetWorldPos() */
    const float*   sigma2;       /* [..] mvLevelSigma2[octave] */
    const int32_t* kp_index;     /* [..] mvKeyPointIndices, each in [0, n1[k]) */
    double         probability;  /* SetRansacParameters(probability = 0.99, minInliers = 8, maxIterations = 300, minSet = 4, */
    int32_t        min_inliers;  /*                     epsilon = 0.4, th2 = 5.991)  (PnPSolver.h:91) */
    int32_t        max_iterations;
    int32_t        min_set;      /* 4 .. 8, otherwise CCM_E_ARG */
    float          epsilon;
    float          th2;
    int32_t        reserve;      /* hypotheses stored past mRansacMaxIts, >= 0 (see above) */
    const int32_t* draws;        /* [n_solvers][max_iterations + reserve][min_set] */
    uint32_t       flags;        /* bit 0: keep the detail tap */
} ccm_pnp_ransac_problem;
typedef struct ccm_pnp_solver ccm_pnp_solver;
#define CCM_PNP_DETAIL 68        /* doubles per row of the detail tap: cws[12], basis[4][12] (v[0..3] = ut rows 11..8), betas[4] of
                                  * the chosen candidate, rep_error[3], which (1..3) */

/* SetRansacParameters (:119-142) for N = n correspondences: nMinInliers = (int)(N * epsilon) in float, raised to min_inliers and to
 * min_set; epsilon raised to (float)nMinInliers / N; nIterations = 1 if nMinInliers == N, else ceil(log(1 - probability) / log(1 -
 * pow(epsilon, 3))) with the float epsilon raised to 3 in double; max(1, min(nIterations, max_iterations)).  For N < nMinInliers
 * (which includes N = 0) the reference's value is undefined and unused (iterate leaves at :163); it is 1 here.  Host only; each
 * output may be NULL. */
int ccm_pnp_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                              int32_t* min_inliers_out, int32_t* max_its_out, float* epsilon_out);
/* EPnP compute_pose (:468-516) of n >= 4 correspondences on the host, the same arithmetic as the kernels: Rt = R (9, row-major), t
 * (3).  detail may be NULL, else CCM_PNP_DETAIL doubles.  Needs no device.  n < 4 or a null array: CCM_E_ARG, outputs untouched. */
int ccm_pnp_compute_pose(int n, const float* P3Dw, const float* P2D, const float* K, double* Rt, double* detail);
/* One upload of the batch, k_pnp_hypotheses, one download and synchronisation; the records (hypotheses that become the running best)
 * are found by a scan over the counts on the host and their list (24 bytes each) goes up; k_pnp_refine, one download and a second
 * synchronisation (none of the three when no hypothesis reaches mRansacMinInliers).  Device memory is the context's
 * (grow-only, reused by the next batch); the solver object holds host memory only and belongs to the thread that made it.  On an
 * error *out is untouched. */
int ccm_pnp_solver_create(ccm_ctx*, const ccm_pnp_ransac_problem*, ccm_pnp_solver** out);
/* ccm_pnp_solver_create with the constructor's loop (:69-91) on the device: correspondence e is named by two 4-byte numbers, feature
 * i = feature[e] of the current frame's handle and slot[e], the table slot of vpMapPointMatches[i], in the place of P2D, P3Dw,
 * sigma2 and kp_index (24 bytes).  k_pnp_gather, one thread per correspondence in front of k_pnp_hypotheses, fills the same three
 * device arrays the array route uploads: P2D = (kx[i], ky[i]) of the handle, P3D = the slot's pos, max_err = level_sigma2[oct[i]] *
 * th2 in float, the product ccm_pnp_solver_create forms.  kp_index is feature and n1[k] is the handle's N for every solver, so
 * iterate's inliers has N entries.  Everything else -- first, K (per solver), the RANSAC parameters, draws, flags, the two solver
 * kernels and the host replay -- is ccm_pnp_solver_create's, and the solver object answers every ccm_pnp_solver_* call alike: for
 * the same frame, table rows and draws both routes store the same bits.  The caller still filters "set and not bad" (:75-80): it
 * needs N_k for its draws.
 * Errors, each CCM_E_ARG with *out untouched: n_levels outside 1..CCM_MAX_LEVELS; a feature outside [0, N) or a slot outside the
 * table (found on the host); a slot that is not LIVE or an octave outside [0, n_levels) (found by the kernel, which writes zeros for
 * that correspondence and never forms the address; reported with the first download, before the refinements).  When no solver has
 * enough correspondences to evaluate a hypothesis nothing is launched and only the host checks run.  BAD is not an error: a caller
 * that keeps a bad point gets its position, as the array route would.
 * Traffic: the upload is 8 bytes per correspondence plus 64 bytes of level_sigma2, 16 per hypothesis and 64 per solver as before;
 * downloads and the two synchronisations are those of ccm_pnp_solver_create.  Reads the table's rows (a shared lock). */
typedef struct {
    int32_t        n_solvers;
    const int32_t* first;        /* [n_solvers+1], as ccm_pnp_ransac_problem */
    const float*   K;            /* [n_solvers][4] */
    const int32_t* feature;      /* [..] feature of cur (mvKeyPointIndices) */
    const int32_t* slot;         /* [..] table slot */
    const float*   level_sigma2; /* [n_levels] mvLevelSigma2 */
    int32_t        n_levels;
    double         probability;  /* the rest as ccm_pnp_ransac_problem */
    int32_t        min_inliers;
    int32_t        max_iterations;
    int32_t        min_set;
    float          epsilon;
    float          th2;
    int32_t        reserve;
    const int32_t* draws;
    uint32_t       flags;
} ccm_pnp_frames_problem;
int ccm_pnp_solver_create_frames(ccm_ctx*, ccm_frame* cur, ccm_map_table* table, const ccm_pnp_frames_problem*, ccm_pnp_solver** out);
/* NULL is a no-op. */
void ccm_pnp_solver_destroy(ccm_pnp_solver*);
/* n_solvers of the batch, or CCM_E_ARG for NULL. */
int ccm_pnp_solver_count(const ccm_pnp_solver*);
/* PnPsolver::iterate(nIterations, bNoMore, vbInliers, nInliers) (:155-249) of solver k, exactly.  The outputs are cleared first
 * (:157-159); N < mRansacMinInliers -> *no_more = 1 and nothing else (:163-167).  For each hypothesis in order with mnInliersi >=
 * mRansacMinInliers: it becomes the running best if mnInliersi > mnBestInliers (:203); then Refine() of the CURRENT best is
 * consulted (:217) and returns when its count is > mRansacMinInliers (:283, strict): *found = 1, Tcw = the refined pose as float
 * (4x4 row-major), *n_inliers the refined count, inliers[mvKeyPointIndices[i]] = 1 over the refined mask.  After the loop,
 * mnIterations >= mRansacMaxIts sets *no_more = 1 and, if mnBestInliers >= mRansacMinInliers, returns found with the best
 * hypothesis' own pose, count and mask (:232-246).  mnIterations and mnBestInliers persist over calls.  inliers has n1[k] entries;
 * inliers and Tcw may be NULL; Tcw is untouched unless *found.  CCM_E_STATE: the call would need hypotheses beyond the reserve. */
int ccm_pnp_solver_iterate(ccm_pnp_solver*, int k, int n_iterations, int32_t* found, int32_t* no_more, uint8_t* inliers,
                           int32_t* n_inliers, float* Tcw);
/* PnPsolver::find (:149-153) = iterate(mRansacMaxIts) without bNoMore. */
int ccm_pnp_solver_find(ccm_pnp_solver*, int k, int32_t* found, uint8_t* inliers, int32_t* n_inliers, float* Tcw);
/* The RANSAC state of solver k (each output may be NULL): mnIterations, mnBestInliers, the hypothesis behind the running best
 * (-1 = none yet), mRansacMaxIts and mRansacMinInliers. */
int ccm_pnp_solver_state(const ccm_pnp_solver*, int k, int32_t* iterations, int32_t* best_inliers, int32_t* best_hypothesis,
                         int32_t* max_iterations, int32_t* min_inliers);
/* Test / diagnostic taps of solver k.  Each returns the number of rows (>= 0) or an error; each output may be NULL.
 * _hypotheses: H rows: sample [H][min_set] correspondence indices, count [H], Rt [H][12] double, mask [H][ceil(N/64)] with
 * correspondence i at bit i % 64 of word i / 64, detail [H][CCM_PNP_DETAIL] (CCM_E_STATE unless the batch was created with flag bit
 * 0).  _refinements: R rows, one per record in hypothesis order: hyp [R] the record hypothesis whose mask was refined (:256-272),
 * count [R] mnRefinedInliers, Rt, mask = mvbRefinedInliers, detail. */
int ccm_pnp_solver_hypotheses(const ccm_pnp_solver*, int k, int32_t* sample, int32_t* count, double* Rt, uint64_t* mask, double* detail);
int ccm_pnp_solver_refinements(const ccm_pnp_solver*, int k, int32_t* hyp, int32_t* count, double* Rt, uint64_t* mask, double* detail);

/* ---- Initializer: the monocular two-view initialisation (src/Initializer.cpp, called from Tracking::MonocularInitialization,
 * src/Tracking.cpp:293-357, between ccm_search_for_initialization and the first ccm_ba_solve).
 * Initializer::Initialize (:40-117) evaluates mMaxIterations minimal sets of 8 matches twice -- FindHomography (:120-168) and
 * FindFundamental (:171-219) in two threads, each hypothesis scored over all N matches -- picks a model from the score ratio
 * (:108-114) and reconstructs the motion from it (ReconstructH :568-728, ReconstructF :466-566), testing 8 or 4 motion hypotheses
 * with CheckRT (:794-903).  ccm_initialize does the 2 x mMaxIterations hypotheses in one launch and all CheckRT calls in a second
 * one; the ordered parts (first strictly best score :161-166 / :212-217, the decisions :495-565 / :685-727) are replayed on the host
 * over the stored results.
 *
 * Arithmetic: float storage and float per-match arithmetic in the reference's operation order (Normalize :745-791 with sums in index
 * order over ALL keypoints of each frame, the rows of ComputeH21 / ComputeF21, CheckHomography, CheckFundamental, CheckRT).  The null
 * vectors that the reference takes from cv::SVDecomp (9 unknowns, the rank-2 step, Triangulate, the 3x3 SVDs of the reconstruction)
 * come from a cyclic Jacobi in double on A^T A; cv::SVDecomp, cv::Mat::inv and cv::gemm are not part of the reference tree, so the
 * contract on H21 / H12 / F21 is a tolerance (DESIGN.md "Initializer"), while the inlier flags, scores and decisions are exact
 * functions of the matrices the library reports.
 *
 * The sign conventions of cv::SVD are not defined by the reference, so the ORDER of the 8 (4) motion candidates may differ from the
 * reference's.  It cannot change the outcome: in ReconstructF two candidates equal to maxGood make nsimilar > 1, in ReconstructH a
 * tie makes secondBestGood = bestGood, and both reject.  The contract is on the chosen (R21, t21, points), not on a candidate index. */
typedef struct {
    int32_t        n1;              /* mvKeys1.size() */
    const float*   kp1_xy;          /* [n1][2] mvKeysUn of the reference frame */
    int32_t        n2;
    const float*   kp2_xy;          /* [n2][2] mvKeysUn of the current frame */
    const int32_t* matches12;       /* [n1] index into frame 2, or < 0 (vMatches12); N = number of entries >= 0 */
    float          fx, fy, cx, cy;  /* mK */
    float          sigma;           /* mSigma (1.0) */
    int32_t        max_iterations;  /* mMaxIterations (200) */
    float          min_parallax;    /* 1.0 (:112) */
    int32_t        min_triangulated;/* 50 (:112) */
    /* [max_iterations][8]: the raw results of DUtils::Random::RandomInt(0, vAvailableIndices.size()-1) at :85.  Draw j of a set lies in
     * [0, N-1-j]; the library turns the draws into match indices by the swap-with-last removal of :86-91.  The random source stays
     * with the caller (the reference seeds it with SeedRandOnce(0), :76). */
    const int32_t* draws;
} ccm_initializer_problem;
/* Test / diagnostic tap of ccm_initialize; every pointer may be NULL.  `it` runs over the max_iterations sets, words = ceil(N / 64),
 * match i (in mvMatches12 order: ascending frame-1 index) is bit i % 64 of word i / 64. */
typedef struct {
    float*    H21;                  /* [it][9] H21i (:156) */
    float*    H12;                  /* [it][9] H12i (:157) */
    float*    F21;                  /* [it][9] F21i (:208) */
    float*    score_h;              /* [it] currentScore of FindHomography */
    float*    score_f;              /* [it] currentScore of FindFundamental */
    uint64_t* mask_h;               /* [it][words] vbCurrentInliers of CheckHomography */
    uint64_t* mask_f;               /* [it][words] vbCurrentInliers of CheckFundamental */
    int32_t*  sets;                 /* [it][8] mvSets */
    /* the reconstruction: 8 (ReconstructH), 4 (ReconstructF) or 0 candidates (none tested: N < 8, no set scored, or the early exit
     * d1/d2 < 1.00001 || d2/d3 < 1.00001 of :593) */
    int32_t   n_candidates;
    float     cand_R[8][9];
    float     cand_t[8][3];
    int32_t   cand_n_good[8];       /* nGood of CheckRT */
    float     cand_parallax[8];     /* parallax of CheckRT, degrees */
    uint8_t*  cand_flags;           /* [8][N]: bit 0 = the match counts in nGood (vP3D written), bit 1 = vbGood */
    float*    cand_cos;             /* [8][N] cosParallax where bit 0 is set */
    float*    cand_p3d;             /* [8][N][3] p3dC1 where bit 0 is set */
} ccm_initializer_tap;
typedef struct {
    int32_t  initialized;           /* the return value of Initialize */
    int32_t  model;                 /* 0 = ReconstructH ran, 1 = ReconstructF (RH > 0.40 is false, also for RH = NaN when both scores are 0) */
    float    score_h, score_f;      /* SH, SF */
    int32_t  best_h, best_f;        /* the sets behind them, -1 if no set scored > 0 */
    int32_t  n_matches;             /* N */
    float    R21[9], t21[3];        /* row-major; written when initialized */
    float*   p3d;                   /* in: [n1][3] caller-allocated; out: vP3D, indexed by frame-1 keypoint */
    uint8_t* triangulated;          /* in: [n1] caller-allocated; out: vbTriangulated.  Both arrays are cleared first and stay cleared
                                     * when initialized == 0 */
    ccm_initializer_tap* tap;       /* in: NULL or a tap to fill */
} ccm_initializer_result;
/* One Initializer::Initialize.  N < 8: returns CCM_OK with initialized = 0 and launches nothing (the reference would sample out of
 * range; its caller guards with nmatches < 100).  A set whose score is not > 0 never becomes the best; if the chosen model has no
 * best set, initialized = 0.  Errors (CCM_E_ARG: a NULL array, a draw outside [0, N-1-j], a matches12 entry >= n2, max_iterations <
 * 1) leave every output untouched and name the argument in ccm_last_error.  p3d, triangulated and tap are read before anything is
 * written, so a result object can be reused. */
int ccm_initialize(ccm_ctx*, const ccm_initializer_problem*, ccm_initializer_result*);

/* ---- LocalMapping::CreateNewMapPoints (src/Mapping.cpp:284-469), once per keyframe: for each of up to 20 covisible neighbours
 * SearchForTriangulation (ORBmatcher.cpp:700-852, constructed as ORBmatcher(0.6, false): no rotation histogram), then per matched
 * pair the parallax test, the linear triangulation, the depth, reprojection and scale tests (:363-448).
 *
 * The loop is separable.  vbMatched2 is declared in SearchForTriangulation but never set (:721, :763) and there is no orientation
 * filter, so the match of feature i1 against neighbour k depends on (k, i1) and on the map-point flags at entry only.  The one
 * sequential rule -- a feature that received a point with neighbour k is skipped for the neighbours after k -- reduces to: i1 belongs
 * to the FIRST neighbour, in order, where it has a match that passes every gate; later results for i1 are dropped.
 * ccm_create_new_map_points matches and triangulates every (k, i1) in parallel and resolves that order on the device: three
 * launches whatever n_kf is, one upload, one download, one synchronisation.  No candidate distance leaves the device.
 *
 * Arithmetic: the match (Hamming distance <= TH_LOW = 50, the epipole test :775-777, CheckDistEpipolarLine :159-176, smallest
 * distance and the last in node order among equals) is exact: the same float operations as ccm_search_for_triangulation.
 * Triangulation and gates: float storage in the reference's operation order; the sums of cv::Mat products, dot and norm are taken in
 * double; the null vector of the float 4x4 comes from a cyclic Jacobi in double on A^T A (cv::SVD is not part of the reference tree),
 * so the contract on the point is a tolerance against a float64 restatement (DESIGN.md "CreateNewMapPoints") while every gate from
 * the depth test on is an exact function of the point the library reports.
 * Deviation: the reference has no test for a non-finite point and would create it (every later comparison with NaN is false); here
 * such a pair gets CCM_NP_NONFINITE and creates nothing. */
typedef struct {
    int32_t        n;                 /* KeyFrame::N */
    const float*   kp_x;              /* [n] mvKeysUn[i].pt.x */
    const float*   kp_y;
    const int32_t* kp_octave;         /* [n] mvKeysUn[i].octave, each in [0, n_levels) */
    const uint8_t* desc;              /* [n][32] mDescriptors */
    const int32_t* node;              /* [n] FeatureVector node of feature i, -1 for none, as for ccm_match_bow; below 2^24 */
    const uint8_t* has_mp;            /* [n] GetMapPoint(i) != null when CreateNewMapPoints is entered */
    float          fx, fy, cx, cy;
    const float*   Tcw;               /* [12] rows of [Rcw | tcw] (GetRotation, GetTranslation) */
    const float*   Ow;                /* [3] GetCameraCenter() as the keyframe stores it */
    const float*   scale_factors;     /* [n_levels] mvScaleFactors */
    const float*   level_sigma2;      /* [n_levels] mvLevelSigma2 */
    int32_t        n_levels;
} ccm_map_keyframe;
typedef struct {
    const ccm_map_keyframe* current;     /* mpCurrentKeyFrame */
    int32_t                 n_kf;
    const ccm_map_keyframe* neighbours;  /* [n_kf] GetBestCovisibilityKeyFrames(20), in that order */
    const float*            F12;         /* [n_kf][9] row-major ComputeF12(current, neighbour k) (Mapping.cpp:549-566) */
    const float*            epipole;     /* [n_kf][2] ex, ey of ORBmatcher.cpp:708-714 */
    const float*            median_depth;/* [n_kf] neighbour k's ComputeSceneMedianDepth(2), > 0 */
} ccm_new_points_problem;
/* What became of (neighbour k, feature i1).  The gate codes follow the order of Mapping.cpp:363-448. */
enum {
    CCM_NP_SKIPPED_KF = 0,    /* baseline / median depth < 0.01 (:319-328): the whole neighbour */
    CCM_NP_HAS_MP,            /* the feature already holds a map point on entry */
    CCM_NP_NO_MATCH,          /* no match for (k, i1) */
    CCM_NP_LOW_PARALLAX,      /* fails cos > 0 && cos < 0.9998 (:373) */
    CCM_NP_W_ZERO,            /* fourth component of the null vector is 0 (:387) */
    CCM_NP_NONFINITE,         /* the point has a non-finite coordinate (deviation, see above) */
    CCM_NP_BEHIND_1,          /* z1 <= 0 (:401) */
    CCM_NP_BEHIND_2,          /* z2 <= 0 (:405) */
    CCM_NP_REPROJ_1,          /* reprojection gate in the current keyframe (:418) */
    CCM_NP_REPROJ_2,          /* reprojection gate in the neighbour (:431) */
    CCM_NP_ZERO_DIST,         /* dist1 == 0 || dist2 == 0 (:441) */
    CCM_NP_SCALE,             /* scale consistency (:447) */
    CCM_NP_OK,                /* the winner for this feature: a row of the result list */
    CCM_NP_SUPERSEDED         /* passes every gate, but an earlier neighbour already won this feature */
};
/* Test / diagnostic tap; every pointer may be NULL.  n1 = current->n. */
typedef struct {
    int32_t* match;                   /* [n_kf][n1] the independent match of (k, i1): index into neighbour k, or -1 */
    uint8_t* status;                  /* [n_kf][n1] CCM_NP_* */
    float*   x3d_all;                 /* [n_kf][n1][3] the point wherever one was computed (status >= CCM_NP_NONFINITE), else 0 */
} ccm_new_points_tap;
/* Caller-allocated arrays with room for current->n rows (a feature wins at most once); rows past n_new are not written.  The order
 * is the reference's creation order: neighbour by neighbour, idx1 ascending inside a neighbour. */
typedef struct {
    int32_t  n_new;                   /* out */
    int32_t* kf;                      /* [n_new] neighbour index */
    int32_t* idx1;                    /* [n_new] feature of the current keyframe */
    int32_t* idx2;                    /* [n_new] feature of neighbour kf */
    float*   x3d;                     /* [n_new][3] */
    int32_t* first;                   /* [n_kf+1] the new points of neighbour k are rows first[k] .. first[k+1]-1 */
    ccm_new_points_tap* tap;          /* in: NULL (production) or a tap to fill */
} ccm_new_points_result;
/* Returns n_new (>= 0) or an error.  CCM_E_ARG (a null pointer, n_kf < 0, an octave outside [0, n_levels), a median_depth that is
 * not positive, a node >= 2^24) names the argument in ccm_last_error and touches no output, the tap included.  n_kf == 0,
 * current->n == 0 and a neighbour with n == 0 are valid: the call returns 0, or that neighbour contributes nothing. */
int ccm_create_new_map_points(ccm_ctx*, const ccm_new_points_problem*, ccm_new_points_result*);
/* The same call on keyframe handles (ccm_frame_set_bow / _camera / _pose, "frame handles" above): the neighbourhood of a keyframe
 * moves slowly, so the same 20 to 30 keyframes come back call after call and nothing of them is uploaded again.  has_mp of every
 * keyframe is mp_id[i] >= 0 as the handle holds it when the call is made; the call writes into no handle (new points get ids when the
 * caller creates them, :451-466).  The baseline rule (:319-328) runs on the host copies of Ow the handles keep.  Per call: one staged
 * upload whose size depends on n_kf only, three launches, one download, one synchronisation.
 * Same result structure, tap, ordering, return value and bytes as ccm_create_new_map_points for the same data, and the same
 * argument checks (CCM_E_ARG: a null pointer, n_kf < 0, a median_depth that is not positive, n_kf * n above 2^30, a handle of
 * another context, current with fewer than 2 levels).  CCM_E_STATE names the keyframe and what it lacks, e.g. "neighbours[3]: no
 * pose".  No output is touched on an error. */
typedef struct {
    ccm_frame*        current;
    int32_t           n_kf;
    ccm_frame* const* neighbours;    /* [n_kf]; the same handle may appear more than once */
    const float*      F12;           /* as ccm_new_points_problem */
    const float*      epipole;
    const float*      median_depth;
} ccm_new_points_frames;
int ccm_create_new_map_points_frames(ccm_ctx*, const ccm_new_points_frames*, ccm_new_points_result*);

/* ---- The per-neighbour inputs of the two calls above, defined.  median_depth, F12 and the epipole come from the caller; these
 * plain host functions (no context, no GPU) state what the library means by them, in arithmetic a device kernel can repeat bit for
 * bit (csrc/map_math.h: functions for host and device, built without fused multiply-add), so that a later form of the call can
 * compute them on the device from the handles and the map-point table.
 *
 * ccm_map_pair_geometry = LocalMapping::ComputeF12 (src/Mapping.cpp:549-566) and the epipole of ORBmatcher.cpp:708-714, in the
 * library's reading of float cv::Mat products: each entry of a product is summed in double (k ascending) and stored as float,
 * element-wise adds are in float.  K = (fx, fy, cx, cy), Tcw = rows of [Rcw | tcw], 1 = the current keyframe, 2 = the neighbour:
 *     R12 = R1w * R2w^T;   t12 = (-R1w * R2w^T) * t2w + t1w   (products left to right, each stored as float; the add in float)
 *     F12 = ((K1^-T * [t12]x) * R12) * K2^-1                  (left to right, row-major [3][3])
 *     K^-1 = [ a 0 c ; 0 b d ; 0 0 1 ] in closed form, each entry one division in double stored as float:
 *            a = (float)(1.0 / fx), b = (float)(1.0 / fy), c = (float)(-(double)cx / fx), d = (float)(-(double)cy / fy)
 *            -- not the product form -cx * (1 / fx).  K^-T is its transpose, entry for entry.
 *     C2 = R2w * Ow1 + t2w;  invz = 1.0f / C2.z;  epipole = (fx2 * C2.x * invz + cx2, fy2 * C2.y * invz + cy2)   (float)
 * This is the operation order of the Python helpers mapping.compute_f12 / compute_epipole.  A numerically inverted K (cv::Mat::inv,
 * numpy.linalg.inv) may differ from the closed form by one float ulp in c or d, and not by the same amount for K and K^T; the C
 * function is the definition, and mapping.compute_f12 is held to it by a bound, not by bits.  The epipole involves no inverse and is
 * bit-equal.  Returns CCM_E_ARG for a NULL pointer. */
int ccm_map_pair_geometry(const float K1[4], const float Tcw1[12], const float Ow1[3], const float K2[4], const float Tcw2[12],
                          float F12[9], float epipole[2]);
/* ccm_scene_median_depth = KeyFrame::ComputeSceneMedianDepth(2) (src/KeyFrame.cpp:1241-1272) of a keyframe whose features carry
 * table slots in mp_id [n], on the table columns pos [capacity][3] and flags [capacity].
 *   Feature i counts iff 0 <= mp_id[i] < capacity and the row has CCM_MP_LIVE.  CCM_MP_BAD rows count: the reference tests
 *   IsEmpty(), not isBad().
 *   Its depth is z = Rcw.row(2) . pos + tcw.z: the dot in double, the add in double, stored as float.
 *   *median = the depth of rank (m - 1) / 2 in ascending order of the m counted depths (vDepths[(size - 1) / q], q = 2);
 *   *n_depths = m.
 * Deviations: a non-finite depth is not counted (the reference would sort it in); m == 0 is undefined behaviour in the reference
 * (it indexes an empty vector) and gives n_depths = 0 and median = 0 here; -0.0f orders
 * before +0.0f (std::sort leaves their order open).  Returns CCM_E_ARG for n < 0, capacity < 0 or a NULL array that would be read. */
int ccm_scene_median_depth(int n, const int32_t* mp_id, int capacity, const float* pos, const uint8_t* flags, const float Tcw[12],
                           float* median, int32_t* n_depths);

/* The optimisation inside Optimizer::OptimizeEssentialGraphLoopClosure / OptimizeEssentialGraphMapFusion
 * (src/Optimizer.cpp:1064-1331, :1333-1574): one VertexSim3Expmap per keyframe (sim3 = Scw or the corrected Sim3,
 * :1094-1108; fixed = pLoopKF, :1110), one EdgeSim3 per loop / spanning-tree / covisibility edge built by the caller
 * exactly as :1123-1250 with edge_i = vertex 0, edge_j = vertex 1, measurement = Sji; identity information, numeric
 * Jacobians, Levenberg with lambda 1e-16, `iterations` = 20.  sim3 comes back as the CorrectedSiw of :1262.
 * Solved like :1072-1074 (BlockSolver_7_3 + sparse Cholesky): block-sparse normal equations, fill-reducing ordering once per call,
 * numeric factorisation per LM trial on the device; no dense matrix. */
typedef struct {
    int32_t        n_vertices;
    double*        sim3;          /* [n_vertices][8] in/out: qx,qy,qz,qw, tx,ty,tz, s */
    const uint8_t* fixed;         /* [n_vertices] */
    int32_t        fix_scale;     /* bFixScale */
    int32_t        n_edges;
    const int32_t* edge_i;        /* [n_edges] */
    const int32_t* edge_j;
    const double*  measurement;   /* [n_edges][8] */
    int32_t        iterations;
    int32_t        iterations_done;   /* out */
    double         chi2_initial, chi2_final;   /* out */
    /* out, the block-sparse solve: 7x7 blocks of the Cholesky factor (diagonal + lower, fill included), rounds of independent
     * columns (= launches per factorisation), device bytes of system + factor */
    int32_t        factor_blocks, factor_rounds;
    int64_t        solver_bytes;
} ccm_essential_graph;
int ccm_optimize_essential_graph(ccm_ctx*, ccm_essential_graph*);
/* Map point correction that follows it (:1300-1330): points[i] <- correctedSwr.map(Srw.map(points[i])) with r =
 * ref_vertex[i] (-1: leave the point), Srw = sim3_before[r] (vScw), correctedSwr = inverse(sim3_after[r]). */
int ccm_correct_map_points(ccm_ctx*, int n_points, double* points, const int32_t* ref_vertex, int n_vertices, const double* sim3_before,
                           const double* sim3_after);

/* ---------------------------------------------------------------- local BA on the table
 * Optimizer::LocalBundleAdjustmentClient (src/Optimizer.cpp:349-644) on keyframe handles and the map-point table: ccm_ba_solve
 * whose observations (mvKeysUn[..].pt), information values (mvInvLevelSigma2[octave]) and points (GetWorldPos) are read where they
 * already lie in device memory, and whose results are written back there.
 *   Graph: keyframe k = handle kfs[k] with poses / fixed / intr as in ccm_ba_problem; point p = table slot slot[p]; point p owns
 *   entries obs_first[p] .. obs_first[p+1] of obs_kf / obs_feat (the three lists of ccm_map_refresh).  Edge e of the graph is entry e
 *   of those lists, point-major: the order of vpEdgesMono.  ccm_ba_result.edge_outlier, when given, is in that order.
 *   Contract: the call returns what ccm_ba_solve returns -- poses, every field of ccm_ba_result and edge_outlier, bit for bit -- for
 *   the array problem built from the same data by widening:
 *     obs[e] = ((double)kx[f], (double)ky[f]), f = obs_feat[e], of handle kfs[obs_kf[e]];  info[e] = (double)inv_level_sigma2[oct[f]];
 *     points[p][k] = (double)pos[slot[p]][k];  edge_pose = obs_kf, edge_point = the point index;  poses, fixed, intr, options passed on.
 *   This holds for every graph the array route accepts: a point seen once, a keyframe without observations, a point with an empty
 *   list (a vertex without edges).
 *   Afterwards the device writes, and nothing of this is uploaded again:
 *     pos[slot[p]][k] = (float)points[p][k] (the cast of Converter::toCvMat) for every listed point; the same values go to pos_out.
 *     The other columns, the rows of other slots and the seen stamps are untouched; flags is neither read nor written.
 *     For publish[k] != 0 the handle's Tcw / Ow (what ccm_frame_set_pose sets) become ccm_pose_to_camera(poses[k]), on the device and
 *     in the handle's host copy; a handle without a keyframe block gets one, as ccm_frame_set_pose would give it.
 *   When the solve made no LM iteration because the stop flag was up on entry (:531-533 returns before writing anything), table and
 *   handles are left exactly as they were; pos_out then holds the table's values.
 * ccm_pose_to_camera (host only, no context): Tcw = rows 0-2 of what ccm_pose_to_mat4f gives;
 *   Ow[r] = (float)(((-(double)R[0][r]) * t0 - (double)R[1][r] * t1) - (double)R[2][r] * t2), R and t the float entries of Tcw widened
 *   (-Rwc * tcw of KeyFrame::SetPose, src/KeyFrame.cpp:299-302).  One definition serves host and device (csrc/pose_camera.h).
 * The call is a writer of the table's rows (a view on another thread sees the new positions in any call that starts after this one
 * returns) and is ordered on the context's stream behind earlier ccm_frame_set_* / ccm_map_table_update / _refresh calls.  One
 * page-locked staging copy goes up (pose7, intr, slots, the feature indices in the device's edge order, one small view of device
 * pointers per keyframe, the level table, publish) beside the index arrays ccm_ba_solve uploads for any problem: nothing per edge or
 * per point beyond 4-byte indices.  One download: pose7, the outlier bytes, pos_out.  No synchronisation beyond those of the LM loop
 * and the final one.
 * Errors are found on the host before anything is queued; table, handles and outputs are then untouched.  CCM_E_ARG: a NULL required
 * array (kfs, poses, fixed, intr, inv_level_sigma2; slot, obs_first with points; obs_kf, obs_feat with observations), n_kf <= 0, a
 * handle listed twice, a slot out of range or listed twice, obs_first not ascending from 0, a keyframe index outside [0, n_kf), a
 * feature index outside that handle's [0, N) (the message names the point and the entry), n_levels below a listed handle's own
 * n_levels or outside 1..CCM_MAX_LEVELS, a handle or table of another context.  CCM_E_STATE: a handle or table that outlived its
 * context; a context with a communicator of more than one rank (the table route is unsharded). */
typedef struct {
    int32_t           n_kf;
    ccm_frame* const* kfs;         /* [n_kf] keyframe handles, no handle twice */
    double*           poses;       /* [n_kf][7] in/out, as ccm_ba_problem.poses */
    const uint8_t*    fixed;       /* [n_kf] */
    const double*     intr;        /* [n_kf][4] */
    const uint8_t*    publish;     /* [n_kf] or NULL: write the optimised pose into this handle */
    int32_t           n_points;
    const int32_t*    slot;        /* [n_points] table slots, none twice */
    const int32_t*    obs_first;   /* [n_points+1] ascending from 0 */
    const int32_t*    obs_kf;      /* [obs_first[n_points]] index into kfs */
    const int32_t*    obs_feat;    /* [obs_first[n_points]] feature index in that keyframe */
    const float*      inv_level_sigma2; int32_t n_levels;   /* mvInvLevelSigma2 */
    float*            pos_out;     /* optional [n_points][3]: the positions written to the table */
} ccm_ba_table_problem;
int ccm_ba_solve_table_frames(ccm_ctx*, ccm_map_table*, ccm_ba_table_problem*, const ccm_ba_options*, ccm_ba_result*);
int ccm_pose_to_camera(const double* pose7, float* Tcw12, float* Ow3);
/* Test tap: Tcw [12] and Ow [3] as the DEVICE copy of the handle holds them; synchronises.  CCM_E_STATE without a pose. */
int ccm_frame_get_pose(ccm_frame*, float* Tcw12, float* Ow3);

/* Multi-GPU GBA: every rank calls ccm_ba_solve with the
 * SAME poses and ITS OWN landmark partition (points + their edges); the reduced
 * camera system is summed with one RCCL all-reduce per LM trial.  One rank
 * makes an id, the host program distributes it (e.g. torch.distributed
 * broadcast), every rank calls ccm_comm_init.  */
/* The landmark ranges ccm_ba_solve gives to the ranks (host only, no GPU): cuts[r] .. cuts[r+1]-1 -> rank r. */
int ccm_ba_landmark_cuts(const int32_t* edge_point, int n_edges, int n_points, int n_ranks, int32_t* cuts);
#define CCM_COMM_ID_BYTES 128
int ccm_comm_unique_id(uint8_t id[CCM_COMM_ID_BYTES]);
int ccm_comm_init(ccm_ctx*, const uint8_t id[CCM_COMM_ID_BYTES], int n_ranks, int rank);
/* Bring-your-own transport: a host that already has a collective layer (MPI, a test harness) attaches it instead of
 * RCCL.  The callbacks receive DEVICE pointers and the context's HIP stream; they must leave the reduced values in
 * place and return 0, or non-zero on failure (reported as CCM_E_COMM).  `destroy` runs when the context drops the
 * communicator.  The sharded solve is the same code path as with ccm_comm_init except for the all-reduce itself.
 * (tests/support/shm_transport.cpp, a shared-memory all-reduce between processes sharing ONE GPU, is such a transport:
 * it lets the sharded global BA be rehearsed end to end on a one-GPU box; it is not part of this library.) */
typedef struct {
    void* user;
    int  (*allreduce_f64)(void* user, double* dev, size_t n, int max_op, void* hip_stream);
    int  (*allreduce_u8_max)(void* user, uint8_t* dev, size_t n, void* hip_stream);
    void (*destroy)(void* user);
} ccm_comm_transport;
int ccm_comm_attach(ccm_ctx*, const ccm_comm_transport*, int n_ranks, int rank);
int ccm_comm_destroy(ccm_ctx*);

/* SE3Quat / Converter helpers (src/Converter.cc:40-56, 86-93): float32 4x4 row-major
 * Tcw <-> quaternion+translation double[7]. Host only. */
int ccm_pose_from_mat4f(const float* T16, double* pose7);
int ccm_pose_to_mat4f(const double* pose7, float* T16);

/* --------------------------------------------------------- KeyFrameDatabase
 * Place recognition: KeyFrameDatabase::add / erase / clear (cslam/src/Database.cpp:37-70) and the candidate queries
 * DetectLoopCandidates / DetectMapMatchCandidates (:72-327), which name the keyframes the loop and map-match chain then works on
 * (ccm_search_by_bow_frames, ccm_sim3_solver_*, ...).
 *
 * The reference walks an inverted file and keeps mnLoopWords / mLoopQuery / mLoopScore on the keyframes.  For a keyframe that
 * queries once -- all LoopFinder and MapMatcher do -- the outcome equals the following, which is what is implemented (DESIGN.md
 * section 4 shows the equivalence).  Every stored entry e is a BowVector (word ids strictly ascending, double values), a sequence
 * number seq[e] from a counter that grows with every add (an erased and re-added key gets a new, larger one), and a stable slot.
 * For a query BowVector q the DEVICE computes per slot
 *     words[e]       number of word ids common to q and e
 *     first_word[e]  the smallest common word id, -1 without one
 *     score[e]       L1Scoring::score(q, e) (ScoringObject.cpp:23-68) in double: s = 0; over the common ids in ascending order
 *                    s += (fabs(vi - wi) - fabs(vi)) - fabs(wi) with vi the query's value and wi the entry's; score = -s / 2.0.
 *                    The left-to-right sum is part of the definition: the value is bit-identical to ccm_bow_score_l1.
 *                    0 without a common word.
 * and every order-dependent decision is replayed on the HOST over those arrays by ccm_kfdb_shortlist and ccm_kfdb_candidates.
 *
 * The database lives on the device of the context that creates it; afterwards only queries need a context, and any context on
 * that device will do.  add / erase / clear / size / slot / slots / keys take no context, do no GPU work and may be called from any
 * thread: they copy into a host-side pending list under the database's mutex.  A query holds that mutex from its flush to the end
 * of its download, so queries from several threads (each per-client LoopFinder, the MapMatcher), each with its own context,
 * serialise.  The arena of words grows when it is full and is compacted when more than half of it is holes; both happen inside a
 * query.  Nothing is sized by the vocabulary: n_words only bounds the word ids. */
typedef struct ccm_kfdb ccm_kfdb;
#define CCM_KFDB_NEIGHBOURS 10      /* GetBestCovisibilityKeyFrames(10), Database.cpp:155 */
int  ccm_kfdb_create(ccm_ctx*, int n_words, int64_t initial_capacity_words, ccm_kfdb** out);
void ccm_kfdb_destroy(ccm_kfdb*);
/* add: CCM_E_ARG, with the database unchanged, unless the ids are strictly ascending, every id lies in [0, n_words) and the key is
 * not present; n = 0 is a legal entry.  The entry takes a free slot (a slot freed by erase may be reused).  erase of an unknown key
 * does nothing, as in the reference.  clear forgets every entry and every slot. */
int ccm_kfdb_add(ccm_kfdb*, int64_t key, int n, const int32_t* ids, const double* vals);
int ccm_kfdb_erase(ccm_kfdb*, int64_t key);
int ccm_kfdb_clear(ccm_kfdb*);
int ccm_kfdb_size(ccm_kfdb*);                  /* stored entries */
int ccm_kfdb_slot(ccm_kfdb*, int64_t key);     /* the key's slot, -1 when it is not stored */
int ccm_kfdb_slots(ccm_kfdb*);                 /* high-water mark of the slots = length of the query arrays */
/* keys[s] = the key in slot s, -1 for a free slot; seq[s] (may be null) = its sequence number, -1 for a free slot.  Returns the
 * number of slots, CCM_E_CAPACITY when that exceeds capacity. */
int ccm_kfdb_keys(ccm_kfdb*, int capacity, int64_t* keys, int64_t* seq);
/* The query: applies the pending adds and erases on the context's stream, runs one kernel launch over every slot, downloads and
 * synchronises.  The outputs have room for `capacity` slots; returns the number of slots written (ccm_kfdb_slots at the time of
 * the query) or CCM_E_CAPACITY.  Free slots give words 0, first_word -1, score 0, seq -1; the query's own slot is reported like
 * any other.  CCM_E_ARG for a context on another device, an unknown query_key, or (second form, for a Frame that is not stored) a
 * query vector that fails the checks of add. */
int ccm_kfdb_query(ccm_ctx*, ccm_kfdb*, int64_t query_key, int capacity, int32_t* words, double* score, int32_t* first_word, int64_t* seq);
int ccm_kfdb_query_vector(ccm_ctx*, ccm_kfdb*, int n, const int32_t* ids, const double* vals, int capacity, int32_t* words,
                          double* score, int32_t* first_word, int64_t* seq);
/* Query words the kernel stages in LDS; a longer query is searched in global memory (same results). */
int ccm_kfdb_query_lds_words(void);
/* Taps: the arena in words (allocated, tail, held by live entries) after the last flush; milliseconds the last query spent in
 * its flush, its kernel and its download (HIP events on the querying context's stream). */
int ccm_kfdb_arena(ccm_kfdb*, int64_t* capacity_words, int64_t* used_words, int64_t* live_words);
int ccm_kfdb_last_timing(ccm_kfdb*, double ms3[3]);

/* Host step A (lKFsSharingWords and lScoreAndMatch, :111-146 / :236-271); needs no device.  eligible[s]: loop query -- the entry is
 * in the query's map and is not connected to the query; map-match query -- the entry's client is not in msuAssClients.  A free slot
 * (seq < 0) and query_slot (-1 for a query that is not stored) are ineligible whatever their byte says.  An entry is LISTED when it
 * is eligible and words > 0; listed entries are ordered by (first_word, seq) ascending, the walk's first-encounter order.
 * maxCommonWords = the largest words of a listed entry, *min_common_words = (int)(maxCommonWords * 0.8f); an entry passes the gate
 * when words > *min_common_words.  shortlist = the gated entries with (float)score >= min_score, in listed order.  Returns its
 * length (CCM_E_CAPACITY beyond capacity); nothing listed or nothing shortlisted gives 0 and *min_common_words = 0. */
int ccm_kfdb_shortlist(int n_slots, const int32_t* words, const double* score, const int32_t* first_word, const int64_t* seq,
                       const uint8_t* eligible, int query_slot, float min_score, int capacity, int32_t* shortlist, int32_t* min_common_words);
/* Host step B (the covisibility accumulation, :148-201 / :273-326), all in float as there.  neighbours[i * CCM_KFDB_NEIGHBOURS + k]:
 * the slots of GetBestCovisibilityKeyFrames(10) of shortlist[i] in its order, -1 for none or for a keyframe that is not stored.
 * Per shortlisted entry acc = best = (float)score and bestKF = the entry; each neighbour that is listed and gated adds its
 * (float)score to acc and replaces bestKF when its score is strictly greater than best.  retain = 0.75f * max(min_score, every
 * acc).  candidates (room for n_shortlist) = the bestKF of the entries with acc > retain, in shortlist order, each once.  Returns
 * their number. */
int ccm_kfdb_candidates(int n_slots, const int32_t* words, const double* score, const int64_t* seq, const uint8_t* eligible, int query_slot,
                        float min_score, int min_common_words, int n_shortlist, const int32_t* shortlist, const int32_t* neighbours,
                        int32_t* candidates);
/* DetectRelocalizationCandidates(Frame&) (:329-439) over the arrays of one ccm_kfdb_query_vector call, on the host; needs no device.
 * Step A is ccm_kfdb_shortlist itself with every slot eligible, query_slot = -1 and min_score = -INFINITY: the walk (:337-352) lists
 * every entry with words > 0 in (first_word, seq) order, minCommonWords = (int)(maxCommonWords * 0.8f) (:365) and the gate is the
 * strict words > minCommonWords (:376); there is no score test.
 * Step B, this call (:372-436), all in float as there.  mRelocScore lives on the keyframe and survives from one query to the next:
 * it is the caller's reloc_score [n_slots], in and out.  First every shortlisted entry stores (float)score there (:380).  Then, per
 * shortlisted entry in order, acc = best = (float)score and bestKF = the entry; a neighbour (neighbours[i * CCM_KFDB_NEIGHBOURS + k]
 * as for ccm_kfdb_candidates, -1 or a free slot skipped) counts when it is listed, i.e. words > 0 -- mRelocQuery == F.mId (:403) --
 * whether or not it passed the gate; a counting neighbour adds reloc_score[nb], which is the value an EARLIER query left there when
 * this query did not gate it, and replaces bestKF when that value is strictly greater than best.  bestAccScore starts at 0 (:389,
 * not at a min_score); retain = 0.75f * bestAccScore; candidates (room for n_shortlist) = the bestKF of the entries with acc >
 * retain, in shortlist order, each once.  Returns their number; n_shortlist = 0 gives 0 and touches nothing; a shortlist entry
 * outside [0, n_slots) is CCM_E_ARG with reloc_score untouched.
 * One deviation: the reference never initialises mRelocScore (src/KeyFrame.cpp:56), so a listed neighbour that no query has gated
 * reads an indeterminate value there; here it reads what the caller put into the array.  The Python KeyFrameDatabase and the shim
 * put 0 there when a slot is taken by add (a reused slot included). */
int ccm_kfdb_reloc_candidates(int n_slots, const int32_t* words, const double* score, const int64_t* seq, int n_shortlist,
                              const int32_t* shortlist, const int32_t* neighbours, float* reloc_score, int32_t* candidates);
/* minScore of LoopFinder.cpp:122-139 / MapMatcher.cpp:130-147 from the arrays of the SAME query: float 1, lowered to the least
 * (float)score of the connected slots; -1 and free slots are skipped (pass the keyframes that are not bad). */
float ccm_kfdb_min_score(int n_slots, const double* score, const int64_t* seq, int n_connected, const int32_t* connected);

/* ------------------------------------------------------------------ Covisibility
 * The covisibility counts of a map, for ALL of its keyframes: the counter of KeyFrame::UpdateConnections (cslam/src/KeyFrame.cpp:629-711,
 * called for every new keyframe, src/Mapping.cpp:272, :546, for every connected keyframe after a loop closure, src/LoopFinder.cpp:514,
 * :612, :655, and after a map merge, src/MapMerger.cpp:267, :392, :487) and the observer counts of LocalMapping::KeyFrameCullingV3
 * (src/Mapping.cpp:771-863).  Keyframe handles cannot serve: the counts run against every keyframe of the map, so the index keeps one
 * light RECORD per keyframe, as the KeyFrameDatabase keeps one BowVector:
 *     key        int64, the caller's name of the keyframe
 *     slot[n]    int32 per feature: the map-point table slot the feature holds (mp_id of the handles)
 *     octave[n]  uint8 per feature: mvKeysUn[i].octave
 * An entry HOLDS A POINT iff 0 <= slot < INT32_MAX.  Negative: no map point.  INT32_MAX: a point that has no table slot yet; it
 * never matches anything, not even another INT32_MAX.
 *
 * The counts are derived from "which keyframe holds which slot", not from MapPoint::mObservations.  They equal the reference's
 * wherever  pMP->mObservations contains (pKF, idx)  iff  pKF->mvpMapPoints[idx] == pMP  ("Covisibility
 * index"); the server keeps that invariant, a client's mObservationsLock can break it (src/MapPoint.cpp), so the index is for server
 * paths.
 *
 * Storage and threads as for the KeyFrameDatabase: one device arena of 5 bytes a feature, a stable slot number and a sequence number
 * per record; put / erase / clear / size / slot / slots / keys take no context, do no GPU work and may be called from any thread
 * (a host-side pending list under the index's mutex).  A query holds that mutex from its flush to the end of its download, so queries
 * from several threads, each with its own context on the index's device, serialise.  The arena grows when it is full and is
 * compacted when more than half of it is holes; both happen inside a query. */
typedef struct ccm_covis ccm_covis;
enum { CCM_COVIS_WEIGHTS = 1,       /* weights[q][s]: KFcounter of UpdateConnections */
       CCM_COVIS_REDUNDANCY = 2 };  /* n_redundant[q]: nRedundantObservations of KeyFrameCullingV3 */
/* The index lives on the context's device.  The context may be NULL: the index then belongs to the device of the first context
 * that queries it (bookkeeping needs no device at all).  initial_capacity_features >= 0 sizes the first arena. */
int  ccm_covis_create(ccm_ctx*, int64_t initial_capacity_features, ccm_covis** out);
void ccm_covis_destroy(ccm_covis*);
/* put: stores a record (n = 0 is legal; n < 0 or a NULL array with n > 0: CCM_E_ARG, the index unchanged).  For a key that is present
 * it REPLACES the contents and keeps the record's slot number and sequence number: what the caller does whenever the keyframe's map
 * points change.  A new key takes a free slot (one freed by erase may be reused) and the next sequence number.  erase of an unknown
 * key does nothing; the caller erases a keyframe when it turns bad, which is pKFi->isBad() of src/Mapping.cpp:835.  clear forgets
 * every record and every slot. */
int ccm_covis_put(ccm_covis*, int64_t key, int n, const int32_t* slot, const uint8_t* octave);
int ccm_covis_erase(ccm_covis*, int64_t key);
int ccm_covis_clear(ccm_covis*);
int ccm_covis_size(ccm_covis*);                /* stored records */
int ccm_covis_slot(ccm_covis*, int64_t key);   /* the key's slot number, -1 when it is not stored */
int ccm_covis_slots(ccm_covis*);               /* high-water mark of the slot numbers = length of a query's rows */
/* keys[s] = the key in slot s, -1 for a free slot; seq[s] (may be null) = its sequence number, -1 for a free slot.  Returns the
 * number of slots, CCM_E_CAPACITY when that exceeds capacity. */
int ccm_covis_keys(ccm_covis*, int capacity, int64_t* keys, int64_t* seq);
/* The query, for n_q stored keyframes at once: applies the pending changes on the context's stream, computes, downloads once and
 * synchronises.  table: a map-point table or view of the calling context, or NULL; it supplies MapPoint::isBad() (src/KeyFrame.cpp:651,
 * src/Mapping.cpp:823).  An entry of a query record COUNTS iff it holds a point and, with a table, its slot is below the table's
 * capacity and the row is CCM_MP_LIVE and not CCM_MP_BAD; with table == NULL every entry that holds a point counts.  The entries of
 * the OTHER records are not filtered: an entry that matches a counting entry names the same row.
 *   skipped[q]      entries of query q that hold a point but do not count.  An output, not an error: stale ids in old keyframes
 *                   are normal.
 *   CCM_COVIS_WEIGHTS:  weights[q * capacity + s], for every slot number s below the returned count = the number of pairs (counting
 *                   entry i of the query, entry j of record s) with equal slots: KFcounter of src/KeyFrame.cpp:644-662.  A free slot
 *                   gives 0 and so does the query's own (:658).  The reference never holds a point at two features of a keyframe,
 *                   and the weight is then the number of shared points; where that is broken the pair count is the defined result.
 *   CCM_COVIS_REDUNDANCY, with th_obs (thObs = 3, src/Mapping.cpp:815; 1 .. 2^20):
 *                   n_mps[q] = the number of counting entries (nMPs, :825);
 *                   n_redundant[q] = the number of counting entries i with fine_i >= th_obs, fine_i = the number of pairs (record s
 *                   other than the query's, entry j of s) with slot_s[j] == slot_q[i] and octave_s[j] <= octave_q[i] + 1 (:831-851).
 *                   The reference's further gate Observations() > thObs (:826) is implied under the invariant above: fine_i >= 3
 *                   names three other keyframes, which with the query itself are at least four observations.
 *                   n_mps is written with either bit.
 *   seq[s]          (may be null) the sequence number per slot, -1 for a free slot.
 * capacity = the slots the rows of weights and seq have room for; returns the number of slots (ccm_covis_slots at the time of the
 * query), CCM_E_CAPACITY when that exceeds capacity.  n_q == 0 returns CCM_OK and touches nothing.
 * Errors are found on the host before any work is queued, the outputs are then untouched.  CCM_E_ARG: a NULL argument or a NULL
 * array that `what` needs, an unknown query key, a context on another device than the index, a table of another context, what == 0 or
 * with unknown bits, th_obs out of range with CCM_COVIS_REDUNDANCY.  CCM_E_STATE: a table that outlived its context.
 * What stays with the caller: the parent selection of UpdateConnections (src/KeyFrame.cpp:713-833), AddConnection /
 * UpdateBestCovisibles on the neighbours (:687, :694), and the verdict nRedundantObservations > mfRedundancyThres * nMPs
 * (src/Mapping.cpp:857) in double, as fptype is double (include/cslam/config.h). */
typedef struct {
    int32_t  th_obs;        /* in: thObs, read with CCM_COVIS_REDUNDANCY */
    int32_t* weights;       /* [n_q][capacity], needed with CCM_COVIS_WEIGHTS */
    int32_t* n_mps;         /* [n_q] or NULL */
    int32_t* n_redundant;   /* [n_q], needed with CCM_COVIS_REDUNDANCY */
    int32_t* skipped;       /* [n_q] or NULL */
    int64_t* seq;           /* [capacity] or NULL */
} ccm_covis_result;
int ccm_covis_query(ccm_ctx*, ccm_covis*, ccm_map_table* table /* or NULL */, int n_q, const int64_t* query_keys, int what, int capacity,
                    ccm_covis_result* result);
/* Features of a query record up to which its hash is held in LDS; a longer query is hashed in global scratch (same results).  The
 * environment variable CCM_COVIS_LDS_FEATURES=N, read once, lowers it (tests reach the global path with small inputs). */
int ccm_covis_lds_features(void);
/* Taps: the arena in features (allocated, tail, held by live records) after the last flush; milliseconds the last query spent in
 * its flush, its kernels and its download (HIP events on the querying context's stream). */
int ccm_covis_arena(ccm_covis*, int64_t* capacity_features, int64_t* used_features, int64_t* live_features);
int ccm_covis_last_timing(ccm_covis*, double ms3[3]);
/* The ordered lists of UpdateConnections (src/KeyFrame.cpp:664-711) from one row of weights, on the host; needs no device.  Returns 0
 * when no weight is > 0 (the reference returns early, :664, and leaves the keyframe's connections as they are).  Listed are the slots
 * with weight >= th (th = 15, :673); when none reaches th, the single slot of maximum weight, among equal maxima the FIRST in
 * iteration order (:679 compares strictly).  Output order = sort(vPairs) followed by push_front (:697-704): descending weight, among
 * equal weights DESCENDING iteration position.  The iteration position of slot s is rank[s]: the reference's std::map<kfptr,int>
 * iterates in pointer order, so the caller fixes it (as for ccm_map_table_refresh); distinct values, rank == NULL: the slot number.
 * order_slot / order_weight [capacity] (order_weight may be NULL): returns the number written, CCM_E_CAPACITY beyond capacity. */
int ccm_covis_connections(int n_slots, const int32_t* weights, const int32_t* rank /* or NULL */, int th, int capacity, int32_t* order_slot,
                          int32_t* order_weight);

#ifdef __cplusplus
}
#endif
#endif
