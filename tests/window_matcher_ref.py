"""The windowed matchers restated from the reference's C++ text: numpy and plain Python only, one sequential
loop per map point, every feature of the frame tested for every query (no CSR grid, no candidate lists of a
fixed capacity), Hamming distance by np.unpackbits.  Neither the CPU oracle (oracle/match_oracle.c) nor the
kernels (csrc/match_window.hip) are consulted, so a misreading they share shows as a disagreement with this file.

    Frame::PosInGrid / AssignFeaturesToGrid   src/Frame.cpp:103-118, 255-266
    Frame::GetFeaturesInArea                  src/Frame.cpp:200-253   (KeyFrame's: cslam/src/KeyFrame.cpp:1162-1201)
    ORBmatcher::*                             cslam/src/ORBmatcher.cpp, lines cited per function

Floats: the reference computes in `float`; every product, sum and difference below is therefore one np.float32
operation in the order written there, and a comparison against a `double` literal (0.998, 5.99, 0.0) widens
the float first, as C++ does.

`trace` (a dict, optional) collects which of the easily-misread decisions a call actually took: the tests assert
from it that a hand-built case forces what it claims to force; a list under trace["windows"] also receives every
window searched inside the grid as (x, y, r, min_level, max_level, indices).  `wrong` (a collection of names, for
tests/test_window_matcher_cases_cpu.py alone) turns the definition into one plausible mistake each:
    tie_lowest_index     equal distances go to the lowest feature index, not to the first visited
    radius_inclusive     |dx| <= r
    ratio_any_level      the ratio test regardless of bestLevel == bestLevel2
    occupy_always        `occupied` set whether or not the accepted point has observations
    clear_current_owner  the rotation histogram clears a feature only while the recording point still owns it
    grid_floor           floor instead of round in PosInGrid
    bin_ties_late        ComputeThreeMaxima with >=: of equal bins the later one ranks first
"""
import math

import numpy as np

F = np.float32
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30           # ORBmatcher.cpp:63-65
FRAME_GRID_COLS, FRAME_GRID_ROWS = 75, 48             # include/cslam/Frame.h:51-52
INT_MAX = 2147483647
CHI2_BELOW = np.nextafter(F(5.99), F(0)) if float(F(5.99)) > 5.99 else F(5.99)     # largest float not above the double 5.99
CHI2_ABOVE = np.nextafter(CHI2_BELOW, F(np.inf))                                   # its successor: the smallest float above


def _note(trace, key, n=1):
    if trace is not None and n:
        trace[key] = trace.get(key, 0) + n


def _note_max(trace, key, v):
    if trace is not None:
        trace[key] = max(trace.get(key, 0), v)


class Grid:
    """What the matchers read of a Frame / KeyFrame: undistorted keypoints, octaves, descriptors, angles, and the grid
    parameters of the Frame constructor (src/Frame.cpp:85-88: mfGridElementWidthInv = float(COLS) / float(mnMaxX - mnMinX))."""

    def __init__(self, kx, ky, octave, desc, angle=None, min_x=0.0, max_x=752.0, min_y=0.0, max_y=480.0,
                 cols=FRAME_GRID_COLS, rows=FRAME_GRID_ROWS):
        self.kx = np.ascontiguousarray(kx, F); self.ky = np.ascontiguousarray(ky, F)
        self.oct = np.ascontiguousarray(octave, np.int32)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.angle = None if angle is None else np.ascontiguousarray(angle, F)
        self.n = len(self.kx)
        self.cols, self.rows = int(cols), int(rows)
        self.min_x, self.max_x, self.min_y, self.max_y = F(min_x), F(max_x), F(min_y), F(max_y)
        self.inv_w = F(self.cols) / F(self.max_x - self.min_x)
        self.inv_h = F(self.rows) / F(self.max_y - self.min_y)
        self.bits = np.unpackbits(self.desc, axis=1)            # [n, 256]
        self.cells = {}                                         # pos_in_grid's results


def hamming(a, b) -> int:
    """ORBmatcher::DescriptorDistance (:1653-1669): the number of differing bits of two 256-bit descriptors."""
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def _round_half_away(v):
    """C's round() on an array of floats: nearest integer, halves away from zero."""
    v = np.asarray(v, np.float64)
    return np.copysign(np.floor(np.abs(v) + 0.5), v).astype(np.int64)


def pos_in_grid(g, *, wrong=()):
    """Frame::PosInGrid (src/Frame.cpp:255-266) for every feature: (posX, posY, in_grid).  posX = round((x - mnMinX) * inv_w) in
    float; a feature whose cell lies outside [0, cols) x [0, rows) is pushed into no cell (AssignFeaturesToGrid, :110-117) and so
    can never be returned by GetFeaturesInArea."""
    floor = "grid_floor" in wrong
    if floor not in g.cells:                                    # the same for every query of a frame: computed once
        fx = (g.kx - g.min_x) * g.inv_w
        fy = (g.ky - g.min_y) * g.inv_h
        if floor:
            px, py = np.floor(fx.astype(np.float64)).astype(np.int64), np.floor(fy.astype(np.float64)).astype(np.int64)
        else:
            px, py = _round_half_away(fx), _round_half_away(fy)
        g.cells[floor] = (px, py, (px >= 0) & (px < g.cols) & (py >= 0) & (py < g.rows))
    return g.cells[floor]


def features_in_area(g, x, y, r, min_level=-1, max_level=-1, *, wrong=(), trace=None):
    """Frame::GetFeaturesInArea (src/Frame.cpp:200-253): the feature indices in visiting order = cell column, then cell row, then
    feature index (cells are walked ix outer, iy inner, :223-225; a cell holds its features in index order, :110-117).
    KeyFrame::GetFeaturesInArea is the same walk without the level arguments (= -1, -1)."""
    x, y, r = F(x), F(y), F(r)
    if g.n == 0:
        return []
    min_cx = max(0, int(math.floor(F(F(F(x - g.min_x) - r) * g.inv_w))))                   # :205
    if min_cx >= g.cols:
        return []
    max_cx = min(g.cols - 1, int(math.ceil(F(F(F(x - g.min_x) + r) * g.inv_w))))           # :209
    if max_cx < 0:
        return []
    min_cy = max(0, int(math.floor(F(F(F(y - g.min_y) - r) * g.inv_h))))                   # :213
    if min_cy >= g.rows:
        return []
    max_cy = min(g.rows - 1, int(math.ceil(F(F(F(y - g.min_y) + r) * g.inv_h))))           # :217
    if max_cy < 0:
        return []
    px, py, inside = pos_in_grid(g, wrong=wrong)
    keep = inside & (px >= min_cx) & (px <= max_cx) & (py >= min_cy) & (py <= max_cy)
    if min_level > 0 or max_level >= 0:                                                   # bCheckLevels, :221, :234-241
        keep &= g.oct >= min_level
        if max_level >= 0:
            keep &= g.oct <= max_level
    adx, ady = np.abs(g.kx - x), np.abs(g.ky - y)                                          # :243-246
    if trace is not None:
        up, down = F(np.inf), F(-np.inf)                                                   # the floats next to x +- r, y +- r, on the inside
        edge = ((g.kx == np.nextafter(F(x + r), down)) | (g.kx == np.nextafter(F(x - r), up)) |
                (g.ky == np.nextafter(F(y + r), down)) | (g.ky == np.nextafter(F(y - r), up)))
        _note(trace, "at_radius_excluded", int((keep & (((adx == r) & (ady < r)) | ((ady == r) & (adx < r)))).sum()))
        _note(trace, "just_inside_radius", int((keep & (adx < r) & (ady < r) & edge).sum()))
    keep &= ((adx <= r) & (ady <= r)) if "radius_inclusive" in wrong else ((adx < r) & (ady < r))
    idx = np.nonzero(keep)[0]
    if "tie_lowest_index" not in wrong:
        idx = idx[np.lexsort((idx, py[idx], px[idx]))]
    _note_max(trace, "max_candidates", len(idx))
    if trace is not None and "windows" in trace:                                           # a caller that wants the windows themselves
        trace["windows"].append((x, y, r, int(min_level), int(max_level), [int(i) for i in idx]))
    return [int(i) for i in idx]


def _dist(g, d, idx):
    """Hamming distances of descriptor d to the features idx."""
    if len(idx) == 0:
        return []
    return [int(v) for v in (g.bits[idx] != np.unpackbits(np.asarray(d, np.uint8))[None, :]).sum(axis=1)]


def _tie(trace, idx, dist, usable, best_idx, best_dist):
    """Notes when visiting order, and not the lowest feature index, decided between candidates of equal distance."""
    if trace is not None and best_idx >= 0 and any(u and d == best_dist and i < best_idx for i, d, u in zip(idx, dist, usable)):
        _note(trace, "tie_by_order")


def three_maxima(sizes, *, wrong=(), trace=None):
    """ORBmatcher::ComputeThreeMaxima (:1607-1648) on the bin sizes: (ind1, ind2, ind3)."""
    late = "bin_ties_late" in wrong
    gt = (lambda a, b: a >= b and a > 0) if late else (lambda a, b: a > b)
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if gt(s, max1):
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif gt(s, max2):
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif gt(s, max3):
            max3, ind3 = s, i
    if trace is not None and max1 > 0:
        tenth = F(F(0.1) * F(max1))
        if max2 == max1:
            _note(trace, "bins_tied_12")
        if max3 > 0 and any(s == max3 for i, s in enumerate(sizes) if i not in (ind1, ind2, ind3)):
            _note(trace, "bins_tied_34")
        if max2 > 0 and F(max2) == tenth:
            _note(trace, "second_at_tenth")
        if max2 > 0 and F(max2) < tenth:
            _note(trace, "second_below_tenth")
    if F(max2) < F(F(0.1) * F(max1)):                     # :1639
        ind2 = ind3 = -1
    elif F(max3) < F(F(0.1) * F(max1)):                   # :1644
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(a1, a2):
    """:1439-1444 (and :518-523): rot = a1 - a2 in float, + 360 when negative, bin = round(rot * (1.0f / HISTO_LENGTH)), 30 -> 0."""
    rot = F(F(a1) - F(a2))
    if float(rot) < 0.0:
        rot = F(rot + F(360.0))
    b = int(_round_half_away(F(rot * F(F(1.0) / F(HISTO_LENGTH)))))
    return 0 if b == HISTO_LENGTH else b


def search_by_projection(g, scale_factors, in_view, level, view_cos, proj_x, proj_y, mp_desc, has_obs, occupied, th, nnratio,
                         *, wrong=(), trace=None):
    """ORBmatcher::SearchByProjection(Frame&, vpMapPoints, th) (:71-148).  occupied[idx] = the feature holds a map point with
    Observations() > 0 (:113-115); has_obs[m] = map point m has observations.  match[idx] = the last point written into
    F.mvpMapPoints[idx] (:142), which makes the feature occupied only when that point has observations.
    Returns (nmatches, match, occupied)."""
    sf = np.asarray(scale_factors, F)
    occ = np.array(occupied, bool)
    match = np.full(g.n, -1, np.int32)
    occ0 = occ.copy()
    rejected = set()
    nmatches = 0
    b_factor = float(F(th)) != 1.0                                                        # :75
    for m in range(len(in_view)):
        if not in_view[m]:                                                                # :80-84
            continue
        lvl = int(level[m])
        r = F(2.5) if float(F(view_cos[m])) > 0.998 else F(4.0)                           # RadiusByViewingCos :150-156
        if b_factor:
            r = F(r * F(th))                                                              # :91-92
        idx = features_in_area(g, proj_x[m], proj_y[m], F(r * sf[lvl]), lvl - 1, lvl, wrong=wrong, trace=trace)   # :94-95
        if not idx:
            continue
        dist = _dist(g, mp_desc[m], idx)

        def scan(flags):
            best, best_l, best2, best_l2, best_i = 256, -1, 256, -1, -1                   # :102-106
            for i, d in zip(idx, dist):
                if flags[i]:                                                              # :113-115
                    continue
                if d < best:                                                              # :121-128
                    best2, best, best_l2, best_l, best_i = best, d, best_l, int(g.oct[i]), i
                elif d < best2:                                                           # :129-133
                    best_l2, best2 = int(g.oct[i]), d
            return best, best_l, best2, best_l2, best_i

        def decide(s):
            best, best_l, best2, best_l2, best_i = s
            if best > TH_HIGH:                                                            # :137
                return "far"
            same = best_l == best_l2 or "ratio_any_level" in wrong
            if same and F(best) > F(F(nnratio) * F(best2)):                               # :139
                return "ratio"
            return "take"

        s = scan(occ)
        best, best_l, best2, best_l2, best_i = s
        verdict = decide(s)
        if trace is not None:
            _tie(trace, idx, dist, [not occ[i] for i in idx], best_i, best)
            if any(occ[i] and not occ0[i] for i in idx):
                _note(trace, "candidate_taken_earlier")
                if decide(scan(occ0)) != verdict:
                    _note(trace, "verdict_changed_by_earlier")
            if best == TH_HIGH:
                _note(trace, "best_eq_th")
            if best == TH_HIGH + 1:
                _note(trace, "best_eq_th_plus_1")
            if best <= TH_HIGH and F(best) == F(F(nnratio) * F(best2)) and best_l == best_l2:
                _note(trace, "ratio_equal_kept")
            if best <= TH_HIGH and best_l != best_l2 and F(best) > F(F(nnratio) * F(best2)):
                _note(trace, "ratio_skipped_by_level")
        if verdict == "far":
            continue
        if verdict == "ratio":
            _note(trace, "ratio_rejected")
            rejected.add(best_i)
            continue
        if trace is not None:
            if match[best_i] >= 0:
                _note(trace, "overwrite")
            if best_i in rejected:
                _note(trace, "rejected_feature_taken_later")
        match[best_i] = m                                                                 # :142
        occ[best_i] = True if "occupy_always" in wrong else bool(has_obs[m])
        nmatches += 1
    return nmatches, match, occ.astype(np.uint8)


def search_by_projection_sim3(g, scale_factors, valid, u, v, level, mp_desc, observed, matched, th, *, wrong=(), trace=None):
    """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:308-446) after the projection (valid, u, v, level).
    The level filter sits inside the candidate loop (:396-399), the threshold is TH_LOW (:412).  observed[m] = the point is
    already an observation of pKF: it still chooses a feature (re-mapped by the caller, :414-434) but neither sets vpMatched
    nor counts (:436-441).  Returns (nmatches, best_idx per point, matched)."""
    sf = np.asarray(scale_factors, F)
    mt = np.array(matched, bool)
    mt0 = mt.copy()
    best_idx = np.full(len(valid), -1, np.int32)
    chosen_by_observed = set()
    nmatches = 0
    for m in range(len(valid)):
        if not valid[m]:
            continue
        lvl = int(level[m])
        idx = features_in_area(g, u[m], v[m], F(F(th) * sf[lvl]), wrong=wrong, trace=trace)            # :378-380
        if not idx:
            continue
        dist = _dist(g, mp_desc[m], idx)
        best, best_i = 256, -1                                                            # :388-389
        usable = []
        for i, d in zip(idx, dist):
            ok = not mt[i] and not (g.oct[i] < lvl - 1 or g.oct[i] > lvl)                 # :393-399
            usable.append(ok)
            if ok and d < best:                                                           # :405-409
                best, best_i = d, i
        if trace is not None:
            _tie(trace, idx, dist, usable, best_i, best)
            if any(mt[i] and not mt0[i] for i in idx):
                _note(trace, "candidate_taken_earlier")
            if best == TH_LOW:
                _note(trace, "best_eq_th")
            if best == TH_LOW + 1:
                _note(trace, "best_eq_th_plus_1")
        if best <= TH_LOW:                                                                # :412
            best_idx[m] = best_i
            if observed[m]:
                _note(trace, "observed_chose")
                chosen_by_observed.add(best_i)
            else:
                if best_i in chosen_by_observed:
                    _note(trace, "taken_after_observed_chose")
                mt[best_i] = True                                                         # :439-440
                nmatches += 1
    return nmatches, best_idx, mt.astype(np.uint8)


def search_by_projection_frame(g, scale_factors, valid, u, v, last_octave, last_angle, mp_desc, has_obs, occupied, th, check_ori,
                               orb_dist=TH_HIGH, *, wrong=(), trace=None):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (:1350-1476) after the projection; with has_obs all ones and
    orb_dist = ORBdist also SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1478-1605).  g.angle = the current
    frame's keypoint angles.  The rotation histogram records the FEATURE index at acceptance time (:1446) and the clearing pass
    sets that feature to null and decrements once per recorded entry (:1462-1471), whoever owns the feature by then.
    Returns (nmatches, match, occupied as the point loop left it)."""
    sf = np.asarray(scale_factors, F)
    occ = np.array(occupied, bool)
    occ0 = occ.copy()
    match = np.full(g.n, -1, np.int32)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]                                          # entries (feature, recording point)
    nmatches = 0
    for i in range(len(valid)):
        if not valid[i]:
            continue
        lo = int(last_octave[i])
        idx = features_in_area(g, u[i], v[i], F(F(th) * sf[lo]), lo - 1, lo + 1, wrong=wrong, trace=trace)   # :1400-1404
        if not idx:
            continue
        dist = _dist(g, mp_desc[i], idx)
        best, best_i = 256, -1                                                            # :1411-1412
        for i2, d in zip(idx, dist):
            if occ[i2]:                                                                   # :1417-1419
                continue
            if d < best:                                                                  # :1425-1429
                best, best_i = d, i2
        if trace is not None:
            _tie(trace, idx, dist, [not occ[k] for k in idx], best_i, best)
            if any(occ[k] and not occ0[k] for k in idx):
                _note(trace, "candidate_taken_earlier")
            if best == orb_dist:
                _note(trace, "best_eq_th")
            if best == orb_dist + 1:
                _note(trace, "best_eq_th_plus_1")
        if best <= orb_dist:                                                              # :1432 / :1561
            if match[best_i] >= 0:
                _note(trace, "overwrite")
            match[best_i] = i                                                             # :1434
            occ[best_i] = True if "occupy_always" in wrong else bool(has_obs[i])
            nmatches += 1
            if check_ori:
                rot_hist[rot_bin(last_angle[i], g.angle[best_i])].append((best_i, i))     # :1437-1447
    if check_ori:
        ind = three_maxima([len(b) for b in rot_hist], wrong=wrong, trace=trace)          # :1460
        for b in range(HISTO_LENGTH):
            if b in ind:
                continue
            for feat, point in rot_hist[b]:                                               # :1466-1470
                if match[feat] != point:
                    _note(trace, "stale_clear")
                    if "clear_current_owner" in wrong:
                        continue
                match[feat] = -1
                nmatches -= 1
    return nmatches, match, occ.astype(np.uint8)


def fuse_select(g, scale_factors, inv_level_sigma2, valid, u, v, level, mp_desc, th, chi2_check, accept_th=TH_LOW,
                *, wrong=(), trace=None):
    """The selection loops of ORBmatcher::Fuse: (:920-962) with the chi2 test, (:1071-1101) without; with accept_th = TH_HIGH the
    two passes of SearchBySim3 (:1211-1246, :1291-1326).  Per point the first of the nearest features (strict `dist < bestDist`
    in visiting order) of level [l-1, l], optionally with e2 * invSigma2 <= 5.99 on the float product (:946-951).
    Returns (best_idx or -1 unless best_dist <= accept_th, best_dist or 256)."""
    sf = np.asarray(scale_factors, F)
    n_mp = len(valid)
    best_idx = np.full(n_mp, -1, np.int32); best_dist = np.full(n_mp, 256, np.int32)
    for m in range(n_mp):
        if not valid[m]:
            continue
        lvl = int(level[m])
        idx = features_in_area(g, u[m], v[m], F(F(th) * sf[lvl]), wrong=wrong, trace=trace)            # :920-922
        dist = _dist(g, mp_desc[m], idx)
        best, best_i = 256, -1       # :931 (INT_MAX at :1082: a distance never exceeds 256, and 256 is above every accept_th)
        usable = []
        for i, d in zip(idx, dist):
            kl = int(g.oct[i])
            ok = not (kl < lvl - 1 or kl > lvl)                                           # :941
            if ok and chi2_check:
                ex = F(F(u[m]) - g.kx[i]); ey = F(F(v[m]) - g.ky[i])                      # :946-948
                e2 = F(F(ex * ex) + F(ey * ey))
                c = F(e2 * F(inv_level_sigma2[kl]))
                if trace is not None and c == CHI2_BELOW:
                    _note(trace, "chi2_adjacent_kept")
                if trace is not None and c == CHI2_ABOVE:
                    _note(trace, "chi2_adjacent_rejected")
                if float(c) > 5.99:                                                       # :950
                    ok = False
            usable.append(ok)
            if ok and d < best:                                                           # :957-961
                best, best_i = d, i
        if trace is not None:
            _tie(trace, idx, dist, usable, best_i, best)
            if best == accept_th:
                _note(trace, "best_eq_th")
            if best == accept_th + 1:
                _note(trace, "best_eq_th_plus_1")
        best_dist[m] = best
        if best <= accept_th:                                                             # :965 / :1104 / :1243
            best_idx[m] = best_i
    return best_idx, best_dist


def search_by_sim3(g1, sf1, g2, sf2, valid1, u1, v1, level1, mp_desc1, valid2, u2, v2, level2, mp_desc2, th, *, wrong=(), trace=None):
    """ORBmatcher::SearchBySim3 (:1124-1348) after the projections: the points of KF1 pick in KF2 and the reverse (<= TH_HIGH,
    :1243, :1323), a pair stays when the two directions agree (:1330-1345).  Returns (nFound, match12)."""
    m1, _ = fuse_select(g2, sf2, None, valid1, u1, v1, level1, mp_desc1, th, False, TH_HIGH, wrong=wrong, trace=trace)
    m2, _ = fuse_select(g1, sf1, None, valid2, u2, v2, level2, mp_desc2, th, False, TH_HIGH, wrong=wrong, trace=trace)
    match12 = np.full(g1.n, -1, np.int32)
    found = 0
    for i1 in range(g1.n):
        i2 = int(m1[i1])
        if i2 >= 0:
            if int(m2[i2]) == i1:
                match12[i1] = i2
                found += 1
            else:
                _note(trace, "directions_disagree")
    return found, match12


def search_for_initialization(oct1, desc1, angle1, g2, prev_matched, window, nnratio, check_ori, *, wrong=(), trace=None):
    """ORBmatcher::SearchForInitialization (:448-563).  g2.angle = F2's keypoint angles; prev_matched [n1, 2] = vbPrevMatched.
    Level-0 features of F1 only (:464-466), window levels [0, 0] (:468), vMatchedDistance keeps a feature for the nearer claimant
    (:487), the ratio compares int with (float)bestDist2 * mfNNratio (:504), a re-taken feature un-matches its previous owner
    (:506-510), the histogram records i1 and clears only what is still matched (:546-551), matched features update
    prev_matched (:558-560).  Returns (nmatches, matches12, prev_matched)."""
    n1 = len(oct1)
    pm = np.array(prev_matched, F).reshape(n1, 2)
    m12 = np.full(n1, -1, np.int32)
    matched_dist = [INT_MAX] * g2.n                                                       # :458
    m21 = [-1] * g2.n                                                                     # :459
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i1 in range(n1):
        level1 = int(oct1[i1])
        if level1 > 0:
            continue
        idx = features_in_area(g2, pm[i1, 0], pm[i1, 1], F(window), level1, level1, wrong=wrong, trace=trace)
        if not idx:
            continue
        dist = _dist(g2, desc1[i1], idx)
        best, best2, best_i = INT_MAX, INT_MAX, -1                                        # :475-477
        for i2, d in zip(idx, dist):
            if matched_dist[i2] <= d:                                                     # :487
                if matched_dist[i2] != INT_MAX:
                    _note(trace, "kept_by_nearer_claimant")
                continue
            if d < best:                                                                  # :490-495
                best2, best, best_i = best, d, i2
            elif d < best2:                                                               # :496-499
                best2 = d
        if trace is not None:
            _tie(trace, idx, dist, [matched_dist[k] > d for k, d in zip(idx, dist)], best_i, best)
            if best == TH_LOW:
                _note(trace, "best_eq_th")
            if best == TH_LOW + 1:
                _note(trace, "best_eq_th_plus_1")
            if best <= TH_LOW and F(best) == F(F(best2) * F(nnratio)):
                _note(trace, "ratio_equal_rejected")
        if best <= TH_LOW:                                                                # :502
            if F(best) < F(F(best2) * F(nnratio)):                                        # :504
                if m21[best_i] >= 0:                                                      # :506-510
                    _note(trace, "previous_owner_unmatched")
                    m12[m21[best_i]] = -1
                    nmatches -= 1
                m12[i1] = best_i; m21[best_i] = i1; matched_dist[best_i] = best           # :511-513
                nmatches += 1
                if check_ori:
                    rot_hist[rot_bin(angle1[i1], g2.angle[best_i])].append(i1)            # :516-526
            else:
                _note(trace, "ratio_rejected")
    if check_ori:
        ind = three_maxima([len(b) for b in rot_hist], wrong=wrong, trace=trace)          # :538
        for b in range(HISTO_LENGTH):
            if b in ind:
                continue
            for i1 in rot_hist[b]:
                if m12[i1] >= 0:                                                          # :547-551
                    m12[i1] = -1
                    nmatches -= 1
                else:
                    _note(trace, "histogram_entry_already_unmatched")
    for i1 in range(n1):                                                                  # :558-560
        if m12[i1] >= 0:
            pm[i1, 0] = g2.kx[m12[i1]]; pm[i1, 1] = g2.ky[m12[i1]]
    return nmatches, m12, pm
