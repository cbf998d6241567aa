"""Everything that walks the vocabulary tree or a FeatureVector, restated from the reference's C++ text: numpy and plain Python only,
one sequential loop per feature, Hamming distance by np.unpackbits.  Neither the CPU oracle (oracle/bow_oracle.c, oracle/match_oracle.c)
nor the kernels (csrc/bow_kernels.hip, csrc/match_bow.hip, csrc/map_kernels.hip) are consulted, so a misreading they share shows as a
disagreement with this file.

    TemplatedVocabulary::transform (one feature)      cslam/thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1217-1258
    TemplatedVocabulary::transform (BowVector)        TemplatedVocabulary.h:1125-1193, BowVector.cpp:34-84
    L1Scoring::score                                  ScoringObject.cpp:23-68
    MapPoint::ComputeDistinctiveDescriptors           cslam/src/MapPoint.cpp:957-988
    ORBmatcher::CheckDistEpipolarLine                 cslam/src/ORBmatcher.cpp:159-176
    ORBmatcher::SearchByBoW (KeyFrame, Frame)         ORBmatcher.cpp:178-306
    ORBmatcher::SearchByBoW (KeyFrame, KeyFrame)      ORBmatcher.cpp:565-698
    ORBmatcher::SearchForTriangulation                ORBmatcher.cpp:700-852

Floats: where the reference computes in `float`, every product, sum, difference and quotient below is one np.float32 operation in the
order written there; a comparison against a `double` (0.0, 3.84 * sigma2) widens the float first, as C++ does.  BowVector values are
`double`; their sums are sequential Python float additions in the order the reference visits them, never np.sum.

A FeatureVector is given as one node id per feature (a negative id: the feature is in no entry).  DBoW2 appends features to an entry
in feature order (FeatureVector.cpp, addFeature) and std::map walks entries by ascending node id, which is all the matchers use.

`trace` (a dict, optional) counts the easily-misread decisions a call actually took; the tests assert from it that a hand-built case
forces what it claims to force.  `wrong` (a collection of names, for tests/test_bow_cases_cpu.py alone) turns the definition into one
plausible mistake each:
    child_tie_last           of equally near children the last one wins (<=)
    nid_level_off_by_one     the FeatureVector node is taken one level nearer the root
    words_in_leaf_walk_order words numbered in the order a depth-first walk meets the leaves, not in node order
    stopped_kept             a word counts when w >= 0
    sum_pairwise             np.sum (pairwise) where the reference adds sequentially
    median_upper             the sorted row read at N / 2
    median_tie_last          of equal medians the last row wins (<=)
    second_distinct          the second best must differ from the best: duplicates of the best do not count
    th_inclusive_both        best <= TH_LOW in both SearchByBoW overloads
    th_strict_both           best < TH_LOW in both
    ratio_in_double          the ratio product in double
    taken_counts_for_second  a candidate that is already matched still counts towards the second best
    valid2_counts_for_second a candidate without a (good) map point still counts towards the second best
    negative_nodes_match     features without a node form an entry of their own
    bin_round_half_even      the rotation bin rounded half to even
    bin_ties_late            ComputeThreeMaxima with >=
    tri_tie_first            SearchForTriangulation keeps the first of equally near candidates
    tri_th_strict            SearchForTriangulation needs dist < TH_LOW
    epipole_inclusive        a candidate exactly 100 * scale from the epipole is dropped too
"""
import numpy as np

from window_matcher_ref import rot_bin, three_maxima

F = np.float32
TH_LOW, HISTO_LENGTH = 50, 30                              # ORBmatcher.cpp:64-65
TF_IDF, TF, IDF, BINARY = range(4)                         # BowVector.h:36-42
L1_NORM, L2_NORM, DOT_PRODUCT = 0, 1, 5                    # BowVector.h:54-62


def _note(trace, key, n=1):
    if trace is not None and n:
        trace[key] = trace.get(key, 0) + n


def bits(desc):
    return np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1)


# ------------------------------------------------------------------------------------------------------------ the vocabulary
class Vocabulary:
    """m_nodes as loadFromTextFile leaves them (TemplatedVocabulary.h:1385-1414): node i hangs under parent[i] < i, a node's children are
    in the order they were appended, and a leaf gets word id m_words.size() at the moment it is read: words are the leaves numbered in
    node order.  Node 0 is the root and never a word."""

    def __init__(self, k, L, parent, desc, weight, *, wrong=()):
        self.k, self.L = int(k), int(L)
        self.parent = [int(p) for p in parent]
        n = len(self.parent)
        assert all(0 <= self.parent[i] < i for i in range(1, n))
        self.bits = bits(desc)
        self.weight = np.ascontiguousarray(weight, np.float64)
        self.children = [[] for _ in range(n)]
        for i in range(1, n):
            self.children[self.parent[i]].append(i)
        self.word = [-1] * n
        leaves = [i for i in range(1, n) if not self.children[i]]
        if "words_in_leaf_walk_order" in wrong:
            leaves, stack = [], [0]
            while stack:
                i = stack.pop()
                if i and not self.children[i]:
                    leaves.append(i)
                stack.extend(reversed(self.children[i]))
        for w, i in enumerate(leaves):
            self.word[i] = w
        self.n_words = len(leaves)

    def transform_feature(self, feature, levelsup, *, wrong=(), trace=None):
        """:1217-1258 -> (word_id, weight, nid).  nid = 0 when L - levelsup <= 0 (:1227).  When the descent reaches a leaf above
        nid_level the reference never assigns *nid; the project returns 0 there (its choice, stated here, not the reference's)."""
        fb = np.unpackbits(np.asarray(feature, np.uint8))
        nid_level = self.L - int(levelsup)                                             # :1226
        if "nid_level_off_by_one" in wrong:
            nid_level -= 1
        nid = 0
        final, level = 0, 0
        while True:                                                                    # :1232-1254
            level += 1
            nodes = self.children[final]
            d = (self.bits[nodes] != fb[None, :]).sum(axis=1)
            best_j = 0
            for j in range(1, len(nodes)):                                             # :1240-1249
                if d[j] < d[best_j] or ("child_tie_last" in wrong and d[j] == d[best_j]):
                    best_j = j
            if trace is not None:
                ties = int((d == d[best_j]).sum())
                if ties > 1:
                    _note(trace, "child_tie")
                    if ties == len(nodes):
                        _note(trace, "child_tie_all")
                    _note(trace, "child_tie_level_%d" % level)
                _note(trace, "child_dist_0", int(d[best_j] == 0))
                _note(trace, "child_dist_256", int((d == 256).any()))
                if len(nodes) > self.k:
                    _note(trace, "more_than_k_children")
            final = nodes[best_j]
            if level == nid_level:                                                     # :1251-1252
                nid = final
            if not self.children[final]:
                break
        if trace is not None and nid_level > level:
            _note(trace, "leaf_above_nid_level")
        return self.word[final], float(self.weight[final]), nid                        # :1257-1258

    def transform_features(self, feats, levelsup, *, wrong=(), trace=None):
        f = np.ascontiguousarray(feats, np.uint8).reshape(-1, 32)
        out = [self.transform_feature(x, levelsup, wrong=wrong, trace=trace) for x in f]
        return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.float64), np.array([o[2] for o in out], np.int32))


def bow_vector(word_id, weight, node_id, weighting=TF_IDF, scoring=L1_NORM, *, wrong=(), trace=None):
    """:1125-1193 after the per-feature transform: -> (ids ascending, values, fv_node per feature; -1 where !(w > 0)).  `weight` is what
    the node holds (the idf, or 1 for TF and BINARY: setNodeWeights made it so); TF_IDF and TF add it per hit in feature order
    (addWeight, BowVector.cpp:34-46), IDF and BINARY keep the first (addIfNotExist, :50-58).  Every scoring but DOT_PRODUCT
    normalises (L1: sum of |v|, L2: sqrt of the sum of squares, both in key order, :62-84); without it TF_IDF and TF divide by the
    number of distinct words (:1164-1170)."""
    pairwise = "sum_pairwise" in wrong
    hits = {}
    fv = np.full(len(word_id), -1, np.int32)
    for i in range(len(word_id)):
        w = float(weight[i])
        if not (w >= 0 if "stopped_kept" in wrong else w > 0):                         # :1157
            _note(trace, "stopped")
            continue
        hits.setdefault(int(word_id[i]), []).append(w)
        fv[i] = int(node_id[i])
    tf = weighting in (TF_IDF, TF)
    v = {}
    for wid, ws in hits.items():
        if not tf:
            v[wid] = ws[0]
        elif pairwise:
            v[wid] = float(np.sum(np.array(ws, np.float64)))
        else:
            acc = ws[0]
            for w in ws[1:]:
                acc = acc + w
            v[wid] = acc
        if trace is not None:
            trace["max_hits"] = max(trace.get("max_hits", 0), len(ws))
    ids = sorted(v)
    must = scoring != DOT_PRODUCT
    if tf and ids and not must:                                                        # :1164-1170
        nd = float(len(ids))
        for wid in ids:
            v[wid] = v[wid] / nd
    if must:                                                                           # BowVector.cpp:62-84
        terms = [abs(v[wid]) if scoring != L2_NORM else v[wid] * v[wid] for wid in ids]
        if pairwise:
            norm = float(np.sum(np.array(terms, np.float64))) if terms else 0.0
        else:
            norm = 0.0
            for t in terms:
                norm = norm + t
        if scoring == L2_NORM:
            norm = float(np.sqrt(np.float64(norm)))
        if norm > 0.0:
            for wid in ids:
                v[wid] = v[wid] / norm
    return np.array(ids, np.int32), np.array([v[wid] for wid in ids], np.float64), fv


def score_l1(a, b):
    """ScoringObject.cpp:23-68 on two (ids ascending, values): the terms of the common words added in key order, then -score / 2."""
    (i1, v1), (i2, v2) = a, b
    p = q = 0
    score = 0.0
    while p < len(i1) and q < len(i2):
        if i1[p] == i2[q]:
            vi, wi = float(v1[p]), float(v2[q])
            score = score + (abs(vi - wi) - abs(vi) - abs(wi))                         # :41
            p += 1; q += 1
        elif i1[p] < i2[q]:
            while p < len(i1) and i1[p] < i2[q]:                                       # lower_bound, :50
                p += 1
        else:
            while q < len(i2) and i2[q] < i1[p]:
                q += 1
    return -score / 2.0


# ------------------------------------------------------------------------------------------------------------ distinctive descriptor
def distinctive(desc, *, wrong=(), trace=None):
    """MapPoint.cpp:957-988: the row whose median distance to all rows (itself included, as 0) is least; the median is the sorted row
    read at int(0.5 * (N - 1)) (:981) and only a strictly smaller median replaces the best (:983), so the first minimal row wins.
    N = 0: the reference returns before this point (:956); -1 here."""
    b = bits(desc)
    n = len(b)
    if n == 0:
        return -1
    best_median, best_idx = 2147483647, 0
    at = n // 2 if "median_upper" in wrong else int(0.5 * (n - 1))
    medians = []
    for i in range(n):
        row = sorted(int(x) for x in (b != b[i][None, :]).sum(axis=1))
        median = row[at]
        medians.append(median)
        if median < best_median or ("median_tie_last" in wrong and median == best_median):
            best_median, best_idx = median, i
    if trace is not None:
        tied = [i for i, m in enumerate(medians) if m == best_median]
        if len(tied) > 1:
            _note(trace, "median_tie")
            if any(j % 64 < tied[0] % 64 for j in tied[1:]):
                _note(trace, "median_tie_later_row_smaller_lane")
        if max(medians) == 256:
            _note(trace, "median_256")
    return best_idx


# ------------------------------------------------------------------------------------------------------------ FeatureVector
def feature_vector(node):
    """The FeatureVector of Frame::ComputeBoW as three arrays: (order = the features that have a node by (node, feature index), nodes =
    the distinct node ids ascending, first = where each node's features start in order, with the total appended)."""
    node = [int(x) for x in node]
    order = sorted((i for i in range(len(node)) if node[i] >= 0), key=lambda i: (node[i], i))
    nodes, first = [], []
    for p, i in enumerate(order):
        if p == 0 or node[i] != node[order[p - 1]]:
            nodes.append(node[i]); first.append(p)
    first.append(len(order))
    return np.array(order, np.int32), np.array(nodes, np.int32), np.array(first, np.int32)


def _entries(node, wrong):
    """std::map<NodeId, vector<unsigned>>: {node: features ascending} and the sorted keys."""
    m = {}
    for i, nd in enumerate(node):
        nd = int(nd)
        if nd >= 0 or "negative_nodes_match" in wrong:
            m.setdefault(nd, []).append(i)
    return m, sorted(m)


def _common_nodes(k1, k2):
    """The merge walk of :199-283 over two sorted key lists -> the keys both hold, in order."""
    out = []
    p = q = 0
    while p < len(k1) and q < len(k2):
        if k1[p] == k2[q]:
            out.append(k1[p]); p += 1; q += 1
        elif k1[p] < k2[q]:
            while p < len(k1) and k1[p] < k2[q]:                                       # lower_bound(:277)
                p += 1
        else:
            while q < len(k2) and k2[q] < k1[p]:
                q += 1
    return out


def _rot_bin(a1, a2, wrong, trace):
    """:257-262 through window_matcher_ref.rot_bin (round half away from zero, HISTO_LENGTH -> 0)."""
    rot = F(F(a1) - F(a2))
    if float(rot) < 0.0:
        _note(trace, "rot_negative")
        rot = F(rot + F(360.0))
    x = F(rot * F(F(1.0) / F(HISTO_LENGTH)))
    half = float(x) - np.floor(float(x)) == 0.5
    if half:
        _note(trace, "bin_half")
    if half and "bin_round_half_even" in wrong:
        b = int(np.rint(float(x)))
        return 0 if b == HISTO_LENGTH else b
    return rot_bin(a1, a2)


def search_by_bow(desc1, node1, valid1, angle1, desc2, node2, angle2, valid2=None, nnratio=0.6, check_ori=True, kfkf=False,
                  *, wrong=(), trace=None):
    """Both SearchByBoW overloads.  Side 1 is the keyframe whose map points are matched (valid1[i] = it holds a good map point, :210-216
    / :601-605); side 2 is the Frame (kfkf False, :178-306: a candidate is skipped once vpMapPointMatches holds a point for it, :228;
    accepted at best <= TH_LOW, :247) or the second KeyFrame (kfkf True, :565-698: skipped when vbMatched2 or without a good map
    point = !valid2, :619-623; accepted at best < TH_LOW, :641).  Both: float ratio test (:249 / :643), rotation histogram and
    ComputeThreeMaxima (:285-303 / :677-695).
    -> (nmatches, match12 [n1]) and, for the Frame form, also match21 [n2] = the keyframe feature per frame feature (:251)."""
    b1, b2 = bits(desc1), bits(desc2)
    n1, n2 = len(b1), len(b2)
    e1, k1 = _entries(node1, wrong)
    e2, k2 = _entries(node2, wrong)
    match12 = np.full(n1, -1, np.int32)
    taken = np.zeros(n2, bool)
    taken_by = np.full(n2, -1, np.int32)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    inclusive = not kfkf
    if "th_inclusive_both" in wrong:
        inclusive = True
    if "th_strict_both" in wrong:
        inclusive = False
    if trace is not None:
        _note(trace, "nodes_one_side_only", len(set(k1) ^ set(k2)))
        _note(trace, "negative_nodes_both_sides", int((np.asarray(node1) < 0).any() and (np.asarray(node2) < 0).any()))
    for nd in _common_nodes(k1, k2):
        _note(trace, "groups")
        g2 = e2[nd]
        if trace is not None:
            trace["max_group2"] = max(trace.get("max_group2", 0), len(g2))
        for idx1 in e1[nd]:
            if not valid1[idx1]:
                _note(trace, "skipped_invalid1")
                continue
            dist = (b2[g2] != b1[idx1][None, :]).sum(axis=1)
            best1, best2, best_idx = 256, 256, -1                                      # :220-222
            usable, skipped = [], []
            for pos, (idx2, d) in enumerate(zip(g2, dist)):
                d = int(d)
                skip_taken = bool(taken[idx2])
                skip_invalid = bool(kfkf and not valid2[idx2])
                if skip_taken or skip_invalid:                                         # :228 / :619-623
                    _note(trace, "skipped_taken", int(skip_taken))
                    _note(trace, "skipped_invalid2", int(skip_invalid and not skip_taken))
                    if (skip_taken and not skip_invalid and "taken_counts_for_second" in wrong) or \
                            (skip_invalid and not skip_taken and "valid2_counts_for_second" in wrong):
                        skipped.append(d)
                    continue
                usable.append((pos, d))
                if d < best1:                                                          # :235-240
                    best2, best1, best_idx = best1, d, idx2
                elif d < best2 and not ("second_distinct" in wrong and d == best1):    # :241-244
                    best2 = d
            if skipped:                                                                # the two wrong variants only
                best2 = min(best2, min(skipped))
            if trace is not None and best_idx >= 0:
                _note(trace, "dist_256_candidate", int(any(d == 256 for _, d in usable)))
                if sum(1 for _, d in usable if d == best1) > 1:
                    _note(trace, "best_tie")
                if best2 == best1:
                    _note(trace, "second_eq_best")
                if best2 == 256 and best1 < 256:
                    _note(trace, "lone_candidate")
                if best1 == TH_LOW:
                    _note(trace, "best_eq_th")
                if best1 == TH_LOW + 1:
                    _note(trace, "best_eq_th_plus_1")
                best_pos = g2.index(best_idx)                                          # where the best and its equals sit, in chunks of 64
                if any(d == best1 and p // 64 > best_pos // 64 for p, d in usable):
                    _note(trace, "later_chunk_equals_best")
                if best_pos % 64 == 63:
                    _note(trace, "best_at_lane_63")
                if best_pos >= 64 and best_pos % 64 == 0:
                    _note(trace, "best_at_lane_0_of_a_later_chunk")
                second_pos = [p for p, d in usable if d == best2 and p != best_pos]
                if second_pos:
                    _note(trace, "second_in_same_chunk", int(any(p // 64 == best_pos // 64 for p in second_pos)))
                    _note(trace, "second_in_other_chunk", int(all(p // 64 != best_pos // 64 for p in second_pos)))
            if trace is not None and best_idx < 0:
                _note(trace, "no_candidate")
            if not (best1 <= TH_LOW if inclusive else best1 < TH_LOW):                 # :247 / :641
                continue
            if "ratio_in_double" in wrong:
                ok = float(best1) < float(F(nnratio)) * float(best2)
            else:
                ok = F(best1) < F(F(nnratio) * F(best2))                               # :249 / :643
            if trace is not None:
                if F(best1) == F(F(nnratio) * F(best2)):
                    _note(trace, "ratio_equal")
                if (F(best1) < F(F(nnratio) * F(best2))) != (float(best1) < float(F(nnratio)) * float(best2)):
                    _note(trace, "ratio_float_differs_from_double")
            if not ok:
                _note(trace, "ratio_rejected")
                continue
            match12[idx1] = best_idx                                                   # :251 / :645-646
            taken[best_idx] = True
            taken_by[best_idx] = idx1
            nmatches += 1
            if check_ori:                                                              # :255-265 / :648-658
                rot_hist[_rot_bin(angle1[idx1], angle2[best_idx], wrong, trace)].append(idx1)
    if check_ori:                                                                      # :285-303 / :677-695
        keep = three_maxima([len(h) for h in rot_hist], wrong=wrong, trace=trace)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in rot_hist[b]:
                taken_by[match12[idx1]] = -1
                match12[idx1] = -1
                nmatches -= 1
                _note(trace, "cleared_by_histogram")
    if kfkf:
        return nmatches, match12
    return nmatches, match12, taken_by


# ------------------------------------------------------------------------------------------------------------ SearchForTriangulation
def check_dist_epipolar_line(x1, y1, x2, y2, octave2, F12, level_sigma2, *, trace=None):
    """:159-176 in float; the last comparison is float < double (3.84 * float widens to double)."""
    f = np.asarray(F12, F).reshape(3, 3)
    x1, y1, x2, y2 = F(x1), F(y1), F(x2), F(y2)
    a = F(F(F(x1 * f[0, 0]) + F(y1 * f[1, 0])) + f[2, 0])                              # :162
    b = F(F(F(x1 * f[0, 1]) + F(y1 * f[1, 1])) + f[2, 1])
    c = F(F(F(x1 * f[0, 2]) + F(y1 * f[1, 2])) + f[2, 2])
    num = F(F(F(a * x2) + F(b * y2)) + c)                                              # :166
    den = F(F(a * a) + F(b * b))                                                       # :168
    if den == 0:                                                                       # :170
        _note(trace, "den_zero")
        return False
    dsqr = F(F(num * num) / den)                                                       # :173
    return float(dsqr) < 3.84 * float(F(level_sigma2[octave2]))                        # :175


def search_for_triangulation(desc1, node1, has_mp1, x1, y1, angle1, desc2, node2, has_mp2, x2, y2, angle2, octave2, F12, ex, ey,
                             scale_factors2, level_sigma2_2, check_ori=False, *, wrong=(), trace=None):
    """:700-852 with the epipole (ex, ey) given.  bestDist starts at TH_LOW and a candidate is passed over when dist > TH_LOW or
    dist > bestDist (:770): an equal distance goes on to the two geometric gates and, passing them, REPLACES the best (:780-784), so
    of equally near passing candidates the last one wins.  vbMatched2 is declared (:721) and never set: a feature of side 2 may be
    chosen by any number of features of side 1.  -> (nmatches, match12 [n1])."""
    b1, b2 = bits(desc1), bits(desc2)
    n1 = len(b1)
    e1, k1 = _entries(node1, wrong)
    e2, k2 = _entries(node2, wrong)
    ex, ey = F(ex), F(ey)
    sf = np.asarray(scale_factors2, F)
    has2 = [bool(x) for x in has_mp2]
    match12 = np.full(n1, -1, np.int32)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for nd in _common_nodes(k1, k2):
        g2 = e2[nd]
        if trace is not None:
            trace["max_group2"] = max(trace.get("max_group2", 0), len(g2))
        for idx1 in e1[nd]:
            if has_mp1[idx1]:                                                          # :743-747
                _note(trace, "skipped_has_mp1")
                continue
            dist = (b2[g2] != b1[idx1][None, :]).sum(axis=1).tolist()
            best, best_idx = TH_LOW, -1                                                # :753-754
            for pos, idx2 in enumerate(g2):
                d = dist[pos]
                if has2[idx2]:                                                         # :763
                    _note(trace, "skipped_has_mp2")
                    continue
                if trace is not None:
                    _note(trace, "dist_eq_th", int(d == TH_LOW))
                    _note(trace, "dist_eq_th_plus_1", int(d == TH_LOW + 1))
                if "tri_th_strict" in wrong and d >= TH_LOW:
                    continue
                if d > TH_LOW or d > best:                                             # :770
                    continue
                if "tri_tie_first" in wrong and best_idx >= 0 and d == best:
                    continue
                dx = F(ex - F(x2[idx2])); dy = F(ey - F(y2[idx2]))                     # :775-776
                r2 = F(F(dx * dx) + F(dy * dy))
                lim = F(F(100) * sf[octave2[idx2]])                                    # :777
                if trace is not None:
                    _note(trace, "epipole_at_limit", int(r2 == lim))
                    _note(trace, "epipole_just_above", int(r2 == np.nextafter(lim, F(np.inf))))
                if r2 < lim or ("epipole_inclusive" in wrong and r2 == lim):
                    _note(trace, "epipole_rejected")
                    continue
                if check_dist_epipolar_line(x1[idx1], y1[idx1], x2[idx2], y2[idx2], octave2[idx2], F12, level_sigma2_2, trace=trace):
                    if best_idx >= 0 and d == best:
                        _note(trace, "equal_replaces")
                        if (pos - best_pos) % 64 == 0:
                            _note(trace, "equal_replaces_same_lane")
                        if pos // 64 != best_pos // 64:
                            _note(trace, "equal_replaces_across_stride")
                    best_idx, best, best_pos = idx2, d, pos                            # :782-783
                else:
                    _note(trace, "epipolar_rejected")
            if best_idx >= 0:                                                          # :787-804
                match12[idx1] = best_idx
                nmatches += 1
                if check_ori:
                    rot_hist[_rot_bin(angle1[idx1], angle2[best_idx], wrong, trace)].append(idx1)
    if check_ori:                                                                      # :820-839
        keep = three_maxima([len(h) for h in rot_hist], wrong=wrong, trace=trace)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in rot_hist[b]:
                match12[idx1] = -1
                nmatches -= 1
                _note(trace, "cleared_by_histogram")
    return nmatches, match12
