"""Hand-built frames for the windowed matchers: no extraction, no GPU, every distance known by construction.

A descriptor is BASE with chosen bits flipped; unless said otherwise a query carries BASE itself and a feature
"of distance d" has bits 0..d-1 flipped, so its Hamming distance to every query of the case is d.  Coordinates are small
integers or one-ulp neighbours of them, so that every float expression of the reference (differences, products with the
scale factor, the grid cell) is exact or far from a rounding boundary unless the case is about that boundary.

Every builder returns a dict: name, kind (which entry point), grid (keyword arguments of window_matcher_ref.Grid;
by_sim3: grid1 / grid2), args (the entry point's arguments in order of window_matcher_ref's function), forces
(trace key -> the least number of times the case makes the reference take that decision).  run_ref() runs a case
through the definition; the outputs are tuples of numpy arrays / ints, compared with == everywhere.
"""
import numpy as np

import window_matcher_ref as R

F = np.float32
BASE = np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8)
SF = np.cumprod(np.concatenate([[F(1.0)], np.full(7, F(1.2), F)]), dtype=F)      # mvScaleFactors of ORBextractor(1.2, 8)
PREV = lambda v: np.nextafter(F(v), F(-np.inf))                                  # noqa: E731  the float before v
NEXT = lambda v: np.nextafter(F(v), F(np.inf))                                   # noqa: E731


def desc(d=0, bits=None):
    """BASE with bits 0..d-1 (or the listed bits) flipped."""
    b = np.unpackbits(BASE)
    b[list(range(d)) if bits is None else list(bits)] ^= 1
    return np.packbits(b)


class _Feats:
    def __init__(self, **bounds):
        self.x, self.y, self.o, self.d, self.a, self.bounds = [], [], [], [], [], bounds

    def add(self, x, y, octave=0, d=0, angle=0.0, bits=None):
        self.x.append(F(x)); self.y.append(F(y)); self.o.append(octave); self.d.append(desc(d, bits)); self.a.append(F(angle))
        return len(self.x) - 1

    def grid(self):
        return dict(kx=np.array(self.x, F), ky=np.array(self.y, F), octave=np.array(self.o, np.int32),
                    desc=np.array(self.d, np.uint8).reshape(-1, 32), angle=np.array(self.a, F), **self.bounds)


class _Pts:
    """Queries: position, level, descriptor, the per-point flag (has_obs / observed), active, angle."""

    def __init__(self):
        self.x, self.y, self.l, self.d, self.f, self.v, self.a = [], [], [], [], [], [], []

    def add(self, x, y, level=1, flag=1, d=0, bits=None, active=1, angle=0.0):
        self.x.append(F(x)); self.y.append(F(y)); self.l.append(level); self.d.append(desc(d, bits)); self.f.append(flag)
        self.v.append(active); self.a.append(F(angle))
        return len(self.x) - 1

    def arrays(self):
        return dict(x=np.array(self.x, F), y=np.array(self.y, F), level=np.array(self.l, np.int32),
                    desc=np.array(self.d, np.uint8).reshape(-1, 32), flag=np.array(self.f, np.uint8), active=np.array(self.v, np.uint8),
                    angle=np.array(self.a, F))


def _projection(name, fe, pt, forces, th=1.0, nnratio=0.8, occupied=None, view_cos=0.5):
    """kind projection: mode 0.  view_cos 0.5 -> r = 4 (x th when th != 1) x scale factor of the level."""
    g, p = fe.grid(), pt.arrays()
    n = len(g["kx"])
    return dict(name=name, kind="projection", grid=g, forces=forces,
                args=dict(scale_factors=SF, in_view=p["active"], level=p["level"], view_cos=np.full(len(p["x"]), view_cos, F), proj_x=p["x"],
                          proj_y=p["y"], mp_desc=p["desc"], has_obs=p["flag"], occupied=np.zeros(n, np.uint8) if occupied is None else occupied,
                          th=th, nnratio=nnratio))


def _sim3(name, fe, pt, forces, th=4.0, matched=None):
    g, p = fe.grid(), pt.arrays()
    n = len(g["kx"])
    return dict(name=name, kind="sim3", grid=g, forces=forces,
                args=dict(scale_factors=SF, valid=p["active"], u=p["x"], v=p["y"], level=p["level"], mp_desc=p["desc"], observed=p["flag"],
                          matched=np.zeros(n, np.uint8) if matched is None else matched, th=th))


def _frame(name, fe, pt, forces, th=4.0, check_ori=False, orb_dist=100, occupied=None):
    g, p = fe.grid(), pt.arrays()
    n = len(g["kx"])
    return dict(name=name, kind="frame", grid=g, forces=forces,
                args=dict(scale_factors=SF, valid=p["active"], u=p["x"], v=p["y"], last_octave=p["level"], last_angle=p["angle"],
                          mp_desc=p["desc"], has_obs=p["flag"], occupied=np.zeros(n, np.uint8) if occupied is None else occupied, th=th,
                          check_ori=check_ori, orb_dist=orb_dist))


def _fuse(name, fe, pt, forces, th=4.0, chi2=False, accept_th=50, is2=None):
    g, p = fe.grid(), pt.arrays()
    return dict(name=name, kind="fuse", grid=g, forces=forces,
                args=dict(scale_factors=SF, inv_level_sigma2=np.ones(8, F) if is2 is None else is2, valid=p["active"], u=p["x"], v=p["y"],
                          level=p["level"], mp_desc=p["desc"], th=th, chi2_check=chi2, accept_th=accept_th))


# ------------------------------------------------------------------------------------------------ geometry
def area_radius_edge():
    """Query (100, 100), r = 8: a feature at exactly x + r, x - r, y + r is outside (strict <), its float neighbour is inside.
    Grid 752 x 480: x 92 -> column 9, 100 -> 10, 108 -> 11; y 100 -> row 10, 108 -> row 11."""
    fe = _Feats()
    fe.add(108, 100); fe.add(PREV(108), 100); fe.add(100, 108); fe.add(100, PREV(108)); fe.add(92, 100); fe.add(NEXT(92), 100)
    return dict(name="area_radius_edge", kind="area", grid=fe.grid(), args=dict(queries=[(100, 100, 8, -1, -1)]),
                forces=dict(at_radius_excluded=3, just_inside_radius=3))


def area_zero_outside_whole():
    """r = 0 finds nothing, not even a feature at the query; queries far outside each side leave early; r = 1000 covers the grid
    and returns every feature that has a cell, by column, row, index."""
    fe = _Feats()
    fe.add(700, 400); fe.add(100, 100); fe.add(100, 50); fe.add(30, 470); fe.add(100, 100.25)
    q = [(100, 100, 0, -1, -1), (-500, 100, 10, -1, -1), (1500, 100, 10, -1, -1), (100, -500, 10, -1, -1), (100, 1500, 10, -1, -1),
         (376, 240, 1000, -1, -1)]
    return dict(name="area_zero_outside_whole", kind="area", grid=fe.grid(), args=dict(queries=q), forces=dict(max_candidates=5))


def area_max_x():
    """A feature at mnMaxX = 752 has cell column 75 = FRAME_GRID_COLS: PosInGrid refuses it, no window finds it.  So does x = 748
    (74.6 rounds to 75; a floor would keep it); x = 746 (74.4) is in column 74."""
    fe = _Feats()
    fe.add(752, 100); fe.add(746, 100); fe.add(748, 100)
    return dict(name="area_max_x", kind="area", grid=fe.grid(), args=dict(queries=[(749, 100, 5, -1, -1)]), forces={})


def area_half_cells():
    """Bounds (-16, 584) x (-8, 376): both cell sizes are exactly 8, so (x + 16) / 8 lands on k + 0.5 exactly.  x = 4 -> 2.5 -> column 3,
    x = 3 -> 2.375 -> column 2: the window (3.5, 100, 4) visits feature 1 before feature 0.  x = -20 -> -0.5 -> round away from zero
    = -1: no cell (round-half-even would say 0); x = -19 -> -0.375 -> column 0 (a floor says -1).  Negative coordinates throughout."""
    fe = _Feats(min_x=-16.0, max_x=584.0, min_y=-8.0, max_y=376.0)
    fe.add(4, 100); fe.add(3, 100); fe.add(-20, 100); fe.add(-19, 100); fe.add(-15, -7)
    q = [(3.5, 100, 4, -1, -1), (-18, 100, 4, -1, -1), (-14, -6, 2, -1, -1)]
    return dict(name="area_half_cells", kind="area", grid=fe.grid(), args=dict(queries=q), forces={})


def area_levels():
    """Five features of octave 0..4 in one cell; bCheckLevels = minLevel > 0 || maxLevel >= 0 in every combination."""
    fe = _Feats()
    for o in range(5):
        fe.add(100 + 0.25 * o, 100, o)
    q = [(100, 100, 8, mn, mx) for mn, mx in ((-1, -1), (0, -1), (0, 0), (1, -1), (2, 3))]
    return dict(name="area_levels", kind="area", grid=fe.grid(), args=dict(queries=q), forces={})


# ------------------------------------------------------------------------------------------------ visiting order
def _tie_feats():
    """Feature 1 (higher index) at x = 94 lies in column 9, feature 0 at x = 105 in column 10: both at distance 20 from the query
    at (100, 100), different octaves so that mode 0's ratio test stays out of it."""
    fe = _Feats()
    fe.add(105, 100, 1, 20); fe.add(94, 100, 0, 20)
    return fe


def proj_tie_order():
    pt = _Pts(); pt.add(100, 100, 1)                                # r = 4 * 2 * 1.2 = 9.6
    return _projection("proj_tie_order", _tie_feats(), pt, dict(tie_by_order=1, ratio_skipped_by_level=1), th=2.0)


def sim3_tie_order():
    pt = _Pts(); pt.add(100, 100, 1, flag=0)                        # r = 8 * 1.2
    return _sim3("sim3_tie_order", _tie_feats(), pt, dict(tie_by_order=1), th=8.0)


def frame_tie_order():
    pt = _Pts(); pt.add(100, 100, 1)
    return _frame("frame_tie_order", _tie_feats(), pt, dict(tie_by_order=1), th=8.0)


def fuse_tie_order():
    pt = _Pts(); pt.add(100, 100, 1)
    return _fuse("fuse_tie_order", _tie_feats(), pt, dict(tie_by_order=1), th=8.0)


# ------------------------------------------------------------------------------------------------ thresholds
def proj_thresholds():
    """nnratio 0.5, points 100 px apart, level 1 (r = 4.8, octaves 0 and 1 pass).  A: lone feature at 100 -> taken.  B: lone at 101 ->
    not.  C: 10 and 20, same octave: 10 > 0.5 * 20 is false -> taken.  D: 11 and 20 same octave -> rejected.  E: 11 and 20 on
    different octaves -> taken."""
    fe, pt = _Feats(), _Pts()
    fe.add(100, 100, 1, 100); pt.add(100, 100)
    fe.add(200, 100, 1, 101); pt.add(200, 100)
    fe.add(300, 100, 1, 10); fe.add(302, 100, 1, 20); pt.add(301, 100)
    fe.add(400, 100, 1, 11); fe.add(402, 100, 1, 20); pt.add(401, 100)
    fe.add(500, 100, 1, 11); fe.add(502, 100, 0, 20); pt.add(501, 100)
    return _projection("proj_thresholds", fe, pt, dict(best_eq_th=1, best_eq_th_plus_1=1, ratio_equal_kept=1, ratio_rejected=1,
                                                       ratio_skipped_by_level=1), nnratio=0.5)


def sim3_thresholds():
    """TH_LOW: 50 taken, 51 not.  Third point (level 1): a feature of octave 2 at distance 0 is filtered inside the loop, the
    octave-0 feature at 30 is chosen."""
    fe, pt = _Feats(), _Pts()
    fe.add(100, 100, 1, 50); pt.add(100, 100, flag=0)
    fe.add(200, 100, 1, 51); pt.add(200, 100, flag=0)
    fe.add(300, 100, 2, 0); fe.add(302, 100, 0, 30); pt.add(301, 100, flag=0)
    return _sim3("sim3_thresholds", fe, pt, dict(best_eq_th=1, best_eq_th_plus_1=1))


def frame_thresholds(orb_dist):
    """orb_dist taken, orb_dist + 1 not; window octaves [o - 1, o + 1]: with o = 1 an octave-3 feature at distance 0 is outside."""
    fe, pt = _Feats(), _Pts()
    fe.add(100, 100, 1, orb_dist); pt.add(100, 100)
    fe.add(200, 100, 1, orb_dist + 1); pt.add(200, 100)
    fe.add(300, 100, 3, 0); fe.add(302, 100, 2, 30); pt.add(301, 100)
    return _frame("frame_thresholds_%d" % orb_dist, fe, pt, dict(best_eq_th=1, best_eq_th_plus_1=1), orb_dist=orb_dist)


def fuse_thresholds(accept_th):
    fe, pt = _Feats(), _Pts()
    fe.add(100, 100, 1, accept_th); pt.add(100, 100)
    fe.add(200, 100, 1, accept_th + 1); pt.add(200, 100)
    fe.add(300, 100, 2, 0); fe.add(302, 100, 0, 30); pt.add(301, 100)
    fe.add(400, 100, 1, 5); pt.add(400, 100, active=0)
    return _fuse("fuse_thresholds_%d" % accept_th, fe, pt, dict(best_eq_th=1, best_eq_th_plus_1=1), accept_th=accept_th)


def fuse_chi2():
    """e2 = 1 exactly (the feature one pixel beside the projection), so e2 * invSigma2 is invSigma2 itself: octave 0 carries the largest
    float below 5.99, octave 1 the smallest above.  Point 0 (level 0): its octave-0 feature passes.  Point 1 (level 1): the octave-1
    feature at distance 10 fails the test, the octave-0 feature at distance 30 passes and is chosen."""
    fe, pt = _Feats(), _Pts()
    fe.add(99, 100, 0, 10); pt.add(100, 100, 0)
    fe.add(199, 100, 1, 10); fe.add(201, 100, 0, 30); pt.add(200, 100, 1)
    is2 = np.ones(8, F); is2[0] = R.CHI2_BELOW; is2[1] = R.CHI2_ABOVE
    return _fuse("fuse_chi2", fe, pt, dict(chi2_adjacent_kept=2, chi2_adjacent_rejected=1), chi2=True, is2=is2)


# ------------------------------------------------------------------------------------------------ order dependence
def proj_order_a():
    """(a) five points without observations want the one feature: each is accepted and counted, the last owns it, it stays free."""
    fe, pt = _Feats(), _Pts()
    fe.add(100, 100, 1, 10)
    for k in range(5):
        pt.add(100 + 0.5 * k, 100, flag=0)
    return _projection("proj_order_a", fe, pt, dict(overwrite=4))


def proj_order_b():
    """(b) four points with observations, features at 10 / 30 / 40 (same octave; 10 < 0.8 * 30, 30 < 0.8 * 40): the first takes 10,
    the second 30, the third 40, the fourth finds nothing."""
    fe, pt = _Feats(), _Pts()
    fe.add(100, 100, 1, 10); fe.add(101, 100, 1, 30); fe.add(102, 100, 1, 40)
    for k in range(4):
        pt.add(101, 100)
    return _projection("proj_order_b", fe, pt, dict(candidate_taken_earlier=3))


def proj_order_cd():
    """(c) X at (207, 100) sees only g1 (204, d 12) and takes it; Y at (202, 100) sees g0 (200, d 10) and g1: alone it would fail the
    ratio test (10 > 0.8 * 12), after X it has no second and takes g0.
    (d) R at (402, 100) sees h0 (400, d 10) and h1 (404, d 12), is rejected and leaves both free; S at (397, 100) sees only h0, takes it."""
    fe, pt = _Feats(), _Pts()
    fe.add(200, 100, 1, 10); fe.add(204, 100, 1, 12); fe.add(400, 100, 1, 10); fe.add(404, 100, 1, 12)
    pt.add(207, 100); pt.add(202, 100); pt.add(402, 100); pt.add(397, 100)
    return _projection("proj_order_cd", fe, pt, dict(verdict_changed_by_earlier=1, ratio_rejected=1, rejected_feature_taken_later=1))


def sim3_order_e():
    """(e) f0 at 10, f1 at 20.  p0 observed: chooses f0, sets nothing.  p1: takes f0 (count 1).  p2 observed: f0 is matched, chooses
    f1, sets nothing.  p3: takes f1 (count 2).  p4: nothing left."""
    fe, pt = _Feats(), _Pts()
    fe.add(100, 100, 1, 10); fe.add(101, 100, 1, 20)
    for k in range(5):
        pt.add(100.5, 100, flag=1 if k in (0, 2) else 0)
    return _sim3("sim3_order_e", fe, pt, dict(observed_chose=2, taken_after_observed_chose=2, candidate_taken_earlier=3))


def _lattice(k, x0=40.0, y0=40.0, step=30.0, per_row=20):
    return F(x0 + step * (k % per_row)), F(y0 + step * (k // per_row))


def frame_hist_ties():
    """(f) one lone feature per point (lattice, 30 px apart, th 3, octave 0), bins by last_angle = 30 * bin, current angle 0:
    bins 2: 3, 5: 3, 7: 2, 9: 2, 11: 1.  ComputeThreeMaxima's strict compares keep 2, 5, 7; bins 9 and 11 go: three matches cleared.
    The bin-11 entry is point A (no observations) on feature 0; point B, later, in bin 2, re-takes feature 0.  A's stale entry
    clears feature 0 although B owns it: 11 accepted - 3 = 8 counted, 7 features still matched."""
    fe, pt = _Feats(), _Pts()
    x, y = _lattice(0)
    fe.add(x, y, 0, 10)
    a = pt.add(x, y, 0, flag=0, angle=330.0)                       # A: bin 11
    k = 1
    for b, cnt in ((2, 2), (5, 3), (7, 2), (9, 2)):
        for _ in range(cnt):
            x, y = _lattice(k); k += 1
            fe.add(x, y, 0, 10); pt.add(x, y, 0, angle=30.0 * b)
    x, y = _lattice(0)
    pt.add(x, y, 0, angle=60.0)                                    # B: bin 2, same feature as A
    assert a == 0
    return _frame("frame_hist_ties", fe, pt, dict(bins_tied_12=1, bins_tied_34=1, stale_clear=1, overwrite=1), th=3.0, check_ori=True)


def frame_hist_tenth(first):
    """bins 3: `first`, 6: 1.  first = 10: max2 = 1 is not below 0.1f * 10 = 1.0f -> both bins stay; first = 11: 1 < 1.1f -> bin 6 goes."""
    fe, pt = _Feats(), _Pts()
    for k in range(first + 1):
        x, y = _lattice(k)
        fe.add(x, y, 0, 10); pt.add(x, y, 0, angle=90.0 if k < first else 180.0)
    key = "second_at_tenth" if first == 10 else "second_below_tenth"
    return _frame("frame_hist_tenth_%d" % first, fe, pt, {key: 1}, th=3.0, check_ori=True)


# ------------------------------------------------------------------------------------------------ SearchBySim3, SearchForInitialization
def by_sim3_agreement():
    """KF1 feature 0 <-> KF2 feature 0 at distance 100 both ways: kept.  KF1's 1 picks KF2's 1, whose point picks KF1's 2: dropped.
    KF1's 2 finds KF2's 2 at 101: nothing."""
    f1, f2, p1, p2 = _Feats(), _Feats(), _Pts(), _Pts()
    f1.add(100, 100, 1, 100); f1.add(200, 100, 1, 10); f1.add(300, 100, 1, 10)
    f2.add(100, 200, 1, 100); f2.add(200, 200, 1, 10); f2.add(300, 200, 1, 101)
    p1.add(100, 200); p1.add(200, 200); p1.add(300, 200)            # the points of KF1's features, projected into KF2
    p2.add(100, 100); p2.add(300, 100); p2.add(300, 100, active=0)  # the points of KF2's features, projected into KF1
    a, b = p1.arrays(), p2.arrays()
    return dict(name="by_sim3_agreement", kind="by_sim3", grid1=f1.grid(), grid2=f2.grid(),
                forces=dict(best_eq_th=2, best_eq_th_plus_1=1, directions_disagree=1),
                args=dict(sf1=SF, sf2=SF, valid1=a["active"], u1=a["x"], v1=a["y"], level1=a["level"], mp_desc1=a["desc"],
                          valid2=b["active"], u2=b["x"], v2=b["y"], level2=b["level"], mp_desc2=b["desc"], th=4.0))


def init_basic():
    """window 10, nnratio 0.5, check_ori.  F2: a0 (100,100) = bits 0..9, a1 (103,100) = bits 20..49, a2 (300,100) d 50, a3 (400,100) d 51,
    a4 (500,100) d 10, a5 (502,100) d 20, a6 (301,100) octave 1 d 0.
    i0 BASE at a0: 10 < 0.5 * 30 -> a0.  i1 bits 0..4: 5 to a0, 35 to a1 -> takes a0, i0 is un-matched.  i2 octave 1: skipped.
    i3 BASE: a0 is kept by its nearer claimant (5 <= 10), a1 at 30 with no second -> a1.  i4: a2 at 50 -> taken (a6 is octave 1).
    i5: a3 at 51 -> no.  i6: 10 < 0.5f * 20 is false -> rejected (the other way round than SearchByProjection's >).
    Histogram: i0 -> bin 11, i1 -> 0, i3 -> 1, i4 -> 2: bin 11 is the fourth, removed; i0 is already un-matched, nothing to clear."""
    f2 = _Feats()
    f2.add(100, 100, 0, bits=range(10)); f2.add(103, 100, 0, bits=range(20, 50)); f2.add(300, 100, 0, 50); f2.add(400, 100, 0, 51)
    f2.add(500, 100, 0, 10); f2.add(502, 100, 0, 20); f2.add(301, 100, 1, 0)
    p = _Pts()
    p.add(100, 100, 0, angle=330.0); p.add(101, 100, 0, bits=range(5)); p.add(100, 100, 1); p.add(101, 100, 0, angle=30.0)
    p.add(300, 100, 0, angle=60.0); p.add(400, 100, 0); p.add(501, 100, 0)
    a = p.arrays()
    return dict(name="init_basic", kind="init", grid=f2.grid(),
                forces=dict(previous_owner_unmatched=1, kept_by_nearer_claimant=1, best_eq_th=1, best_eq_th_plus_1=1, ratio_equal_rejected=1,
                            ratio_rejected=1, histogram_entry_already_unmatched=1),
                args=dict(oct1=a["level"], desc1=a["desc"], angle1=a["angle"], prev_matched=np.stack([a["x"], a["y"]], 1), window=10,
                          nnratio=0.5, check_ori=True))


# ------------------------------------------------------------------------------------------------ kernel sizes
SIZE_POINTS = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
N_CHAIN = 200


def _chain_feats():
    """200 features inside one window around (300, 200) (a 20 x 10 lattice, 2 px apart), feature j at distance j + 1, octaves
    alternating 0 / 1: the nearest free one and the next are never of one octave, so mode 0's ratio test never applies."""
    fe = _Feats()
    for j in range(N_CHAIN):
        fe.add(281 + 2 * (j % 20), 191 + 2 * (j // 20), j % 2, j + 1)
    return fe


def size_chain(kind, n_pts):
    """Variant (b) at a kernel size: n_pts points with the flag set, all at (300, 200) with r = 24 (200 candidates each: the 16 in
    registers, the spill path and the cap = 64 retry at once).  Point m takes feature m while m + 1 <= threshold; every point
    waits for all earlier ones: a chain far longer than a wave and than the three workgroup-wide rounds."""
    pt = _Pts()
    for m in range(n_pts):
        pt.add(300, 200, 1, flag=0 if kind == "sim3" else 1)
    forces = dict(max_candidates=N_CHAIN)
    if n_pts > 1:
        forces["candidate_taken_earlier"] = n_pts - 1
    name = "size_chain_%s_%d" % (kind, n_pts)
    if kind == "projection":
        return _projection(name, _chain_feats(), pt, forces, th=5.0)
    if kind == "sim3":
        return _sim3(name, _chain_feats(), pt, forces, th=20.0)
    return _frame(name, _chain_feats(), pt, forces, th=20.0)


def size_sparse(kind, n_pts):
    """No contention: 200 lone features on a lattice (30 px apart, r <= 4.8); point m sits on feature m / stride when stride divides m
    (stride = max(1, n_pts / 200)) and in the empty middle of four features otherwise."""
    fe, pt = _Feats(), _Pts()
    for j in range(200):
        x, y = _lattice(j)
        fe.add(x, y, 1, 10 + j % 40)
    stride = max(1, n_pts // 200)
    for m in range(n_pts):
        j = m // stride
        if m % stride == 0 and j < 200:
            x, y = _lattice(j)
            pt.add(x, y, 1, flag=0 if kind == "sim3" else 1)
        else:
            pt.add(55, 55, 1, flag=0 if kind == "sim3" else 1)
    name = "size_sparse_%s_%d" % (kind, n_pts)
    mk = dict(projection=_projection, sim3=_sim3, frame=_frame)[kind]
    return mk(name, fe, pt, dict(max_candidates=1), th=1.0 if kind == "projection" else 4.0)


CLUSTER_SIZES = (0, 1, 16, 17, 64, 65, 200)


def _clusters(sizes, flag):
    """One cluster of c features per entry (100 px apart, a lattice 2 px apart inside r = 24), distances a permutation of 1..c so that
    the nearest sit deep in the list, octaves alternating; three points per cluster."""
    fe, pt = _Feats(), _Pts()
    for k, c in enumerate(sizes):
        cx, cy = 60 + 100 * (k % 7), 60 + 100 * (k // 7)
        for j in range(c):
            fe.add(cx - 19 + 2 * (j % 20), cy - 9 + 2 * (j // 20), j % 2, 1 + (j * 37) % c)
        for _ in range(3):
            pt.add(cx, cy, 1, flag=flag)
    return fe, pt


def cand_counts(kind, sizes):
    """Candidates per point at the register / spill boundary (16, 17), at the first capacity (64) and past it (65, 200: the retry)."""
    fe, pt = _clusters(sizes, 0 if kind == "sim3" else 1)
    name = "cand_%s_%s" % (kind, "_".join(str(s) for s in sizes))
    forces = dict(max_candidates=max(sizes))
    if kind == "projection":
        return _projection(name, fe, pt, forces, th=5.0)
    if kind == "sim3":
        return _sim3(name, fe, pt, forces, th=20.0)
    if kind == "frame":
        return _frame(name, fe, pt, forces, th=20.0)
    return _fuse(name, fe, pt, forces, th=20.0)


def cand_positions(kind, positions):
    """The nearest candidate AT a given list position: per entry p a cluster of p + 2 features in one row, half a pixel apart (visiting
    order = index order), feature j at distance 1 + (j - p) mod (p + 2): the three points of the cluster take list positions p, p + 1
    and 0.  p = 15, 16, 17 straddles the candidates a thread keeps in registers, p = 63, 64, 65 the first list capacity."""
    fe, pt = _Feats(), _Pts()
    for k, p in enumerate(positions):
        c = p + 2
        cx, cy = 100 + 150 * k, 100
        for j in range(c):
            fe.add(cx - 16 + 0.5 * j, cy, j % 2, 1 + (j - p) % c)
        for _ in range(3):
            pt.add(cx, cy, 1, flag=0 if kind == "sim3" else 1)
    name = "pos_%s_%s" % (kind, "_".join(str(p) for p in positions))
    forces = dict(max_candidates=max(positions) + 2)
    if kind == "projection":
        return _projection(name, fe, pt, forces, th=5.0)
    if kind == "sim3":
        return _sim3(name, fe, pt, forces, th=20.0)
    if kind == "frame":
        return _frame(name, fe, pt, forces, th=20.0)
    return _fuse(name, fe, pt, forces, th=20.0)


# ------------------------------------------------------------------------------------------------ batches
def batch(kind):
    """kind sim3 / fuse.  Keyframe 0: sparse, with pre-set matched flags (sim3: feature 0 is matched already, its point falls to the
    second feature).  Keyframe 1: one window of 65 candidates: every keyframe repeats with longer lists after keyframe 0's workgroup
    has set its flags.  Keyframe 2: no features (25 queries).  Keyframe 3: features, no queries.  One th = 20 for the batch (r = 24)."""
    subs = []
    fe, pt = _Feats(), _Pts()
    fe.add(100, 100, 1, 10); fe.add(102, 100, 1, 20); fe.add(300, 100, 1, 15); fe.add(500, 300, 0, 50)
    pt.add(101, 100, flag=0); pt.add(101, 100, flag=0); pt.add(300, 100, flag=0); pt.add(500, 300, flag=0); pt.add(600, 400, flag=0)
    mk = _sim3 if kind == "sim3" else _fuse
    subs.append(mk("kf0", fe, pt, {}, th=20.0, **(dict(matched=np.array([1, 0, 0, 0], np.uint8)) if kind == "sim3" else {})))
    fe, pt = _clusters((65, 17), 0)
    subs.append(mk("kf1", fe, pt, dict(max_candidates=65), th=20.0))
    pt = _Pts()
    for k in range(25):
        pt.add(30 * k, 100, flag=0)
    subs.append(mk("kf2", _Feats(), pt, {}, th=20.0))
    fe = _Feats(); fe.add(100, 100, 1, 10); fe.add(200, 100, 1, 10)
    subs.append(mk("kf3", fe, _Pts(), {}, th=20.0))
    return dict(name="batch_" + kind, kind=kind + "_batch", subs=subs, forces={})


def small_cases():
    """The cases whose answers tests/test_window_matcher_cases_cpu.py writes down by hand."""
    return [area_radius_edge(), area_zero_outside_whole(), area_max_x(), area_half_cells(), area_levels(),
            proj_tie_order(), sim3_tie_order(), frame_tie_order(), fuse_tie_order(),
            proj_thresholds(), sim3_thresholds(), frame_thresholds(64), frame_thresholds(100), fuse_thresholds(50), fuse_thresholds(100),
            fuse_chi2(), proj_order_a(), proj_order_b(), proj_order_cd(), sim3_order_e(),
            frame_hist_ties(), frame_hist_tenth(10), frame_hist_tenth(11), by_sim3_agreement(), init_basic()]


def size_cases():
    """The kernel-size cases: closed-form answers (see the test), point counts and candidate counts at every boundary of the kernels."""
    out = []
    for kind in ("projection", "sim3", "frame"):
        for n in SIZE_POINTS:
            if kind == "projection" or n in (65, 1025):             # the chain at every size in mode 0 (two candidates looked at), the other
                out.append(size_chain(kind, n))                     # modes of the same kernel past one wave and past one batch
            out.append(size_sparse(kind, n))
        out.append(cand_counts(kind, (0, 1, 16, 17, 64)))
        out.append(cand_counts(kind, (65, 17, 1)))
        out.append(cand_counts(kind, (200, 16)))
    for kind in ("projection", "sim3", "frame", "fuse"):
        out.append(cand_positions(kind, (15, 16, 17))); out.append(cand_positions(kind, (63, 64, 65)))
    out.append(cand_counts("fuse", CLUSTER_SIZES))
    return out


def all_cases():
    return small_cases() + size_cases()


def run_ref(case, *, wrong=(), trace=None):
    """The case through the definition.  area: a list of index lists; the others: the function's tuple; batches: a list of tuples."""
    kw = dict(wrong=wrong, trace=trace)
    k, a = case["kind"], case.get("args")
    if k.endswith("_batch"):
        return [run_ref(s, **kw) for s in case["subs"]]
    if k == "by_sim3":
        g1, g2 = R.Grid(**case["grid1"]), R.Grid(**case["grid2"])
        return R.search_by_sim3(g1, a["sf1"], g2, a["sf2"], a["valid1"], a["u1"], a["v1"], a["level1"], a["mp_desc1"], a["valid2"], a["u2"], a["v2"],
                                a["level2"], a["mp_desc2"], a["th"], **kw)
    g = R.Grid(**case["grid"])
    if k == "area":
        return [R.features_in_area(g, *q, **kw) for q in a["queries"]]
    if k == "init":
        return R.search_for_initialization(a["oct1"], a["desc1"], a["angle1"], g, a["prev_matched"], a["window"], a["nnratio"], a["check_ori"], **kw)
    fn = dict(projection=R.search_by_projection, sim3=R.search_by_projection_sim3, frame=R.search_by_projection_frame, fuse=R.fuse_select)[k]
    return fn(g, *a.values(), **kw)
