"""Table views (ccm_map_table_attach, include/ccm_hot.h "map-point table"): what sharing costs a table nobody shares, what a view buys
a second context, and what two contexts on one table's rows do to each other's latency.

  (a) the unshared path against the parent commit: ccm_frame_search_local_points (a 20,000-point map, 1,000 features),
      ccm_fuse_select_table_frames (20 keyframes x 1,000 points and 40 x 4,000) and ccm_map_table_refresh (2,500 points with
      descriptor and normal / depth and a result; 20,000 points, normal / depth, positions given, no result, then a synchronisation) on a
      table nobody attached to -- the sizes of tools/bench_search_local_points.py, bench_fuse_table.py and bench_map_refresh.py.  Each
      build runs in a process of its own, the two alternating ROUNDS times; only the C calls are timed.  The parent's process imports the
      package from a checkout of the parent commit with its library built (--parent-root): the Python binding asks the library for
      every symbol it lists, so CCM_HOT_LIB alone cannot put the parent's library under this tree's binding.  The bar: this build's
      median is at most the parent's plus the larger of 5 % and the parent's own p10-p90 spread.
  (b) the LocalMapping-shaped sequence -- refresh 1,000 points, then Fuse them into 20 keyframes -- through a view of a second context,
      against the same sequence on a table of that context's own, and against the route a second thread had before views existed: the
      host projection (tests/fuse_table_ref.py fuse_gates in numpy, standing in for the reference's per-point loop; timed separately)
      and ccm_fuse_select_batch_frames.  (The host route of the refresh is what tools/bench_map_refresh.py measures.)
  (c) contention: the tracking call (ccm_frame_search_local_points and ccm_frame_pose_optimize_table on the table's own handle) alone,
      and while a second thread issues (b)'s sequence through a view as fast as it can.  Median and p99.  Reported, not gated.
Output: profiles/shared_table.json and one summary line.

    python tools/bench_shared_table.py [--parent-root CHECKOUT] [--rounds 3] [--reps 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a worker of measurement (a) imports the package, and with it the library, from the checkout it is given
PKG_ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[:-1] else ROOT
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, PKG_ROOT)

import numpy as np  # noqa: E402

import fuse_table_ref as R  # noqa: E402
import map_refresh_ref as MR  # noqa: E402
import search_local_points_ref as S  # noqa: E402
from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable  # noqa: E402

COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
p = _lib.ptr


def stats(ts, p99=False):
    t = np.asarray(ts) * 1e3
    out = {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
           "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}
    if p99:
        out["p99_ms"] = round(float(np.percentile(t, 99)), 4)
    return out


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return ts


# ------------------------------------------------------------------------------------------------------------------ the calls
class Slp:
    """ccm_frame_search_local_points and the pose on a frame of 1,000 synthetic features over a map whose first 1,000 points were made
    for them; the rows lie in the slots [off, off + M) of `table`."""

    def __init__(self, ctx, M=20000):
        self.ctx, self.lib = ctx, _lib.load()
        f = R.synthetic_features(1000, 5)
        self.cam = S.camera()
        self.rows = S.concat(S.matchable_points(f["kx"], f["ky"], f["oct"], f["desc"], *self.cam, seed=4), S.random_points(M - 1000, 2))
        self.ids0 = np.where(np.random.default_rng(6).random(1000) < 0.3, np.arange(1000), -1).astype("i4")
        self.frame = DeviceFrame(FrameGridView(f["kx"], f["ky"], f["oct"], f["desc"]), None, ctx=ctx)

    def bind(self, table, off=0):
        self.table = table
        table.update(np.arange(len(self.rows["flags"])) + off, **self.rows)
        self.ids = np.where(self.ids0 >= 0, self.ids0 + off, -1).astype("i4")
        cap, n = table.capacity, 1000
        q = _lib.SlpParams()
        q.Tcw[:] = [float(v) for v in self.cam[0].reshape(-1)]; q.Ow[:] = [float(v) for v in self.cam[1]]
        q.fx, q.fy, q.cx, q.cy = S.INTR
        q.min_x, q.max_x, q.min_y, q.max_y = S.BOUNDS
        q.viewing_cos_limit = 0.5; q.log_scale_factor = float(S.LOG_SF); q.n_levels = S.N_LEVELS; q.scale_factors = S.SCALE.ctypes.data
        q.th = 1.0; q.nnratio = 0.8
        self.keep = [np.zeros(cap, "i4"), np.zeros(n, "i4"), np.zeros(n, "i4"), np.zeros(n, np.uint8), np.zeros(n, np.uint8)]
        self.par, self.res = q, _lib.SlpResult(0, cap, p(self.keep[0]), None, None, None, None, p(self.keep[1]), p(self.keep[2]), p(self.keep[3]))
        self.pose0 = np.zeros(7)
        T16 = np.concatenate([self.cam[0], np.array([[0, 0, 0, 1]], "f4")]).copy()
        assert self.lib.ccm_pose_from_mat4f(p(T16), p(self.pose0)) == 0
        self.pose0[4:] += [0.02, -0.01, 0.03]
        self.intr = np.array(S.INTR, "f8"); self.ninl = np.zeros(1, "i4")

    def search(self):
        c = self.ctx
        return c.check(self.lib.ccm_frame_search_local_points(c.handle, C.c_void_p(self.frame.handle), C.c_void_p(self.table.handle), C.byref(self.par),
                                                              C.byref(self.res)))

    def pose(self):
        c = self.ctx
        pose = self.pose0.copy()
        c.check(self.lib.ccm_frame_pose_optimize_table(c.handle, C.c_void_p(self.frame.handle), C.c_void_p(self.table.handle), p(R.INV_SIGMA2), R.N_LEVELS,
                                                       p(self.intr), p(pose), p(self.keep[4]), p(self.ninl)))

    def reset(self):
        self.frame.map_points = self.ids


class Mapping:
    """LocalMapping's work on n_kf keyframes of 1,000 synthetic features and n_points map points (bench_fuse_table.py's workload): the
    refresh of those points from random observations, then Fuse of the same list into every keyframe."""

    def __init__(self, ctx, n_kf, n_points, par, seed=11):
        self.ctx, self.lib, self.par_d = ctx, _lib.load(), par
        rng = np.random.default_rng(seed)
        cams = [S.camera(tuple(rng.normal(0, 0.04, 3)), tuple(np.array([2.5, -1.5, 1.5]) + rng.normal(0, 0.4, 3))) for _ in range(n_kf)]
        n_match = int(0.6 * n_points / n_kf)
        self.sc = sc = R.make_scene([R.synthetic_features(1000, seed + 1 + k) for k in range(n_kf)], n_points, n_match, n_match // 5, seed=seed, cams=cams)
        self.n_kf, self.n_points, self.m = n_kf, n_points, n_kf * n_points
        self.handles = []
        for kf in sc["kfs"]:
            h = DeviceFrame(FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"]), None, ctx=ctx)
            h.map_points = kf["mp_id"]
            h.set_camera(np.array(R.INTR, "f4"), R.SCALE, (R.SCALE * R.SCALE).astype("f4")); h.set_pose(kf["Tcw"], kf["Ow"])
            self.handles.append(h)
        counts = rng.integers(2, 15, n_points).astype("i4")
        self.first = np.concatenate([[0], np.cumsum(counts)]).astype("i4")
        self.okf = np.concatenate([rng.permutation(n_kf)[:c] for c in counts]).astype("i4")
        self.ofeat = rng.integers(0, 1000, self.first[-1]).astype("i4")
        self.rkf = self.okf[self.first[:-1]].copy(); self.rfeat = self.ofeat[self.first[:-1]].copy()
        self.slots = np.ascontiguousarray(sc["slots"], "i4")

    def bind(self, table, what=3, result=True):
        self.table = table
        sc, n_kf, n = self.sc, self.n_kf, self.n_points
        live = np.flatnonzero(sc["rows"]["flags"] & R.LIVE)
        table.update(live, **{k: sc["rows"][k][live] for k in COLS})
        self.views = (_lib.FuseView * n_kf)()
        for k, kf in enumerate(sc["kfs"]):
            V = self.views[k]
            V.kf = self.handles[k].handle
            V.Tcw[:] = [float(x) for x in kf["Tcw"].reshape(-1)]; V.Ow[:] = [float(x) for x in kf["Ow"]]
            V.fx, V.fy, V.cx, V.cy = R.INTR
            V.min_x, V.max_x, V.min_y, V.max_y = R.BOUNDS
        d = self.par_d
        self.prob = _lib.FuseTableProblem(n_kf, self.views, n, p(self.slots), None, float(R.LOG_SF), R.N_LEVELS, p(R.SCALE), p(R.INV_SIGMA2), float(d["th"]),
                                          int(d["chi2_check"]), int(d["accept_th"]))
        self.b_idx = np.empty(self.m, "i4"); self.b_dist = np.empty(self.m, "i4")
        self.fres = _lib.FuseTableResult(p(self.b_idx), p(self.b_dist), None, None, None, None, 0)
        self.harr = (C.c_void_p * n_kf)(*[h.handle for h in self.handles])
        self.rprob = _lib.MapRefresh(n, p(self.slots), None, None, n_kf, self.harr, p(self.first), p(self.okf), p(self.ofeat), p(self.rkf), p(self.rfeat), int(what))
        self.rout = [np.zeros(n, "i4"), np.zeros((n, 3), "f4"), np.zeros(n, "f4"), np.zeros(n, "f4")]
        self.rres = _lib.MapRefreshResult(*[p(a) for a in self.rout]) if result else None

    def fuse(self):
        c = self.ctx
        c.check(self.lib.ccm_fuse_select_table_frames(c.handle, C.c_void_p(self.table.handle), C.byref(self.prob), C.byref(self.fres)))

    def refresh(self):
        c = self.ctx
        c.check(self.lib.ccm_map_table_refresh(c.handle, C.c_void_p(self.table.handle), C.byref(self.rprob), C.byref(self.rres) if self.rres else None))
        if not self.rres:
            c.sync()

    def close(self):
        for h in self.handles:
            h.close()


# ------------------------------------------------------------------------------------------------------------------ (a)
def worker(reps, warmup):
    """The unshared calls with the package and library of --package-root; one JSON line of raw times in seconds."""
    ctx = _lib.default_context(0)
    out = {}
    s = Slp(ctx)
    with MapPointTable(20000, ctx=ctx) as t:
        s.bind(t)

        def slp():
            s.search()
        ts = []
        for r in range(warmup + reps):
            s.reset(); ctx.sync()
            t0 = time.perf_counter(); slp(); ts.append(time.perf_counter() - t0)
        out["search_local_points_20000"] = ts[warmup:]
    s.frame.close()
    for name, n_kf, n_points, par in (("fuse_local_mapping_20x1000", 20, 1000, R.PARAMS[0]), ("fuse_loop_closing_40x4000", 40, 4000, R.PARAMS[1])):
        mp = Mapping(ctx, n_kf, n_points, par)
        with MapPointTable(mp.sc["capacity"], ctx=ctx) as t:
            mp.bind(t)
            out[name] = timed(mp.fuse, reps, warmup)
        mp.close()
    for name, n_points, what, give_pos in (("refresh_local_mapping_2500", 2500, 3, False), ("refresh_local_ba_20000", 20000, MR.NORMAL_DEPTH, True)):
        mp = Mapping(ctx, 20, n_points, R.PARAMS[0], seed=7)
        with MapPointTable(mp.sc["capacity"], ctx=ctx) as t:
            mp.bind(t, what=what, result=not give_pos)
            if give_pos:
                pos = np.ascontiguousarray(mp.sc["rows"]["pos"][mp.slots]); mp.keep_pos = pos
                mp.rprob.pos = pos.ctypes.data
            out[name] = timed(mp.refresh, reps, warmup)
        mp.close()
    print("RAW " + json.dumps(out), flush=True)


def against_parent(a):
    roots = {"parent": os.path.abspath(a.parent_root), "this": ROOT}
    raw = {k: {} for k in roots}
    for r in range(a.rounds):
        for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps), "--warmup", str(a.warmup),
                                  "--package-root", roots[who]], capture_output=True, text=True, timeout=240)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("RAW ")]
            if res.returncode or not line:
                raise SystemExit("worker with the %s build failed (%d):\n%s" % (who, res.returncode, res.stderr[-2000:]))
            for k, v in json.loads(line[0][4:]).items():
                raw[who].setdefault(k, []).extend(v)
    out, ok = {}, True
    for k in raw["this"]:
        sp, st = stats(raw["parent"][k]), stats(raw["this"][k])
        margin = max(0.05 * sp["median_ms"], sp["p90_ms"] - sp["p10_ms"])
        within = st["median_ms"] <= sp["median_ms"] + margin
        ok &= within
        out[k] = {"parent": sp, "this": st, "margin_ms": round(margin, 4), "this_over_parent": round(st["median_ms"] / sp["median_ms"], 4), "within_bar": bool(within)}
        print("(a) %-28s parent %.4f ms [%.4f, %.4f] | this %.4f ms [%.4f, %.4f] | ratio %.3f | %s" % (
            k, sp["median_ms"], sp["p10_ms"], sp["p90_ms"], st["median_ms"], st["p10_ms"], st["p90_ms"], out[k]["this_over_parent"],
            "within the bar" if within else "OUTSIDE the bar"), flush=True)
    return {"rounds": a.rounds, "calls": out, "all_within_bar": bool(ok)}


# ------------------------------------------------------------------------------------------------------------------ (b), (c)
def view_and_contention(a):
    ctx_a, ctx_b = _lib.default_context(0), _lib.Context(0)
    lib = _lib.load()
    n_kf, n_points, par = 20, 1000, R.PARAMS[0]
    mp = Mapping(ctx_b, n_kf, n_points, par)
    off = mp.sc["capacity"]
    trk = Slp(ctx_a)
    root = MapPointTable(off + 20000, ctx=ctx_a)
    trk.bind(root, off)
    view = root.attach(ctx_b)
    own = MapPointTable(off, ctx=ctx_b)
    result = {}

    def sequence():
        mp.refresh(); mp.fuse()
    mp.bind(own)
    t_own = timed(sequence, a.reps, a.warmup)
    mp.bind(view)
    ctx_b.sync()
    t_view = timed(sequence, a.reps, a.warmup)
    # the route without a view: the rows as the refresh left them come to the host once; the device's level where the restatement is ambiguous
    m = mp.m
    b_gate = np.empty(m, np.uint8); b_u = np.empty(m, "f4"); b_v = np.empty(m, "f4"); b_lvl = np.empty(m, "i4")
    res = _lib.FuseTableResult(p(mp.b_idx), p(mp.b_dist), p(b_gate), p(b_u), p(b_v), p(b_lvl), 0)
    ctx_b.check(lib.ccm_fuse_select_table_frames(ctx_b.handle, C.c_void_p(view.handle), C.byref(mp.prob), C.byref(res)))
    got = view.fetch(np.arange(off))
    sc = dict(mp.sc, rows={k: got[k] for k in COLS})
    g = R.fuse_gates(sc)
    level = np.ascontiguousarray(np.where(g["ambiguous"].ravel(), b_lvl, g["level"].ravel()), "i4")
    desc = np.ascontiguousarray(np.tile(sc["rows"]["desc"][mp.slots], (n_kf, 1)))
    first = (np.arange(n_kf + 1) * n_points).astype("i4")
    a_idx = np.empty(m, "i4"); a_dist = np.empty(m, "i4")
    t_proj, t_call = [], []

    def host_route():
        t0 = time.perf_counter()
        gg = R.fuse_gates(sc)
        t1 = time.perf_counter()
        valid = np.ascontiguousarray((gg["gate"] == R.SEARCHED).ravel(), np.uint8)
        uu = np.ascontiguousarray(gg["u"].ravel()); vv = np.ascontiguousarray(gg["v"].ravel())
        t2 = time.perf_counter()
        ctx_b.check(lib.ccm_fuse_select_batch_frames(ctx_b.handle, n_kf, mp.harr, p(R.SCALE), p(R.INV_SIGMA2), p(first), p(valid), p(uu), p(vv), p(level), p(desc),
                                                     C.c_float(par["th"]), int(par["chi2_check"]), int(par["accept_th"]), p(a_idx), p(a_dist)))
        t3 = time.perf_counter()
        t_proj.append(t1 - t0); t_call.append(t3 - t2)
    for _ in range(a.warmup + a.reps):
        host_route()
    mp.fuse()
    sv, so = stats(t_view), stats(t_own)
    result["b_view_route"] = {"keyframes": n_kf, "points": n_points, "refresh_then_fuse_through_view": sv, "refresh_then_fuse_on_own_table": so,
                              "host_projection_numpy": stats(t_proj[a.warmup:]), "fuse_select_batch_frames": stats(t_call[a.warmup:]),
                              "fuse_results_equal_host_route": bool((a_idx == mp.b_idx).all() and (a_dist == mp.b_dist).all()),
                              "gates_equal_restatement": bool((g["gate"].ravel() == b_gate).all()),
                              "view_over_own": round(sv["median_ms"] / so["median_ms"], 3)}
    print("(b) refresh + Fuse, %d kf x %d points: through a view %.3f ms [%.3f, %.3f] | own table %.3f ms | host projection %.3f ms + select_batch_frames %.3f ms" % (
        n_kf, n_points, sv["median_ms"], sv["p10_ms"], sv["p90_ms"], so["median_ms"], result["b_view_route"]["host_projection_numpy"]["median_ms"],
        result["b_view_route"]["fuse_select_batch_frames"]["median_ms"]), flush=True)

    # (c) the tracking call alone and under LocalMapping's traffic
    n_track = a.track

    def track(ts):
        for r in range(n_track + a.warmup):
            trk.reset(); ctx_a.sync()
            t0 = time.perf_counter(); trk.search(); trk.pose()
            if r >= a.warmup:
                ts.append(time.perf_counter() - t0)
    alone, busy = [], []
    track(alone)
    stop = threading.Event()
    laps, err = [0], []

    def traffic():
        try:
            while not stop.is_set():
                sequence(); laps[0] += 1
        except BaseException as e:  # noqa: BLE001
            err.append(e)
    th = threading.Thread(target=traffic, daemon=True)
    th.start()
    try:
        track(busy)
    finally:
        stop.set(); th.join(60)
    if err or th.is_alive():
        raise SystemExit("the mapping thread failed: %r" % (err or "still running"))
    sa, sb = stats(alone, True), stats(busy, True)
    result["c_contention"] = {"tracking_call": "search_local_points (%d-point table, 1000 features) + pose" % root.capacity, "alone": sa,
                              "with_refresh_and_fuse_through_a_view": sb, "mapping_sequences_meanwhile": laps[0],
                              "median_ratio": round(sb["median_ms"] / sa["median_ms"], 3), "p99_ratio": round(sb["p99_ms"] / sa["p99_ms"], 3)}
    print("(c) tracking call alone %.3f ms (p99 %.3f) | under refresh + Fuse through a view %.3f ms (p99 %.3f), %d sequences meanwhile" % (
        sa["median_ms"], sa["p99_ms"], sb["median_ms"], sb["p99_ms"], laps[0]), flush=True)
    view.close(); own.close(); root.close(); mp.close(); trk.frame.close(); ctx_b.close()
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built; without it measurement (a) is left out")
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--track", type=int, default=300, help="tracking calls per condition of (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_table.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.reps, a.warmup)
    result = {"workload": {"reps": a.reps, "warmup": a.warmup, "tracking_calls": a.track}}
    result["a_unshared_against_parent"] = against_parent(a) if a.parent_root else "not measured: no --parent-root"    # before this process opens the GPU
    result.update(view_and_contention(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    ra = result["a_unshared_against_parent"]
    print(json.dumps({"a_all_within_bar": ra["all_within_bar"] if isinstance(ra, dict) else None,
                      "b_view_ms": result["b_view_route"]["refresh_then_fuse_through_view"]["median_ms"],
                      "c_median_ratio": result["c_contention"]["median_ratio"], "c_p99_ratio": result["c_contention"]["p99_ratio"]}))
    return 0 if not isinstance(ra, dict) or ra["all_within_bar"] else 1


if __name__ == "__main__":
    sys.exit(main())
