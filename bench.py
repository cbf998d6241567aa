#!/usr/bin/env python3
"""Headline benchmark of the hot path (BASELINE.json metric).

A "step" is one pass over one batch: ORB-extract 256 synthetic 752x480 frames ALREADY RESIDENT IN HBM (8-level
pyramid, FAST + quadtree + rBRIEF, BASELINE config 2) and brute-force Hamming match every consecutive frame pair on
the device (config 3's kernel on the extracted descriptors).  `value` is features extracted+matched per second over
all ranks (frames are sharded by rank, weak scaling, no collective); `config.residency` says "device".

A plain run sets up, warms up, times --steps steps and prints the line; everything else is measured only with --full.
--dump-outputs DIR writes what the last timed step computed on rank 0 (keypoints, descriptors, counts, matches) as
float32 .npy files into DIR; the inputs are seeded, so two builds can be compared output for output.

With --full the same JSON line also carries, all measured in this run unless a field says where else it comes from:
  kernels         per-kernel milliseconds per step (a second pass of --steps steps with HIP events on)
  roofline        the slowest extraction kernel against the HBM roofline (HIP events on the library's stream)
  match_10k       config 3 at its stated size: 10,000 pairs of 1000x1000 descriptors, one launch (N=1 only)
  pcie_inclusive  the drop-in call with host buffers: 256 frames, and the single-frame latency Tracking sees (N=1 only)
  cpu_baseline    the CPU oracle on this box's host cores: 1 core like the reference, and all cores over frames
  gba             global BA on the 2000-keyframe / 200k-point graph (config 5; landmarks sharded over ranks, one RCCL
                  all-reduce per LM trial): LM iterations/s over the whole call and over the LM loop alone, per-phase
                  roofline figures, and the oracle timed on the same graph

    python bench.py --gpus 1 --steps 20 --warmup 3 [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FRAMES = 256
W, H = 752, 480
# algorithmic bytes per 752x480 frame, split by the stage that moves them
ALG_BYTES = {
    "k_pyr_resize": 360960 + 756407,                 # read level 0, write levels 1..7
    "k_fast_score": 1117367,                         # FAST reads every pyramid pixel once
    "k_fast_cells": 1117367,                         # fused score + per-cell NMS (the default path): same algorithmic read
    "k_cell_nms": 0, "k_octree": 0,                  # candidate lists: not in the survey's figure
    "k_orient_desc": 2234734 + 1982000,              # blur read+write (fused here) + 1000 kp patches/desc/kp
}
ALG_BYTES_FRAME = 6451468
MATCH_BYTES_PAIR = 76000                             # 64,000 in + 12,000 out per 1000x1000 pair
MATCH_WORDOPS_PAIR = 8e6                             # 10^6 distances x 8 32-bit xor+popcount words
HBM_PEAK_GBS = 8000.0                                # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec
FP64_MATRIX_PEAK_TF = 78.6                           # v_mfma_f64_16x16x4_f64: 256 CUs x 4 SIMDs x 32 flop/clk x 2.4 GHz
I8_MFMA_PEAK_TOPS = 5033.0                           # dense int8 MFMA (= fp8 rate, guide: ~5 PF dense)
BA_BYTES_PER_EDGE = 344                              # ~200 B read + 144 B written per edge and linearisation


def host_cores():
    try:
        return len(os.sched_getaffinity(0))
    except Exception:
        return os.cpu_count() or 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also measure per-kernel times and the roofline, match_10k, pcie_inclusive, the CPU baselines and global BA")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's results (rank 0) as float32 .npy files into DIR")
    ap.add_argument("--gba-iters", type=int, default=20, help="--full: LM iterations of the timed global-BA call (the reference's GBA runs 20)")
    ap.add_argument("--no-gba", action="store_true", help="--full: skip the global-BA leg")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the match_10k and pcie_inclusive legs")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # Rehearsal switches (a one-GPU box cannot host two RCCL ranks): CCM_BENCH_BACKEND=gloo moves the torch.distributed
    # control traffic to gloo and lets several ranks share a GPU, CCM_BENCH_COMM=shm replaces the library's RCCL all-reduce
    # by its shared-memory transport.  The driver's runs use neither.
    backend = os.environ.get("CCM_BENCH_BACKEND", "nccl")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    torch.cuda.set_device(local)
    red_dev = "cuda" if backend == "nccl" else "cpu"          # where the few scalars that cross ranks live

    from motioncheck_ccm_slam_amd import _lib, synth
    from motioncheck_ccm_slam_amd import dist as D
    from motioncheck_ccm_slam_amd.orb import ORBextractor

    lib = _lib.load()
    ctx = _lib.Context(local)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    m = ex.max_per_image
    solo = rank == 0 and world == 1                            # legs that describe one GPU / this box's host cores

    # ---- inputs resident in HBM before the timed region
    frames = synth.frames(rank * FRAMES, FRAMES)
    img_dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    n_pairs = FRAMES - 1
    bi = torch.empty((n_pairs, m), dtype=torch.int32, device="cuda")
    bd = torch.empty_like(bi); sd = torch.empty_like(bi)

    def step():
        ex.extract_dev(img_dev.data_ptr(), W, H, W, W * H, FRAMES)
        d_ptr, c_ptr, mm = ex.result_dev()
        ctx.check(lib.ccm_hamming_match_dev(ctx.handle, C.c_void_p(d_ptr), mm, C.c_size_t(mm), C.c_void_p(d_ptr + mm * 32), mm,
                                            C.c_size_t(mm), n_pairs, C.c_void_p(c_ptr), C.c_void_p(c_ptr + 4),
                                            C.c_void_p(bi.data_ptr()), C.c_void_p(bd.data_ptr()), C.c_void_p(sd.data_ptr())))

    def fence():
        ctx.sync(); torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    for _ in range(max(args.warmup, 1)):
        step()
    fence()
    _, _, counts = ex.fetch()
    feats = int(counts.sum())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    ctx.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        ft = torch.tensor([feats], dtype=torch.float64, device=red_dev)
        dist.all_reduce(ft)
        feats_all = float(ft.item())
        dist.barrier()
    else:
        feats_all = float(feats)
    ms_per_step = dt / args.steps * 1e3
    value = feats_all * args.steps / dt / 1e6

    # ---- what the last timed step computed, as a caller of the device path receives it (before any further step runs).  Rows past
    # a frame's keypoint count are filled (0 for keypoints and descriptors, -1 for matches): memory the step did not write never
    # enters a comparison.  256 x 1096 keypoints as float32 come to 47 MB in all.
    if args.dump_outputs and rank == 0:
        kps, desc, counts = ex.fetch()
        valid = np.arange(m)[None, :] < counts[:, None]
        kp = np.stack([kps[name].astype(np.float32) for name in kps.dtype.names], axis=-1)    # x y size angle response octave class_id
        dump = {"counts": counts.astype(np.float32),
                "keypoints": np.where(valid[..., None], kp, np.float32(0)),
                "descriptors": np.where(valid[..., None], desc, 0).astype(np.float32)}       # one byte per element
        for name, t in (("match_best_idx", bi), ("match_best_dist", bd), ("match_second_dist", sd)):
            dump[name] = np.where(valid[:n_pairs], t.cpu().numpy(), -1).astype(np.float32)  # pair p: frame p's queries
        assert sum(a.nbytes for a in dump.values()) <= 64 << 20
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in dump.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)

    # ---- per-kernel durations: HIP events on the stream the kernels are launched on
    kern = roofline = None
    if args.full:
        ctx.profile(True)
        for _ in range(args.steps):
            step()
        prof = ctx.profile_read()
        ctx.profile(False)
        kern = {}
        for k, (ms, n) in prof.items():
            if n:
                per_step = ms / args.steps
                kern[k] = {"ms_per_step": round(per_step, 4), "launches_per_step": n // args.steps}
        if "k_cell_nms" not in kern and "k_fast_score" in kern:      # the fused kernel is timed under the score label
            kern["k_fast_cells"] = kern.pop("k_fast_score")
        if "k_hamming_bf" in kern and m <= 2048 and os.environ.get("CCM_BF_VARIANT", "3") == "3":
            kern["k_hamming_mfma"] = kern.pop("k_hamming_bf")        # <= 2048 train rows: the matrix-core kernel runs under this label
        dom = max((k for k in kern if k in ALG_BYTES), key=lambda k: kern[k]["ms_per_step"])
        dom_bytes = ALG_BYTES[dom] * FRAMES
        dom_s = kern[dom]["ms_per_step"] * 1e-3
        achieved = dom_bytes / dom_s / 1e9 if dom_s > 0 else 0.0
        traffic = None
        pmc = {}
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tpath):
            try:
                pmc = json.load(open(tpath)).get(dom, {})
                traffic = pmc.get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        extract_ms = sum(v["ms_per_step"] for k, v in kern.items() if not k.startswith("k_hamming"))
        roofline = {"kernel": dom, "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                    # traffic and the issue figures are NOT measured in this run: they are read from the committed rocprofv3 --pmc
                    # passes of this same command (separate FETCH_SIZE / WRITE_SIZE / SQ passes, tools/profile_round.sh)
                    "traffic_from": "profiles/pmc_traffic.json" if traffic is not None else None,
                    "algorithmic_bytes_per_launch": dom_bytes,
                    # vector-issue occupancy of the same kernel: SQ_INSTS_VALU x c / (1024 SIMDs x busy cycles) with c = 2.3 cycles
                    # (every instruction full rate) and c = 4.2 (every instruction a packed / 3-operand one); the two costs are
                    # measured, profiles/r02_valu_issue_calibration.txt
                    "valu_issue_frac_bounds": pmc.get("valu_issue_frac_bounds"), "valu_issue_frac_from": "profiles/pmc_traffic.json",
                    "pipeline_algorithmic_GBps": round(ALG_BYTES_FRAME * FRAMES / (extract_ms * 1e-3) / 1e9, 2) if extract_ms else None}

    # ---- config 3 at its stated size: 10,000 independent 1000x1000 pairs, descriptors resident in HBM, one launch
    match10k = None
    if args.full and solo and not args.no_extra:
        NP = 10000
        qa, tb = synth.descriptor_pairs_torch(0, NP, device="cuda")
        b10 = torch.empty((NP, 1000), dtype=torch.int32, device="cuda"); d10 = torch.empty_like(b10); s10 = torch.empty_like(b10)

        def match_all():
            ctx.check(lib.ccm_hamming_match_dev(ctx.handle, C.c_void_p(qa.data_ptr()), 1000, C.c_size_t(1000), C.c_void_p(tb.data_ptr()), 1000,
                                                C.c_size_t(1000), NP, None, None, C.c_void_p(b10.data_ptr()), C.c_void_p(d10.data_ptr()),
                                                C.c_void_p(s10.data_ptr())))
        match_all(); ctx.sync()
        reps = 5
        ctx.profile(True)
        tm = time.perf_counter()
        for _ in range(reps):
            match_all()
        ctx.sync()
        wall = (time.perf_counter() - tm) / reps
        ms10, _n = ctx.profile_read()["k_hamming_bf"]
        ctx.profile(False)
        ms10 /= reps
        matched = int(((d10 <= 50) & (d10.to(torch.float32) < 0.7 * s10.to(torch.float32))).sum().item())
        # matrix-core work of the kernel: per 32-train x 32-query tile 8 v_mfma_i32_32x32x32_i8 (k = 256 bits), 65,536 MACs each
        macs = NP * (1024 / 32) * (1000 / 32 + (1 if 1000 % 32 else 0)) * 8 * 32 * 32 * 32
        match10k = {"workload": "configs[2]: 10,000 pairs, 1000 query x 1000 train 256-bit descriptors each (seeds 0xDE5C0000+p), "
                                "best/second-best/index per query, device-resident", "pairs": NP,
                    "ms_per_launch": round(ms10, 4), "wall_ms_per_call": round(wall * 1e3, 4),
                    "pairs_per_s": round(NP / (ms10 * 1e-3), 1), "Mqueries_per_s": round(NP * 1000 / (ms10 * 1e-3) / 1e6, 2),
                    "Tdistances_per_s": round(NP * 1e6 / (ms10 * 1e-3) / 1e12, 3),
                    "word_ops_per_s": round(NP * MATCH_WORDOPS_PAIR / (ms10 * 1e-3), 0),
                    "algorithmic_GBps": round(NP * MATCH_BYTES_PAIR / (ms10 * 1e-3) / 1e9, 2),
                    "mfma_int8_Tops": round(2 * macs / (ms10 * 1e-3) / 1e12, 1), "mfma_int8_peak_Tops": I8_MFMA_PEAK_TOPS,
                    "mfma_frac": round(2 * macs / (ms10 * 1e-3) / 1e12 / I8_MFMA_PEAK_TOPS, 4),
                    "accepted_by_ratio_test": matched}
        del qa, tb, b10, d10, s10
        torch.cuda.empty_cache()

    # ---- the drop-in call with host buffers (what cslam::ORBextractor::operator() hands over): PCIe both ways included
    pcie = None
    if args.full and solo and not args.no_extra:
        ex.extract_batch(frames)                                   # first touch of the library's staging
        ts = []
        for _ in range(5):
            t1 = time.perf_counter(); _k, _d, cnt = ex.extract_batch(frames); ts.append(time.perf_counter() - t1)
        tb_ = float(np.median(ts))
        one = frames[0:1]
        lat = []
        ex.extract_batch(one)
        for i in range(100):
            t1 = time.perf_counter(); ex.extract_batch(one); lat.append(time.perf_counter() - t1)
        lat = np.asarray(lat) * 1e3
        # the same batch from a page-locked frame pool (ccm_host_register: what a server re-using its buffers would do)
        reg_ms = None
        pool_ms = None
        try:
            ctx.host_register(frames)
            ex.extract_batch(frames)
            ts2 = []
            for _ in range(5):
                t1 = time.perf_counter(); ex.extract_batch(frames); ts2.append(time.perf_counter() - t1)
            reg_ms = round(float(np.median(ts2)) * 1e3, 3)
            # ... and page-locked result pools as well: each 64-frame chunk's keypoints and descriptors go down while the next
            # chunk is extracted (round 3)
            outs = ex.extract_batch(frames)
            for a in outs:
                ctx.host_register(a)
            ex.extract_batch(frames, out=outs)
            ts3 = []
            for _ in range(5):
                t1 = time.perf_counter(); ex.extract_batch(frames, out=outs); ts3.append(time.perf_counter() - t1)
            pool_ms = round(float(np.median(ts3)) * 1e3, 3)
            for a in outs:
                ctx.host_unregister(a)
            ctx.host_unregister(frames)
        except Exception as e:
            reg_ms = reg_ms if reg_ms is not None else "failed: %s" % e
            pool_ms = pool_ms if pool_ms is not None else "failed: %s" % e
        pcie = {"batch256_ms": round(tb_ * 1e3, 3), "batch256_Mfeatures_per_s": round(float(cnt.sum()) / tb_ / 1e6, 2),
                "batch256_registered_input_ms": reg_ms, "batch256_registered_input_and_output_ms": pool_ms,
                "batch256_note": "ccm_orb_extract with pageable host frames in (92 MB) and host keypoints+descriptors out (17 MB); "
                                 "extraction only, no matching; median of 5 calls",
                "single_frame_latency_ms": {"median": round(float(np.median(lat)), 4), "p90": round(float(np.percentile(lat, 90)), 4),
                                            "min": round(float(lat.min()), 4), "calls": 100},
                "single_frame_note": "n_images = 1, host image in, host keypoints+descriptors out: what Tracking calls per frame "
                                     "(src/Frame.cpp:120-123)"}

    # ---- CPU oracle on this box's host cores (rank 0, N=1 only): the same batch, one core like the reference, then all cores
    cpu = None
    cpu_all = None
    if args.full and solo and not args.no_cpu:
        from oracle import oracle_py as O
        par = O.default_params()
        t1 = time.perf_counter()
        n_cpu = 0
        descs = []
        for f in range(FRAMES):
            r = O.orb_extract(par, frames[f])
            n_cpu += len(r["kps"]); descs.append(r["desc"])
        t2 = time.perf_counter()
        for f in range(FRAMES - 1):
            O.hamming_match(descs[f], descs[f + 1])
        t3 = time.perf_counter()
        cpu = {"value": round(n_cpu / (t3 - t1) / 1e6, 5), "unit": "Mfeatures/s", "cores": 1, "kind": "port",
               "sample": "the same %d frames + %d consecutive-pair matches, scalar C oracle on 1 core "
                         "(extract %.2f s, match %.2f s); host has %d cores" % (FRAMES, FRAMES - 1, t2 - t1, t3 - t2, host_cores())}
        # all cores: the same frames (then pairs) dealt to one POSIX thread per usable core INSIDE the oracle (no Python in the loop)
        nthr = max(1, min(host_cores(), FRAMES))
        n_all, t_ex, t_ma = O.bench_extract_match_mt(par, frames, nthr)
        cpu_all = {"value": round(n_all / (t_ex + t_ma) / 1e6, 5), "unit": "Mfeatures/s", "cores": nthr, "kind": "port",
                   "sample": "the same %d frames + %d pair matches dealt to %d pthreads inside the C oracle (one per usable core: "
                             "sched_getaffinity = %d, os.cpu_count = %d); extract %.3f s, match %.3f s; with one frame per core the wall "
                             "time is one frame's time, so this is the latency-bound best case of the batch"
                             % (FRAMES, FRAMES - 1, nthr, host_cores(), os.cpu_count() or 0, t_ex, t_ma)}

    # ---- global BA (config 5): LM iterations per second.  Runs in a worker thread with a deadline: with N > 1 it
    # is the only part that talks over RCCL, and a communicator that never completes must not cost the
    # extract+match result (the thread cannot be cancelled, so on a timeout the process reports and hard-exits non-zero).
    gba_box = {}

    def run_gba():
        try:
            torch.cuda.set_device(local)                                # the current device is per thread
            from motioncheck_ccm_slam_amd.optimizer import Optimizer
            if world > 1:
                if os.environ.get("CCM_BENCH_COMM") == "shm":
                    from tests.support import shm_transport                 # rehearsal only: test scaffolding, not the product
                    shm_transport.attach(ctx, "/ccm_bench_%s" % os.environ.get("MASTER_PORT", "0"), rank, world)
                else:
                    D.init_comm(ctx, rank, world)
            g = synth.gba_graph()
            E = len(g["edge_pose"])
            # the map's edge arrays are page-locked once, as a server that keeps its graph buffers would (ccm_host_register);
            # three timed calls, the median is reported (pageable uploads were seen to take 1.5 or 19 ms from call to call)
            Optimizer.MapFusionGBA(g, 1, ctx=ctx)                       # warm-up (allocations, graph capture)
            # the same call from pageable edge arrays first (what a caller that does not page-lock its graph buffers gets): five calls, all reported
            pageable = []
            if world == 1:
                for _ in range(5):
                    tg = time.perf_counter(); Optimizer.MapFusionGBA(g, args.gba_iters, ctx=ctx); pageable.append(round(time.perf_counter() - tg, 4))
            for k in ("edge_pose", "edge_point", "obs", "info"):
                ctx.host_register(g[k])
            # ... and so are the pose / point arrays the solve reads its start values from and writes its results to (BaWorkspace:
            # the graph's values are copied into it inside the timed call)
            from motioncheck_ccm_slam_amd.optimizer import BaWorkspace
            ws = BaWorkspace(ctx, len(g["poses"]), len(g["points"]))
            Optimizer.MapFusionGBA(g, 1, ctx=ctx, workspace=ws)
            fence()
            calls = []
            for _ in range(3):
                tg = time.perf_counter()
                r = Optimizer.MapFusionGBA(g, args.gba_iters, ctx=ctx, workspace=ws)
                dt = time.perf_counter() - tg
                calls.append((dt, dict(r, poses=r["poses"].copy(), points=r["points"].copy())))     # (views of the workspace: kept outside the timed call)
            calls.sort(key=lambda c: c[0])
            call_s, r = calls[1]
            lm_s = r["t_linearize"] + r["t_schur"] + r["t_solve"] + r["t_update"]
            if world > 1:
                t = torch.tensor([lm_s, call_s], dtype=torch.float64, device=red_dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                lm_s, call_s = float(t[0]), float(t[1])
            its = max(r["iterations_done"], 1)
            gba = {"metric": "GBA LM iterations/s (2000 KF, 200k points, %d edges)" % E,
                   # headline: the whole call as the reference times optimize() (src/Optimizer.cpp:796-801 brackets buildStructure too)
                   "iter_per_s": round(r["iterations_done"] / call_s, 3),
                   "iter_per_s_lm_loop_only": round(r["iterations_done"] / lm_s, 3),
                   "iterations": r["iterations_done"], "iterations_requested": args.gba_iters, "trials": r["trials"],
                   "call_seconds": round(call_s, 4), "call_seconds_all": [round(c[0], 4) for c in calls], "timed_calls": "3, median reported",
                   "call_seconds_pageable_all": pageable,
                   "lm_seconds": round(lm_s, 4),
                   "setup_seconds": round(call_s - lm_s, 4),
                   "setup_note": "graph upload (edge, pose and point arrays page-locked by the caller), edge-list check and index on the device, pair enumeration, radix sorts, block pattern, PCG graph capture, result download",
                   "t_linearize": round(r["t_linearize"], 4), "t_schur": round(r["t_schur"], 4),
                   "t_solve": round(r["t_solve"], 4), "t_update": round(r["t_update"], 4),
                   "ms_per_iteration_lm": round(lm_s / its * 1e3, 3),
                   "schur_blocks": r["schur_blocks"], "schur_pairs_this_rank": r["schur_pairs"], "pcg_iterations": r["pcg_iterations"],
                   "chi2_initial": r["chi2_initial"], "chi2_final": r["chi2_final"], "n_gpus": world, "scaling": "strong",
                   "dtype": "f64",
                   "pcg_pipelined": r.get("pcg_pipelined", 0), "pcg_fallbacks": r["pcg_fallbacks"],
                   "reduced_solve": "pipelined PCG (Ghysels-Vanroose: two kernels per iteration), cluster + coarse level, relative residual 1e-6 per trial "
                                    "(ccm_ba_options.pcg_tol default; final poses within 1e-8 of the exact-solve oracle on this graph, contract 1e-5: "
                                    "tests/test_ba_gpu.py)"}
            # per-phase roofline figures of this rank: a second call with the library's event profiling on (HIP events on its stream)
            ctx.profile(True)
            rp = Optimizer.MapFusionGBA(g, 5, ctx=ctx)
            pr = ctx.profile_read()
            ctx.profile(False)
            fixed = np.asarray(g["fixed"]).astype(bool)
            k_free = np.bincount(g["edge_point"][~fixed[g["edge_pose"]]], minlength=len(g["points"])).astype(np.float64)
            schur_flops = float((2.0 * (9 + 72 * k_free + 54 * k_free * (k_free + 1)) + 60).sum()) / world      # this rank's share
            roof = {"from": "HIP events of a 5-iteration call of this run (ccm_profile_*); rocprofv3 traces and PMC of the same kernels: profiles/r03*_gba_*, profiles/r02*_gba_*"}
            ms_s, n_s = pr["k_sp_schur_blocks"]
            if n_s:
                tf = schur_flops / (ms_s / n_s * 1e-3) / 1e12
                roof["schur"] = {"kernel": "k_sp_schur_blocks", "bound": "mfma", "ms_per_trial": round(ms_s / n_s, 4),
                                 "algorithmic_GFLOP_per_trial": round(schur_flops / 1e9, 3), "achieved": round(tf, 3), "peak": FP64_MATRIX_PEAK_TF,
                                 "unit": "TFLOP/s", "frac": round(tf / FP64_MATRIX_PEAK_TF, 5),
                                 "gather_GBps": round(r["schur_pairs"] * 288.0 / (ms_s / n_s * 1e-3) / 1e9, 1),
                                 "gather_note": "pairs x 2 operand blocks x 144 B: what the GEMM's operands amount to if nothing is reused"}
            ms_l, n_l = pr["ba_linearize"]
            # (per LM iteration: the library brackets the landmark side and the keyframes' side separately when the latter is enqueued
            #  ahead of the LM decision, so the number of brackets is not the number of linearisations)
            n_l = rp["iterations_done"] if n_l else 0
            if n_l:
                gb = BA_BYTES_PER_EDGE * E / world / (ms_l / n_l * 1e-3) / 1e9
                roof["linearize"] = {"kernels": "k_ba_lin_landmark + k_ba_lin_pose", "bound": "hbm", "ms_per_iteration": round(ms_l / n_l, 4),
                                     "achieved": round(gb, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gb / HBM_PEAK_GBS, 5),
                                     "algorithmic_bytes": BA_BYTES_PER_EDGE * E // world}
            if rp["pcg_iterations"]:
                per_it = rp["t_solve"] / rp["pcg_iterations"]
                spmv_bytes = (2 * r["schur_blocks"] - 1999) * 288.0
                roof["solve"] = {"kernels": ("k_ppcg_prec + k_ppcg_row (HIP graphs)" if rp.get("pcg_pipelined") else
                                             "k_pcg_spmv + k_pcg_update + k_pcg_coarse + k_pcg_direction (HIP graphs)"), "bound": "hbm",
                                 "us_per_pcg_iteration_host_timed": round(per_it * 1e6, 2),
                                 "spmv_algorithmic_bytes": int(spmv_bytes), "achieved": round(spmv_bytes / per_it / 1e9, 1),
                                 "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(spmv_bytes / per_it / 1e9 / HBM_PEAK_GBS, 5),
                                 "note": "whole PCG iteration (its kernels, the per-trial set-up and the host round trips) charged to the mat-vec's bytes"}
            gba["roofline"] = roof
            if solo:
                # BASELINE config 4 beside it: the local BA Mapping runs per keyframe (20 free + 10 fixed keyframes, 5000 points, 5 robust + 10
                # plain iterations with outlier relabelling, src/Optimizer.cpp:536-568) -- a latency figure, host buffers in and out
                gl = synth.local_ba_graph()
                Optimizer.LocalBundleAdjustmentClient(gl, ctx=ctx)
                tl = []
                for _ in range(5):
                    t1 = time.perf_counter(); rl = Optimizer.LocalBundleAdjustmentClient(gl, ctx=ctx); tl.append(time.perf_counter() - t1)
                lb = {"workload": "configs[3]: 20 free + 10 fixed keyframes, 5000 points, %d edges, 5 + 10 LM iterations" % len(gl["edge_pose"]),
                      "ms_per_call": round(float(np.median(tl)) * 1e3, 3), "iterations": rl["iterations_done"], "outliers": int(rl["outlier"].sum())}
                if not args.no_cpu:
                    from oracle import oracle_py as O
                    t1 = time.perf_counter(); O.ba_solve(gl, 5, float(np.float32(np.sqrt(5.991))), 10); lb["cpu_oracle_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
                gba["local_ba"] = lb
            if solo and not args.no_cpu:
                from oracle import oracle_py as O
                tc = time.perf_counter()
                rc = O.ba_solve(g, 2, float(np.float32(np.sqrt(5.99))))
                tc = time.perf_counter() - tc
                gba["cpu_baseline"] = {"value": round(rc["iterations_done"] / tc, 4), "unit": "LM iterations/s", "cores": 1, "kind": "port",
                                       "sample": "config 5 itself (2000 KF / 200k points / %d edges), 2 LM iterations of the oracle incl. its one-off "
                                                 "minimum-degree ordering; reduced solve = block-sparse Cholesky (sparse + exact like g2o's "
                                                 "LinearSolverEigen), chi2 after 2 iterations %.6e" % (E, rc["chi2_final"])}
            for k in ("edge_pose", "edge_point", "obs", "info"):
                ctx.host_unregister(g[k])
            gba_box["gba"] = gba
        except Exception as e:  # the headline number must survive a communicator problem
            gba_box["gba"] = {"error": "%s: %s" % (type(e).__name__, e)}
            print("[bench rank %d] global BA failed: %s: %s" % (rank, type(e).__name__, e), file=sys.stderr, flush=True)

    gba = None
    timed_out = False
    if args.full and not args.no_gba:
        th = threading.Thread(target=run_gba, daemon=True)
        th.start()
        th.join(timeout=420.0)
        timed_out = th.is_alive()
        if timed_out:
            print("[bench rank %d] global BA did not finish within 420 s (stuck collective?)" % rank, file=sys.stderr, flush=True)
        gba = {"error": "timeout: global BA did not finish within 420 s"} if timed_out else gba_box.get("gba")

    if rank == 0:
        out = {
            "metric": "ORB extract+match Mfeatures/s and GBA iter/s (2k KF, 200k pts) @1/2/4/8 GPU",
            "value": round(value, 4), "unit": "Mfeatures/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": "configs[1]: 256 synthetic 752x480 frames per GPU, 8-level pyramid, 1000 features, "
                                   "FAST+quadtree+rBRIEF, then 1000x1000 brute-force Hamming on the 255 consecutive pairs",
                       "residency": "device (frames resident in HBM before the timed region, results left in HBM; "
                                    "the host-buffer call is the pcie_inclusive leg)",
                       "frames_per_gpu": FRAMES, "features_per_step_per_gpu": feats, "pairs_per_step_per_gpu": n_pairs},
            "roofline": roofline, "cpu_baseline": cpu, "cpu_baseline_all_cores": cpu_all, "kernels": kern,
            "match_10k": match10k, "pcie_inclusive": pcie, "gba": gba,
            "frames_per_s": round(FRAMES * world * args.steps / dt, 1),
        }
        print(json.dumps(out), flush=True)
    failed = bool(gba and "error" in gba)
    if timed_out:
        os._exit(3)                 # a stuck collective cannot be cancelled; the result line is already out, the exit code says it hung
    ctx.close()
    if world > 1:
        dist.destroy_process_group()
    if failed and world > 1:
        sys.exit(4)                 # a multi-rank global BA that failed is a failed run, not a line with an error field


if __name__ == "__main__":
    main()
