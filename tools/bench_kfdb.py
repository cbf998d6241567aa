#!/usr/bin/env python3
"""Times ccm_kfdb_query on place-recognition shapes: databases of 1 000 and 5 000 keyframes of about 1 500 words over 10^6 word ids
(an ORBvoc-sized vocabulary; a 2 000-feature keyframe lands in about that many distinct words), queried with stored keyframes.

  call       host clock around ccm_kfdb_query (it synchronises before it returns): median [p10, p90] of --reps steady-state
             queries (nothing pending) after --warmup
  flush / kernel / download
             HIP events inside the same calls (ccm_kfdb_last_timing), medians; with nothing pending the flush is empty
  first      the one query that uploads the whole database (all adds pending): call time and its flush share
  bytes      what one query has to read from the arena, counted from the shapes: every entry's ids (4 bytes a word) and the values of
             the common words (8 bytes each), plus the query; over the kernel time that is the achieved bandwidth, given beside
             the HBM peak of MI355X_MICROARCH (8.0 TB/s spec, about 6.3 TB/s achievable).  The kernel is a search, not a stream:
             the figure says how far from memory-bound it is, not a share of a compute peak.

Half of every keyframe's words come from a popular twentieth of the vocabulary, so that keyframes share tens of words as they do in
a real map.  Output: profiles/kfdb.json and one summary line per database size.  Needs the GPU; nothing here runs on a CPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:
    import torch  # noqa: F401  (first, so that the library binds to the same HIP runtime as in the tests)
except ImportError:
    pass

from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.database import KeyFrameDatabase  # noqa: E402

HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3


def stats(ms):
    t = np.asarray(ms, "f8")
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def keyframe(rng, n_words, words):
    n = int(rng.integers(words - 200, words + 201))
    popular = rng.choice(n_words // 20, n // 2, replace=False)
    rest = n_words // 20 + rng.choice(n_words - n_words // 20, n - n // 2, replace=False)
    ids = np.sort(np.concatenate([popular, rest])).astype("i4")
    v = rng.uniform(0.05, 1.0, n)
    return ids, v / v.sum()


def run(ctx, n_entries, a):
    rng = np.random.default_rng(n_entries)
    db = KeyFrameDatabase(a.n_words, 1 << 20, ctx=ctx)                 # smaller than the data: the first flush also grows the arena
    t0 = time.perf_counter()
    for key in range(n_entries):
        db.add(key, *keyframe(rng, a.n_words, a.words))
    t_add = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = db.query(0)
    first_ms = (time.perf_counter() - t0) * 1e3
    first = db.last_timing()
    cap, used, live = db.arena()
    keys = [int(k) for k in rng.integers(0, n_entries, a.warmup + a.reps)]
    for k in keys[:a.warmup]:
        db.query(k)
    call, parts, read = [], [], []
    for k in keys[a.warmup:]:
        t0 = time.perf_counter()
        r = db.query(k)
        call.append((time.perf_counter() - t0) * 1e3)
        parts.append(db.last_timing())
        q_n = int(r.words[r.query_slot])
        read.append(live * 4 + int(r.words.sum()) * 8 + q_n * 12)
    parts = np.asarray(parts)
    kernel_ms = float(np.median(parts[:, 1]))
    bytes_read = float(np.median(read))
    tbs = bytes_read / (kernel_ms * 1e-3) / 1e12 if kernel_ms > 0 else 0.0
    out = {"entries": n_entries, "arena_words": live, "arena_capacity_words": cap, "add_us_per_entry": round(t_add / n_entries * 1e6, 2),
           "first_query": {"call_ms": round(first_ms, 3), "flush_ms": round(first[0], 3), "kernel_ms": round(first[1], 4), "download_ms": round(first[2], 4)},
           "call": stats(call), "flush": stats(parts[:, 0]), "kernel": stats(parts[:, 1]), "download": stats(parts[:, 2]),
           "common_words_per_entry": round(float(r.words.sum()) / n_entries, 1),
           "bytes_read_per_query": int(bytes_read), "achieved_TBps": round(tbs, 4),
           "share_of_hbm_peak": round(tbs / HBM_PEAK_TBS, 4), "share_of_hbm_achievable": round(tbs / HBM_ACHIEVABLE_TBS, 4)}
    print("kfdb %5d entries: call %.3f ms [%.3f, %.3f] = flush %.4f + kernel %.4f + download %.4f; %.2f MB read, %.3f TB/s (%.1f%% of %.1f TB/s); "
          "first query %.2f ms" % (n_entries, out["call"]["median_ms"], out["call"]["p10_ms"], out["call"]["p90_ms"], out["flush"]["median_ms"],
                                   out["kernel"]["median_ms"], out["download"]["median_ms"], bytes_read / 1e6, tbs, 100 * tbs / HBM_PEAK_TBS,
                                   HBM_PEAK_TBS, first_ms))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--entries", type=int, nargs="+", default=[1000, 5000])
    ap.add_argument("--words", type=int, default=1500, help="words per keyframe, +-200")
    ap.add_argument("--n-words", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb.json"))
    a = ap.parse_args()
    ctx = _lib.Context(0)                                              # raises without a GPU: there is no CPU path to time
    res = {"device": "MI355X", "words_per_entry": a.words, "n_words": a.n_words, "lds_query_words": _lib.load().ccm_kfdb_query_lds_words(),
           "hbm_peak_TBps": HBM_PEAK_TBS, "runs": [run(ctx, n, a) for n in a.entries]}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
