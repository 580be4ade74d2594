#!/usr/bin/env python3
"""Developer probe: gpcc_knn (gauspcc_amd.knn) on the test clouds of tests/knn_ref.py at 1 M points, the all-equal cloud, and 8 M uniform
points -- distCUDA2 end to end and kneighbors(., 4) timed with events on the stream, median of `reps` after warm-up, beside scipy's cKDTree
(16 workers, the same k) as the CPU baseline.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel table; with
GAUSPCC_DEV=1 GAUSPCC_KNN_STATS=1 the library prints the visited leaves and popped tree nodes per wave of every call on stderr (that mode
synchronises: time without it).
    python tools/knn_probe.py [reps] [--no-cpu]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gauspcc_amd.knn import distCUDA2, kneighbors  # noqa: E402
from tests.knn_ref import CLOUDS, make_cloud  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 10
cpu = "--no-cpu" not in sys.argv


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn):
    fn()
    fn()
    return statistics.median(timed(fn) for _ in range(reps))


cases = [(c, 1_000_000) for c in CLOUDS] + [("equal", 1_000_000), ("uniform", 8_000_000)]
for kind, n in cases:
    pts = np.full((n, 3), 0.25, np.float32) if kind == "equal" else make_cloud(kind, n)
    x = torch.tensor(pts, device="cuda")
    print(f"[case] {kind} {n}", file=sys.stderr, flush=True)
    row = {"cloud": kind, "points": n, "distCUDA2_ms": round(median_ms(lambda: distCUDA2(x)), 3)}
    if n == 1_000_000:
        row["kneighbors4_ms"] = round(median_ms(lambda: kneighbors(x, 4)), 3)
    if cpu and kind != "equal":
        from scipy.spatial import cKDTree

        t0 = time.perf_counter()
        cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4, workers=16)
        row["ckdtree16_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    print(json.dumps(row), flush=True)
    del x
    torch.cuda.empty_cache()
