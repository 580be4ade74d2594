#!/usr/bin/env python3
"""Developer probe: CAT-3DGS's multi-scale tri-plane features (gauspcc_amd.cat_triplane) beside the float32 torch formula they replace
(rounded plane copies, six grid_sample calls, cats and the level sum: tests/cat_triplane_ref.py), at N points, C = 72, resolution 167 per
axis, multipliers [1, 2]: forward alone and forward + backward, raw and quantised, on the contract path (plane gradients) and on the
normalize_aabb path (plane gradients and the coordinate gradient).  Both programs run on the same GPU in the same process, alternating,
timed with events on the stream after warm-up (median, min and max of `reps` iterations); each side's peak memory above what the inputs
hold is recorded too.  Prints one JSON line per case with the achieved share of HBM bandwidth of the forward's output write
(N 2 3 C 4 bytes over the forward's time; the peak is the 8 TB/s of the MI355X).
    python tools/cat_triplane_probe.py [reps] [N ...]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import cat_triplane_ref as ref  # noqa: E402
from gauspcc_amd.cat_triplane import ms_triplane_sample  # noqa: E402

HBM_PEAK = 8.0e12
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(a) for a in sys.argv[2:]] or [1_000_000]
C, RES, MULT = 72, (167, 167, 167), (1, 2)
dev = "cuda:0"
if not torch.cuda.is_available():
    sys.exit("cat_triplane_probe: no GPU (a timing taken without one says nothing)")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(fns):
    """{name: (median, min, max) ms, peak MiB above the resident inputs}; the candidates alternate within every repetition"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    peaks = {}
    for k, fn in fns.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}, peaks


for N in sizes:
    g = torch.Generator().manual_seed(N)
    xf = {k: v.to(dev) for k, v in ref.transform(7).items()}
    contract = tuple(xf[k] for k in ("pca_mean", "rotation", "variance", "aabb", "con_aabb"))
    pts = (torch.randn(N, 3, generator=g) * torch.tensor([1.5, 0.8, 1.1])).to(dev)
    grids = [[(torch.randn(1, C, H, W, generator=g) * 0.2).to(dev) for H, W in ref.plane_shapes(RES, (m,))] for m in MULT]
    go = torch.randn(N, len(MULT) * 3 * C, device=dev)
    out_bytes = N * len(MULT) * 3 * C * 4
    plain = {k: v.to(dev) for k, v in ref.plain_aabb().items()}
    for path, quantise in (("contract", False), ("contract", True), ("plain", False), ("plain", True)):
        con = path == "contract"
        kw = dict(contract=contract) if con else dict(aabb=plain["aabb"])

        def fwd(hip):
            with torch.no_grad():
                return ms_triplane_sample(pts, grids, 2, quantise, **kw) if hip else ref.torch_formula(pts, grids, 2, quantise, xf if con else plain, con)

        def fwd_bwd(hip):
            gs = [[p.detach().requires_grad_(True) for p in level] for level in grids]
            x = pts if con else pts.detach().requires_grad_(True)          # the plain path also returns the coordinate gradient
            out = ms_triplane_sample(x, gs, 2, quantise, **kw) if hip else ref.torch_formula(x, gs, 2, quantise, xf if con else plain, con)
            out.backward(go)

        row = {"N": N, "C": C, "resolution": RES[0], "multipliers": list(MULT), "path": path, "quantise": quantise, "reps": reps}
        print(f"[case] {N} {path} quantise={quantise}", file=sys.stderr, flush=True)
        t, peak = measure({"hip_fwd": lambda: fwd(True), "torch_fwd": lambda: fwd(False)})
        t2, peak2 = measure({"hip_fwd_bwd": lambda: fwd_bwd(True), "torch_fwd_bwd": lambda: fwd_bwd(False)})
        t.update(t2)
        peak.update(peak2)
        for k, (med, lo, hi) in t.items():
            row[f"{k}_ms"] = round(med, 3)
            row[f"{k}_ms_min_max"] = [round(lo, 3), round(hi, 3)]
            row[f"{k}_peak_mib"] = round(peak[k], 1)
        row["fwd_speedup"] = round(row["torch_fwd_ms"] / row["hip_fwd_ms"], 2)
        row["fwd_bwd_speedup"] = round(row["torch_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"], 2)
        row["fwd_output_write_share_of_hbm_peak"] = round(out_bytes / (row["hip_fwd_ms"] * 1e-3) / HBM_PEAK, 3)
        print(json.dumps(row), flush=True)
    del pts, grids, go
    torch.cuda.empty_cache()
