#!/usr/bin/env python3
"""Developer probe: the tri-plane context sampler (gauspcc_amd.triplane) beside the float32 torch formula it replaces (twelve grid_sample
calls in two Python loops, tests/triplane_ref.py), at N anchors, K = 4, C = 50, 256 x 256 planes, in the materialised (N, K, 3) and the
repeat (N, 3) x K form: forward, and forward + backward (plane and coordinate gradients), timed with events on the stream over `reps`
iterations after warm-up (median).  Prints one JSON line per case with the achieved share of HBM bandwidth of the forward's output write
(N K 3 C 4 bytes over the forward's time; the peak is the 8 TB/s of the MI355X).
    python tools/triplane_probe.py [reps] [N ...]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import triplane_ref as ref  # noqa: E402
from gauspcc_amd.triplane import triplane_sample  # noqa: E402

HBM_PEAK = 8.0e12
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(a) for a in sys.argv[2:]] or [200_000, 1_000_000]
K, C, R = 4, 50, 256
dev = "cuda:0"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn):
    for _ in range(3):
        fn()
    return statistics.median(timed(fn) for _ in range(reps))


for N in sizes:
    g = torch.Generator().manual_seed(N)
    mx, mn = ref.bounds(device=dev)
    anchors = ((torch.rand(N, 3, generator=g) * 2 - 1) * torch.tensor([0.8, 0.7, 2.2])).to(dev)
    planes = (torch.randn(3, C, R, R, generator=g) * 0.01).to(dev)
    near = (anchors[:, None, :] + torch.randn(N, K, 3, generator=g).to(dev) * 0.01).contiguous()
    go = torch.randn(N, K * 3 * C, device=dev)
    out_bytes = N * K * 3 * C * 4
    for form in ("materialised", "repeat"):
        co_dev = near if form == "materialised" else anchors
        co_ref = near if form == "materialised" else anchors.unsqueeze(1).repeat(1, K, 1)
        rep = None if form == "materialised" else K

        def fwd(hip):
            with torch.no_grad():
                return triplane_sample(planes, co_dev, mx, mn, ref.RADII, repeat=rep) if hip else ref.torch_formula(planes, co_ref, mx, mn, ref.RADII)

        def fwd_bwd(hip):
            p = planes.clone().requires_grad_(True)
            if hip:
                c = co_dev.clone().requires_grad_(True)
                out = triplane_sample(p, c, mx, mn, ref.RADII, repeat=rep)
            else:
                c = (near if form == "materialised" else anchors).clone().requires_grad_(True)
                out = ref.torch_formula(p, c if form == "materialised" else c.unsqueeze(1).repeat(1, K, 1), mx, mn, ref.RADII)
            out.backward(go)

        row = {"N": N, "K": K, "C": C, "planes": f"{R}x{R}", "form": form, "reps": reps}
        print(f"[case] {N} {form}", file=sys.stderr, flush=True)
        row["hip_fwd_ms"] = round(median_ms(lambda: fwd(True)), 3)
        row["torch_fwd_ms"] = round(median_ms(lambda: fwd(False)), 3)
        row["hip_fwd_bwd_ms"] = round(median_ms(lambda: fwd_bwd(True)), 3)
        row["torch_fwd_bwd_ms"] = round(median_ms(lambda: fwd_bwd(False)), 3)
        row["fwd_speedup"] = round(row["torch_fwd_ms"] / row["hip_fwd_ms"], 2)
        row["fwd_bwd_speedup"] = round(row["torch_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"], 2)
        row["fwd_output_write_share_of_hbm_peak"] = round(out_bytes / (row["hip_fwd_ms"] * 1e-3) / HBM_PEAK, 3)
        print(json.dumps(row), flush=True)
    del anchors, planes, near, go
    torch.cuda.empty_cache()
