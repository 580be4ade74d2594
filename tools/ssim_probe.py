"""Times gauspcc_amd.loss_utils.ssim (gsr_ssim_forward / gsr_ssim_backward) against the reference's float32 torch formula
(tests/ssim_ref.py: ssim_torch32) in the same process, alternating, with device events, warm; one JSON line per (size, path, phase).

    python tools/ssim_probe.py [--iters 50] [--sizes 3x1060x1600,3x800x800]

Phases: fwd = the training forward (the graph is built; HIP also writes its derivative maps), bwd = the backward alone, step = both;
eval = the forward under torch.no_grad().  Times are medians over rounds of --iters calls each."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gauspcc_amd.loss_utils import ssim  # noqa: E402
from tests import ssim_ref  # noqa: E402


def _phase_times(fn, x, y, iters):
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    evals = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        a = x.detach().requires_grad_(True)
        e[0].record()
        s = fn(a, y)
        e[1].record()
        s.backward()
        e[2].record()
    evals[0].record()
    with torch.no_grad():
        for _ in range(iters):
            fn(x, y)
    evals[1].record()
    torch.cuda.synchronize()
    fwd = sum(e[0].elapsed_time(e[1]) for e in ev) / iters
    bwd = sum(e[1].elapsed_time(e[2]) for e in ev) / iters
    return {"fwd": fwd, "bwd": bwd, "step": fwd + bwd, "eval": evals[0].elapsed_time(evals[1]) / iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="3x1060x1600,3x800x800")
    args = ap.parse_args()
    paths = {"hip": ssim, "torch": ssim_ref.ssim_torch32}
    for size in args.sizes.split(","):
        shape = tuple(int(v) for v in size.split("x"))
        x, y = ssim_ref.make_images(shape, seed=1, device="cuda")
        for fn in paths.values():   # warm: code objects, MIOpen's algorithm choice
            _phase_times(fn, x, y, 3)
        rounds = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():
                rounds[k].append(_phase_times(fn, x, y, args.iters))
        for k in paths:
            med = {p: statistics.median(r[p] for r in rounds[k]) for p in rounds[k][0]}
            spread = {p: [min(r[p] for r in rounds[k]), max(r[p] for r in rounds[k])] for p in rounds[k][0]}
            print(json.dumps({"size": size, "path": k, "ms": {p: round(v, 4) for p, v in med.items()},
                              "ms_range": {p: [round(a, 4), round(b, 4)] for p, (a, b) in spread.items()}}), flush=True)


if __name__ == "__main__":
    main()
