#!/usr/bin/env python3
"""Forward + backward of the context MLPs: gauspcc_amd.mlp.ContextMLP against the same nn.Sequential in torch, on the same GPU in the same
session, at 50 k and 1 M rows, for the three matrix-pipe classes and TC-GS's 603-100-175 (the plain kernel).

Each figure is the median of three timed repeats (device events around `--iters` steps after a warm-up); the spread is (max - min) of the
three.  The kernel table comes from a run of its own under `rocprofv3 --kernel-trace --stats` with fewer iterations.

    python tools/mlp_train_probe.py [--iters 20] [--rows 50000 1000000] [--out profiles/r07_mlp_train.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gauspcc_amd.mlp import ContextMLP, slab_rows  # noqa: E402

SHAPES = [("HAC mlp_grid", 96, 100, 175, "relu"), ("HAC++ mlp_grid", 48, 100, 225, "relu"), ("HAC++ MLP_d4", 190, 40, 30, "leaky_relu"),
          ("TC-GS mlp_triplane", 603, 100, 175, "relu")]
DEV = "cuda:0"


def step_ms(mod, x, dy, iters):
    for _ in range(3):
        torch.autograd.grad(mod(x), [x] + list(mod.parameters()), dy)
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            torch.autograd.grad(mod(x), [x] + list(mod.parameters()), dy)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / iters)
    return sorted(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, nargs="+", default=[50_000, 1_000_000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mlp_train_probe: needs the GPU (nothing is measured without one)")
    lines = [f"forward + backward (dx and all parameter gradients), ms per step: median of 3 repeats of {a.iters} steps [min .. max]",
             f"{'layer':<20} {'sizes':<12} {'rows':>8} {'slab':>6} | {'ContextMLP':>24} | {'nn.Sequential (torch)':>24} | ratio"]
    for name, din, dh, dout, act in SHAPES:
        for n in a.rows:
            torch.manual_seed(0)
            ours = ContextMLP(din, dh, dout, act).to(DEV)
            theirs = nn.Sequential(nn.Linear(din, dh), nn.ReLU() if act == "relu" else nn.LeakyReLU(0.01), nn.Linear(dh, dout)).to(DEV)
            theirs.load_state_dict(ours.state_dict())
            x = torch.randn(n, din, device=DEV, requires_grad=True)
            dy = torch.randn(n, dout, device=DEV)
            iters = max(2, a.iters // 4) if din > 192 and n > 100_000 else a.iters
            t_ours, t_theirs = step_ms(ours, x, dy, iters), step_ms(theirs, x, dy, iters)
            fmt = lambda t: f"{t[1]:8.3f} [{t[0]:.3f} .. {t[2]:.3f}]"
            lines.append(f"{name:<20} {f'{din}-{dh}-{dout}':<12} {n:>8} {slab_rows(n, din, dh, dout):>6} | {fmt(t_ours):>24} | {fmt(t_theirs):>24} | {t_ours[1] / t_theirs[1]:.2f}")
            print(lines[-1], flush=True)
            if (din, n) == (96, 1_000_000):
                gate = t_ours[1] <= t_theirs[1] + (t_theirs[2] - t_theirs[0])
                lines.append(f"  HAC class at 1 M rows: {'not slower than torch beyond the spread of its repeats' if gate else 'SLOWER than torch beyond the spread of its repeats'}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
