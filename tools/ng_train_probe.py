#!/usr/bin/env python3
"""Developer probe: the neural-Gaussian training path on the 1 M-anchor synthetic frame (SyntheticGaussianModel(1_000_000), F = 50, K = 10;
the frame of tools/raster_train_probe.py) -- the training forward (gsnn_forward_train), the backward (gsnn_backward) and the float32 torch
restatement's forward and backward (tests/ng_train_ref.py, what HAC runs) timed with events on the stream, median of `reps` after warm-up.
Run it under `rocprofv3 --kernel-trace --stats` for the kernel table.
    python tools/ng_train_probe.py [anchors] [reps]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gauspcc_amd.neural_gaussians import mlp_tensors, neural_gaussians_train  # noqa: E402
from gauspcc_amd.synth import SyntheticGaussianModel  # noqa: E402
from tests.ng_train_ref import ng_train_ref  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = torch.device("cuda", 0)
pc = SyntheticGaussianModel(n, seed=0, device="cuda:0")
with torch.no_grad():
    ins = [pc.get_anchor.clone(), pc._anchor_feat.clone(), pc._offset.clone(), pc.get_scaling.clone(), pc.get_mask.clone()]
ctr = ins[0].mean(dim=0)
ext = float((ins[0].max(dim=0).values - ins[0].min(dim=0).values).max())
cam = ctr + torch.tensor([0.0, 0.0, -1.4 * ext], device=dev)
params = mlp_tensors(pc)
for t in ins:
    t.requires_grad_(True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def measure(forward):
    fwd, bwd = [], []
    R = None
    for it in range(reps + 3):
        for t in ins + [p for p in params if p is not None]:
            t.grad = None
        tf, out = timed(forward)
        if R is None:
            g = torch.Generator(device=dev).manual_seed(0)
            R = [torch.randn(o.shape, device=dev, generator=g) for o in out[:6]]
        loss = sum((o * r).sum() for o, r in zip(out[:6], R))
        torch.cuda.synchronize()
        tb, _ = timed(loss.backward)
        if it >= 3:
            fwd.append(tf); bwd.append(tb)
    return statistics.median(fwd), statistics.median(bwd), int(out[0].shape[0])


lib_f, lib_b, m = measure(lambda: neural_gaussians_train(*ins, cam, pc))
ref_f, ref_b, m_ref = measure(lambda: ng_train_ref(*ins, cam, params, False))
print(f"anchors {n}  F {pc.feat_dim}  K {pc.n_offsets}  kept {m} (torch {m_ref})  reps {reps}")
print(f"library  forward {lib_f:.3f} ms  backward {lib_b:.3f} ms   (the backward figure includes the loss's own autograd nodes)")
print(f"torch    forward {ref_f:.3f} ms  backward {ref_b:.3f} ms")
