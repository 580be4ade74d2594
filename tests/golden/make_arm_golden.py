"""Generate tests/golden/arm_rate.npz by IMPORTING CAT-3DGS's scene/arm.py from a checkout of the reference project (it is not part of
this repository; it needs einops):

    python tests/golden/make_arm_golden.py <reference checkout>

Only inputs, parameter values, state-dict key names and the reference's float32 CPU outputs are stored -- no reference source text.
scene/arm.py imports `scene.linear_layers` and `scene.synthesis`; a stub `scene` package whose __path__ is the checkout's scene/ lets
those load without the rest of the framework (scene/__init__.py pulls in the whole training stack).  The module is scripted, as
scene/triplane.py scripts it, and runs on the CPU.  Each case stores its levels y<i> ([1, C, H, W]), the parameters p<j> in state-dict
order and their key names, the hidden widths, the upstream weights w, the reference's rate, mu and scale (flat, in (level, c, h, w)
order) and the autograd gradients of sum(w * rate) for every level and every parameter:

  round   integer latents; levels [1,3,5,7], [1,3,10,14], [1,2,1,2], [1,1,6,1]; generator seed 7; parameters randn * 0.06, last bias
          (0.3, -2.0); latents round(randn * 1.5), every 11th flat element + 40: those alone sit on the 2^-16 floor
  noise   the same parameters and latents + U(-0.5, 0.5) (the training-time quantiser)
  kinks   round's parameters with the output layer's log_scale row * 40 and its bias -11: by the reference's own output 123 latents
          have log_scale below -10, 69 above 13.8155, and 234 lie inside the clamp and off the floor
  wide    hidden widths [24, 24, 8]: a residual block at a width other than 16, and plain layers
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 3, 5, 7), (1, 3, 10, 14), (1, 2, 1, 2), (1, 1, 6, 1)]


def import_arm(ref):
    scene = types.ModuleType("scene")
    scene.__path__ = [os.path.join(ref, "src", "gs_compress", "CAT-3DGS", "scene")]
    sys.modules["scene"] = scene
    return importlib.import_module("scene.arm")


def latents(g):
    out = []
    for s in SHAPES:
        y = torch.round(torch.randn(s, generator=g) * 1.5)
        y.view(-1)[::11] += 40.0
        out.append(y)
    return out


def build(mod, layers, g, gain, last_bias, ls_gain):
    arm = torch.jit.script(mod.ArmMLP(12, layers))
    sd = arm.state_dict()
    keys = list(sd.keys())
    with torch.no_grad():
        for k in keys:
            sd[k].copy_(torch.randn(sd[k].shape, generator=g) * gain)
        sd[keys[-1]].copy_(torch.tensor(last_bias))
        sd[keys[-2]][1].mul_(ls_gain)
    arm.load_state_dict(sd)
    return arm, keys


def run(mod, arm, levels, w):
    levels = [y.clone().requires_grad_(True) for y in levels]
    idx = torch.arange(0, 12)
    flat, ctx = mod.get_flat_latent_and_context(levels, 5, idx)
    rate, mu, scale = mod.compute_rate(flat, arm(ctx))
    params = [p for _, p in arm.named_parameters()]
    for p in params:
        p.grad = None
    (rate * w).sum().backward()
    return rate.detach(), mu.detach(), scale.detach(), [y.grad for y in levels], [p.grad for p in params]


def main(ref):
    mod = import_arm(ref)
    out = {}
    cases = {"round": ([16, 16, 16, 16], 0.0, (0.3, -2.0), 1.0), "noise": ([16, 16, 16, 16], 0.5, (0.3, -2.0), 1.0),
             "kinks": ([16, 16, 16, 16], 0.0, (0.3, -11.0), 40.0), "wide": ([24, 24, 8], 0.0, (0.3, -2.0), 1.0)}
    for key, (layers, noise, last_bias, ls_gain) in cases.items():
        g = torch.Generator().manual_seed(7)
        arm, keys = build(mod, layers, g, 0.06, last_bias, ls_gain)
        assert keys == [k for k, _ in arm.named_parameters()]
        levels = latents(g)
        if noise:
            levels = [y + (torch.rand(y.shape, generator=g) - 0.5) * 2 * noise for y in levels]
        w = torch.randn(sum(y.numel() for y in levels), generator=g)
        rate, mu, scale, gy, gp = run(mod, arm, levels, w)
        floor = float((rate >= 16.0).float().mean())
        ends = (int((scale == scale.max()).sum()), int((scale == scale.min()).sum()))
        print(f"{key}: {rate.numel()} latents, {100 * floor:.1f} % on the floor, scale in [{float(scale.min()):.4g}, {float(scale.max()):.4g}] {ends}")
        out[f"{key}_nlevels"] = np.int64(len(levels))
        out[f"{key}_layers"] = np.asarray(layers, dtype=np.int64)
        out[f"{key}_keys"] = np.asarray(keys)
        for i, y in enumerate(levels):
            out[f"{key}_y{i}"] = y.numpy()
            out[f"{key}_gy{i}"] = gy[i].numpy()
        for j, (p, gr) in enumerate(zip(arm.parameters(), gp)):
            out[f"{key}_p{j}"] = p.detach().numpy()
            out[f"{key}_gp{j}"] = gr.numpy()
        out[f"{key}_w"] = w.numpy()
        out[f"{key}_rate"], out[f"{key}_mu"], out[f"{key}_scale"] = rate.numpy(), mu.numpy(), scale.numpy()
    np.savez_compressed(os.path.join(HERE, "arm_rate.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
