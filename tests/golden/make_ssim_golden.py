"""Generate tests/golden/ssim.npz by IMPORTING the reference's utils/loss_utils.py from a checkout of the reference project (it is not
part of this repository):

    python tests/golden/make_ssim_golden.py <reference checkout>

Only inputs and the reference's outputs are stored -- no reference source text.  Each case: float32 CPU `ssim(img1, img2, window_size,
size_average)` and the autograd gradients of <weights, ssim(...)> for img1 and img2 (weights = 1 for the mean, a fixed vector per item
otherwise).  Inputs are multiples of 1/255 stored as uint8.

  case a  (3, 24, 32)                       window 11, mean
  case b  (2, 3, 40, 56)                    window 11, size_average=False (img1's gradient only, to keep the file small)
  case c  (3, 5, 7): smaller than the window  window 11, mean
  case d  (3, 24, 32), case a's images      window 7, mean
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {"a": ((3, 24, 32), 11, True), "b": ((2, 3, 40, 56), 11, False), "c": ((3, 5, 7), 11, True), "d": ((3, 24, 32), 7, True)}


def import_loss_utils(ref):
    path = os.path.join(ref, "src", "gs_compress", "HAC", "utils", "loss_utils.py")
    spec = importlib.util.spec_from_file_location("ref_loss_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def images(shape, seed):
    rng = np.random.default_rng(seed)
    *lead, H, W = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = 0.5 + 0.35 * np.sin(7 * xx + 3 * yy)
    base = np.broadcast_to(base, shape).copy()
    base[..., : H // 3, : W // 4] = 0.9
    a = np.clip(base + 0.06 * rng.standard_normal(shape), 0, 1)
    b = np.clip(base + 0.1 * rng.standard_normal(shape), 0, 1)
    return np.rint(a * 255).astype(np.uint8), np.rint(b * 255).astype(np.uint8)


def main(ref):
    lu = import_loss_utils(ref)
    out = {}
    for key, (shape, ws, sa) in CASES.items():
        u1, u2 = images(shape, seed=ord(key) if key != "d" else ord("a"))
        x = torch.tensor(u1, dtype=torch.float32) / 255
        y = torch.tensor(u2, dtype=torch.float32) / 255
        x.requires_grad_(True)
        y.requires_grad_(True)
        s = lu.ssim(x, y, window_size=ws, size_average=sa)
        wts = torch.ones(()) if sa else torch.tensor([0.75, -1.25])
        (s * wts).sum().backward()
        if key != "d":
            out[f"{key}_img1"], out[f"{key}_img2"] = u1, u2
        out[f"{key}_ssim"] = s.detach().numpy().astype(np.float32)
        out[f"{key}_weights"] = wts.numpy().astype(np.float32)
        out[f"{key}_grad1"] = x.grad.numpy()
        if key != "b":
            out[f"{key}_grad2"] = y.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "ssim.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
