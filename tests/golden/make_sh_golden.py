"""Generate tests/golden/sh.npz by IMPORTING the reference's HAC/utils/sh_utils.py from a checkout of the reference project (it is not part of
this repository):

    python tests/golden/make_sh_golden.py <reference checkout>

Only inputs and the reference's outputs are stored -- no reference source text:

  sh_q        (200, 3, 25) int8: the coefficients are sh_q / 32 (exact in float32), eval_sh's (..., C, M) layout, C = 3
  dirs        (200, 3) float64 unit directions
  weights     (200, 3) float32: the gradients are those of sum(weights * eval_sh(deg, sh, dirs))
  value64_D   (200, 3) float64 eval_sh(D, sh, dirs), D = 0..4
  value32_D   (200, 3) the same call on float32 tensors
  gdirs64_D   (200, 3) float64 autograd gradient for dirs
  gsh64_D     (16, 3, 25) float64 autograd gradient for sh, its first 16 rows (a row's gradient depends on that row alone)
  c0          RGB2SH / SH2RGB's constant as the reference has it: SH2RGB(1) - 0.5
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, M, ROWS = 200, 25, 16


def import_sh_utils(ref):
    path = os.path.join(ref, "src", "gs_compress", "HAC", "utils", "sh_utils.py")
    spec = importlib.util.spec_from_file_location("ref_sh_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    su = import_sh_utils(ref)
    rng = np.random.default_rng(20)
    sh_q = rng.integers(-64, 64, size=(N, 3, M)).astype(np.int8)
    d = rng.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    out = {"sh_q": sh_q, "dirs": d, "weights": w, "c0": np.float64(su.SH2RGB(1.0) - 0.5)}
    for deg in range(5):
        sh = torch.tensor(sh_q, dtype=torch.float64) / 32
        sh.requires_grad_(True)
        dirs = torch.tensor(d, dtype=torch.float64, requires_grad=True)
        val = su.eval_sh(deg, sh, dirs)
        (val * torch.tensor(w, dtype=torch.float64)).sum().backward()
        out[f"value64_{deg}"] = val.detach().numpy()
        out[f"value32_{deg}"] = su.eval_sh(deg, sh.detach().float(), dirs.detach().float()).numpy()
        out[f"gdirs64_{deg}"] = dirs.grad.numpy() if dirs.grad is not None else np.zeros((N, 3))
        out[f"gsh64_{deg}"] = sh.grad.numpy()[:ROWS]
    np.savez_compressed(os.path.join(HERE, "sh.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
