"""Generate tests/golden/rate.npz by IMPORTING the reference's utils/entropy_models.py (HAC-plus, and CAT-3DGS for the Q floor) from a
checkout of the reference project (it is not part of this repository):

    python tests/golden/make_rate_golden.py <reference checkout>

Only inputs and the reference's float32 CPU outputs are stored -- no reference source text.  The reference modules import
`utils.encodings.use_clamp`; a stub module with use_clamp = True stands in for it.  Their Low_bound backward ends in `.cuda()`, so
torch.Tensor.cuda is patched to the identity while this script runs (here only).  Each case stores its inputs, the output, the upstream
weights w and the autograd gradients of sum(w * out) for every input that takes one:

  k1_row      Entropy_gaussian, Q per row (n, 1) requiring grad, x_mean given
  k1_full     Entropy_gaussian, Q full (n, c) requiring grad, x_mean = None
  k1_num      Entropy_gaussian, Q = 1.3e-3 (a Python number)
  k1_zero_d   Entropy_gaussian, Q a 0-d tensor requiring grad
  k1_clamp    Entropy_gaussian_clamp, Q per row
  k2          Entropy_gaussian_mix_prob_2, Q per row
  k3          Entropy_gaussian_mix_prob_3, Q per row
  k2_lkl      Entropy_gaussian_mix_prob_2, return_lkl=True
  cat_floor   CAT-3DGS's Entropy_gaussian: Q per row with some rows below 1e-9
Every case has elements outside the +-15000 Q window (x_mean is set so that the window cuts into the data), scales below 1e-9, and
elements far in the tails whose likelihood sits on the 1e-6 floor.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, C = 24, 6


def import_entropy(ref, framework):
    enc = types.ModuleType("utils.encodings")
    enc.use_clamp = True
    utils = types.ModuleType("utils")
    utils.encodings = enc
    sys.modules["utils"], sys.modules["utils.encodings"] = utils, enc
    path = os.path.join(ref, "src", "gs_compress", framework, "utils", "entropy_models.py")
    spec = importlib.util.spec_from_file_location(f"ref_entropy_{framework.replace('-', '_')}", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs(seed, k, q_kind):
    g = torch.Generator().manual_seed(seed)
    mean = [torch.randn(N, C, generator=g) * 2 for _ in range(k)]
    scale = [torch.exp(torch.randn(N, C, generator=g) * 0.7 - 0.7) for _ in range(k)]
    for s in scale:
        s.view(-1)[5::17] = 1e-12                        # below the 1e-9 scale floor
    x = torch.round(mean[0] + torch.randn(N, C, generator=g) * 1.5)
    x.view(-1)[3::11] += 40.0                            # far tails: likelihood on the 1e-6 floor
    probs = list(torch.softmax(torch.randn(k, N, C, generator=g), dim=0)) if k > 1 else []
    # odd rows: Q ~ 1e-3 (HAC's scaling bins), window +-15000 Q = +-7.5..22.5 around x_mean: the tails fall outside; even rows: Q ~ 1
    small = torch.where(torch.arange(N) % 2 == 1, 1e-3, 1.0).view(N, 1)
    if q_kind == "row":
        Q = (0.5 + torch.rand(N, 1, generator=g)) * small
    elif q_kind == "full":
        Q = (0.5 + torch.rand(N, C, generator=g)) * small
    elif q_kind == "zero_d":
        Q = torch.tensor(1.1e-3)
    elif q_kind == "floor":
        Q = (0.5 + torch.rand(N, 1, generator=g)) * small
        Q[::5] = 1e-12                                   # below CAT-3DGS's 1e-9 floor
    else:
        Q = 1.3e-3
    w = torch.randn(N, C, generator=g)
    return x, mean, scale, probs, Q, w


CASES = {
    "k1_row": ("HAC-plus", "Entropy_gaussian", 1, "row", True, False),
    "k1_full": ("HAC-plus", "Entropy_gaussian", 1, "full", False, False),
    "k1_num": ("HAC-plus", "Entropy_gaussian", 1, "num", True, False),
    "k1_zero_d": ("HAC-plus", "Entropy_gaussian", 1, "zero_d", True, False),
    "k1_clamp": ("HAC-plus", "Entropy_gaussian_clamp", 1, "row", False, False),
    "k2": ("HAC-plus", "Entropy_gaussian_mix_prob_2", 2, "row", True, False),
    "k3": ("HAC-plus", "Entropy_gaussian_mix_prob_3", 3, "row", False, False),
    "k2_lkl": ("HAC-plus", "Entropy_gaussian_mix_prob_2", 2, "row", True, True),
    "cat_floor": ("CAT-3DGS", "Entropy_gaussian", 1, "floor", True, False),
}


def main(ref):
    torch.Tensor.cuda = lambda self, *a, **kw: self   # Low_bound.backward's .cuda(); this script only
    out = {}
    for i, (key, (fw, cls, k, q_kind, give_mean, lkl)) in enumerate(CASES.items()):
        mod = import_entropy(ref, fw)
        x, mean, scale, probs, Q, w = inputs(100 + i, k, q_kind)
        x_mean = x.mean() + 10.0 if give_mean else None   # off-centre: the window cuts into the data on one side
        leaves = [x] + mean + scale + probs + ([Q] if isinstance(Q, torch.Tensor) else [])
        for t in leaves:
            t.requires_grad_(True)
        m = getattr(mod, cls)()
        if cls == "Entropy_gaussian_clamp":
            res = m(x, mean[0], scale[0], Q)
        elif k == 1:
            res = m(x, mean[0], scale[0], Q, x_mean)
        else:
            res = m(x, *mean, *scale, *probs, Q=Q, x_mean=x_mean, return_lkl=lkl)
        (res * w).sum().backward()
        out[f"{key}_x"] = x.detach().numpy()
        for j in range(k):
            out[f"{key}_mean{j}"] = mean[j].detach().numpy()
            out[f"{key}_scale{j}"] = scale[j].detach().numpy()
            out[f"{key}_gmean{j}"] = mean[j].grad.numpy()
            out[f"{key}_gscale{j}"] = scale[j].grad.numpy()
            if k > 1:
                out[f"{key}_prob{j}"] = probs[j].detach().numpy()
                out[f"{key}_gprob{j}"] = probs[j].grad.numpy()
        if isinstance(Q, torch.Tensor):
            out[f"{key}_Q"] = Q.detach().numpy()
            out[f"{key}_gQ"] = Q.grad.numpy()
        else:
            out[f"{key}_Qnum"] = np.float64(Q)
        if give_mean:
            out[f"{key}_xmean"] = x_mean.detach().numpy()
        out[f"{key}_w"] = w.numpy()
        out[f"{key}_out"] = res.detach().numpy()
        out[f"{key}_gx"] = x.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "rate.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
