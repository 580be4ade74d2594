"""Times gauspcc_amd.entropy_models (gsac_rate_forward / gsac_rate_backward) against a torch restatement of the reference's modules that
keeps torch.distributions.Normal's argument validation and Low_bound's host round trip (tests/rate_ref.py: RefEntropy_*), in the same
process, alternating, with device events, warm; one JSON line per (shape, path).

    python tools/rate_probe.py [--iters 30] [--rounds 5] [--anchors 1000000] [--skip-ng]

Shapes: HAC's three rate terms on 50 k chosen anchors (feat 50, scaling 6, offsets 30, Q per row (n, 1)) as one step, and HAC++'s
mixture term (Entropy_gaussian_mix_prob_2 on feat 50, Q full).  fwd = the three (or one) forward calls, bwd = the backward of the sum of
their means, step = both.  Then one whole generate_neural_gaussians(is_training=True, step=12000) + backward of bit_per_param on
SyntheticGaussianModel (--anchors) with each module.  Times are medians over rounds of --iters calls each (ms per call)."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gauspcc_amd import entropy_models as em  # noqa: E402
from tests import rate_ref  # noqa: E402

DEV = "cuda"


def _hac_inputs(n, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    terms = []
    for c, q0 in ((50, 1.0), (6, 0.001), (30, 0.2)):
        mean = torch.randn(n, c, device=DEV, generator=g)
        scale = torch.rand(n, c, device=DEV, generator=g) + 0.05
        q = q0 * (1 + torch.tanh(torch.randn(n, 1, device=DEV, generator=g)))
        x = mean + torch.randn(n, c, device=DEV, generator=g) * 2 * q
        terms.append((x, mean, scale, q, x.mean()))
    return terms


def _mix_inputs(n, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    m1, m2 = (torch.randn(n, 50, device=DEV, generator=g) for _ in range(2))
    s1, s2 = (torch.rand(n, 50, device=DEV, generator=g) + 0.05 for _ in range(2))
    probs = torch.softmax(torch.randn(n, 50, 2, device=DEV, generator=g), dim=-1)
    q = 1 + torch.tanh(torch.randn(n, 50, device=DEV, generator=g))
    x = m1 + torch.randn(n, 50, device=DEV, generator=g)
    return (x, m1, m2, s1, s2, probs[..., 0], probs[..., 1], q, x.mean())


def _hac_step(mod, terms):
    tot = 0
    for x, m, s, q, xm in terms:
        tot = tot + mod(x, m.requires_grad_(True), s, q.requires_grad_(True), xm).mean()
    return tot


def _mix_step(mod, a):
    x, m1, m2, s1, s2, p1, p2, q, xm = a
    return mod(x, m1.requires_grad_(True), m2, s1, s2, p1, p2, Q=q, x_mean=xm).mean()


def _times(fn, iters):
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for e in ev:
        e[0].record()
        loss = fn()
        e[1].record()
        loss.backward()
        e[2].record()
    torch.cuda.synchronize()
    fwd = sum(e[0].elapsed_time(e[1]) for e in ev) / iters
    bwd = sum(e[1].elapsed_time(e[2]) for e in ev) / iters
    return {"fwd": fwd, "bwd": bwd, "step": fwd + bwd}


def _report(label, paths, iters, rounds):
    for fn in paths.values():
        _times(fn, 2)
    res = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            res[k].append(_times(fn, iters))
    for k in paths:
        med = {p: statistics.median(r[p] for r in res[k]) for p in res[k][0]}
        rng = {p: [round(min(r[p] for r in res[k]), 4), round(max(r[p] for r in res[k]), 4)] for p in res[k][0]}
        print(json.dumps({"shape": label, "path": k, "ms": {p: round(v, 4) for p, v in med.items()}, "ms_range": rng}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--anchors", type=int, default=1000000)
    ap.add_argument("--skip-ng", action="store_true")
    args = ap.parse_args()
    terms = _hac_inputs(args.rows)
    _report(f"HAC 3 terms x {args.rows} rows (50 + 6 + 30 cols, Q per row)",
            {"hip": lambda: _hac_step(em.Entropy_gaussian(), terms), "torch": lambda: _hac_step(rate_ref.RefEntropy_gaussian(), terms)},
            args.iters, args.rounds)
    mix = _mix_inputs(args.rows)
    _report(f"HAC++ mix_prob_2 {args.rows} x 50 (Q full)",
            {"hip": lambda: _mix_step(em.Entropy_gaussian_mix_prob_2(), mix),
             "torch": lambda: _mix_step(rate_ref.RefEntropy_gaussian_mix_prob_2(), mix)}, args.iters, args.rounds)
    if args.skip_ng:
        return
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians
    from gauspcc_amd.synth import SyntheticGaussianModel

    pc = SyntheticGaussianModel(args.anchors, seed=3, device="cuda:0")
    pc.update_anchor_bound = lambda: None
    cam = types.SimpleNamespace(camera_center=pc.get_anchor.mean(dim=0) + torch.tensor([0.0, 0.0, -2.0], device=DEV))
    mods = {"hip": em.Entropy_gaussian(), "torch": rate_ref.RefEntropy_gaussian()}

    def ng(mod):
        def run():
            pc.entropy_gaussian = mod
            out = generate_neural_gaussians(cam, pc, None, is_training=True, step=12000)
            return out[7] + out[0].sum() * 0 + out[5].sum() * 0
        return run
    _report(f"generate_neural_gaussians(is_training=True, step=12000) + backward, {args.anchors} anchors",
            {k: ng(m) for k, m in mods.items()}, max(3, args.iters // 6), args.rounds)


if __name__ == "__main__":
    main()
