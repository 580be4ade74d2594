"""Times gauspcc_amd.arm.arm_rate (gsarm_rate_forward / gsarm_rate_backward) against the float32 torch sequence a framework would run
(tests/arm_ref.py: rate_torch -- pad, unfold twice, the materialised [n, 25] matrix, index_select, linear layers, autograd) at CAT-3DGS's
shape for --anchors anchors: three planes, each with its own ARM and two levels of 72 channels, round(sqrt(anchors / 36)) and twice that
many texels per side (1 M anchors: 167^2 and 334^2, about 10 M latents per plane).  Same process, alternating, device events, warm.

    python tools/arm_probe.py [--anchors 1000000] [--iters 5] [--rounds 5] [--out profiles/r07_arm_rate.txt]

fwd = the three planes' total bits under torch.no_grad() (what an evaluation pass runs); step = forward + backward to every latent and every
ARM parameter (what a training iteration runs).  Times are medians over the rounds of the mean of --iters calls (ms per call), with the
range over the rounds.  Peak memory is torch.cuda.max_memory_allocated() over one step minus what was allocated before it; the library's
workspace comes from torch's allocator, so it is counted.  The report also carries the accuracy ratios of tests/test_gpu_arm_rate.py's
criterion on the golden cases: e_dev / e_t32 against the float64 restatement, the largest per kind of quantity."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gauspcc_amd import arm as A  # noqa: E402
from tests import arm_ref  # noqa: E402

DEV = "cuda"
CHANNELS = 72
MADDS_FWD = 12 * 16 + 3 * 16 * 16 + 16 * 2          # per latent, the reference's ARM: 992 multiply-adds (1 058 with biases and residuals)


def _planes(anchors, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    side = round((anchors / 36) ** 0.5)
    planes, arms = [], []
    for _ in range(3):
        planes.append([(torch.round(torch.randn(1, CHANNELS, s, s, device=DEV, generator=g) * 1.5)
                        + torch.rand(1, CHANNELS, s, s, device=DEV, generator=g) - 0.5).requires_grad_(True) for s in (side, 2 * side)])
        arm = A.ArmMLP(12, [16, 16, 16, 16]).to(DEV)
        with torch.no_grad():
            for p in arm.parameters():
                p.copy_(torch.randn(p.shape, device=DEV, generator=g) * 0.06)
        arms.append(arm)
    return side, planes, arms


def _fused(planes, arms):
    return sum(A.arm_rate(lv, arm) for lv, arm in zip(planes, arms))


def _torch(planes, arms):
    return sum(arm_ref.rate_torch(lv, list(arm.parameters()))[0].sum() for lv, arm in zip(planes, arms))


def _clear(planes, arms):
    for lv in planes:
        for y in lv:
            y.grad = None
    for arm in arms:
        for p in arm.parameters():
            p.grad = None


def _time(fn, planes, arms, iters, backward):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(iters):
        if backward:
            fn(planes, arms).backward()
            _clear(planes, arms)
        else:
            with torch.no_grad():
                fn(planes, arms)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def _peak(fn, planes, arms):
    _clear(planes, arms)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(planes, arms).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    _clear(planes, arms)
    return peak


def _accuracy(lines):
    z = np.load(os.path.join(ROOT, "tests", "golden", "arm_rate.npz"))
    lines.append("accuracy on the golden cases: max |x - float64| of the device (e_dev) over that of the reference's recorded float32 values (e_t32),")
    lines.append("the largest ratio per kind of quantity (tests/test_gpu_arm_rate.py allows 4, plus its floor where e_t32 is about 0)")
    for key in arm_ref.CASES:
        c = arm_ref.golden_case(z, key)
        f64 = arm_ref.forward64(c["levels"], c["params"])
        gl, gp, _ = arm_ref.grads64(c["levels"], c["params"], c["w"], f64)
        arm = A.ArmMLP(12, c["layers"])
        arm.load_state_dict({k: torch.as_tensor(p) for k, p in zip(c["keys"], c["params"])})
        arm = arm.to(DEV)
        leaves = [torch.as_tensor(y).to(DEV).requires_grad_(True) for y in c["levels"]]
        rate, mu, scale = A.arm_rate(leaves, arm, reduce="none", return_params=True)
        (rate * torch.as_tensor(c["w"]).to(DEV)).sum().backward()
        flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).double().cpu().numpy()   # noqa: E731

        def ratio(dev, gold, want):
            want = np.asarray(want).reshape(-1)
            e_dev, e_t32 = np.abs(dev.reshape(-1) - want).max(), np.abs(np.asarray(gold, dtype=np.float64).reshape(-1) - want).max()
            return e_dev / e_t32 if e_t32 else float("inf") if e_dev else 0.0

        kinds = {"rate": ratio(rate.detach().double().cpu().numpy(), c["rate"], f64["rate"]), "mu": ratio(flat(mu), c["mu"], f64["mu"]),
                 "scale": ratio(flat(scale), c["scale"], f64["scale"]),
                 "d latent": max(ratio(y.grad.double().cpu().numpy(), g, w) for y, g, w in zip(leaves, c["g_levels"], gl)),
                 "d parameter": max(ratio(p.grad.double().cpu().numpy(), g, w) for p, g, w in zip(arm.parameters(), c["g_params"], gp))}
        lines.append(f"  {key:6s} " + "  ".join(f"{k} {v:.2f}" for k, v in kinds.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=1000000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_arm_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/arm_probe.py measures on the GPU; none is visible")
    side, planes, arms = _planes(args.anchors)
    n = 3 * CHANNELS * (side * side + 4 * side * side)
    paths = {"fused": _fused, "torch": _torch}
    for fn in paths.values():                                 # warm every shape and both directions
        _time(fn, planes, arms, 1, False)
        _time(fn, planes, arms, 1, True)
    res = {(k, b): [] for k in paths for b in (False, True)}
    for _ in range(args.rounds):
        for k, fn in paths.items():
            for b in (False, True):
                res[(k, b)].append(_time(fn, planes, arms, args.iters, b))
    peaks = {k: _peak(fn, planes, arms) for k, fn in paths.items()}
    lines = [f"tools/arm_probe.py --anchors {args.anchors} --iters {args.iters} --rounds {args.rounds}  ({torch.cuda.get_device_name(0)})",
             f"3 planes x [{CHANNELS}, {side}, {side}] + [{CHANNELS}, {2 * side}, {2 * side}], ARM 12-16-16-16-16-2 per plane: {n} latents per call",
             "ms per call, median over the rounds [min, max]; fwd under no_grad, step = forward + backward"]
    med = {}
    for (k, b), v in res.items():
        med[(k, b)] = statistics.median(v)
        lines.append(f"  {k:5s} {'step' if b else 'fwd ':4s} {med[(k, b)]:9.3f}  [{min(v):.3f}, {max(v):.3f}]")
    lines.append(f"  torch / fused: fwd {med[('torch', False)] / med[('fused', False)]:.1f} x, step {med[('torch', True)] / med[('fused', True)]:.1f} x")
    gf = 2.0 * MADDS_FWD * n / (med[("fused", False)] * 1e-3) / 1e12
    lines.append(f"  fused fwd: {gf:.1f} TFLOP/s of the ARM's {MADDS_FWD} multiply-adds per latent (FP32 vector peak 157.3), "
                 f"{4.0 * n / (med[('fused', False)] * 1e-3) / 1e9:.0f} GB/s of latents read once")
    lines.append("peak device memory of one step beyond the latents and the parameters (bytes, and per latent of the call)")
    for k, v in peaks.items():
        lines.append(f"  {k:5s} {v:14d}  {v / n:8.1f} B / latent")
    big = CHANNELS * 4 * side * side
    lines.append(f"  fused, expected: gradients 4 B / latent of the call + scratch 48 B / latent of the largest level ({48 * big} bytes)")
    _accuracy(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
