"""HAC++'s training branch on the device: gauspcc_amd.hac_plus_renderer.generate_neural_gaussians(is_training=True, step=12000) against the
float32 torch restatement tests/hacpp_branch_ref.py on the same GPU, alternating in one process, on SyntheticGaussianModelPlus with 80 %
of the anchors visible; then the two new kernels alone at the 1 M-anchor shape.

    python tools/hacpp_train_probe.py [anchors ...]          (default: 100000 1000000)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/hacpp_train_probe.py --steps 100000     (a run of its own: drop-in steps only)

Times are device events after warm-up: median [min, max] of three rounds.  The loss is sum(xyz) + sum(color) + sum(opacity) + sum(scaling)
+ sum(rot) + bit_per_param; `step` is forward + backward.  The byte bounds printed beside the kernels are computed from the shapes at the
6.3 TB/s the project uses for HBM; everything else is measured.  profiles/r07_hacpp_train.txt holds a run.
"""
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)
HBM = 6.3e12


def model(n):
    from gauspcc_amd import entropy_models
    from gauspcc_amd.synth import SyntheticGaussianModelPlus

    pc = SyntheticGaussianModelPlus(n, seed=3, device="cuda:0")
    for m in pc.encoding_xyz.modules():
        if hasattr(m, "differentiable"):
            m.differentiable = True
    pc.EG_mix_prob_2, pc.entropy_gaussian = entropy_models.Entropy_gaussian_mix_prob_2(Q=1), entropy_models.Entropy_gaussian(Q=1)
    pc.update_anchor_bound = lambda: None
    for t in (pc._anchor_feat, pc._offset, pc._scaling, pc._mask):
        t.requires_grad_(True)
    cam = types.SimpleNamespace(camera_center=pc.get_anchor.mean(dim=0).detach() + torch.tensor([0.0, 0.0, -2.0], device=DEV))
    vis = torch.rand(pc.get_anchor.shape[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) < 0.8
    return pc, cam, vis


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def one_step(run, seed):
    torch.manual_seed(seed)
    out, fwd = timed(run)
    loss = sum(o.sum() for o in out[:5]) + out[7]
    _, bwd = timed(loss.backward)
    return fwd, bwd


def fmt(v):
    return f"{statistics.median(v):8.2f} [{min(v):.2f}, {max(v):.2f}]"


def compare(n, rounds=3, warm=2):
    from gauspcc_amd.hac_plus_renderer import generate_neural_gaussians
    from tests.hacpp_branch_ref import ShadowModel, hacpp_branch_ref

    pc, cam, vis = model(n)
    shadow = ShadowModel(pc, torch.float32)
    progs = {"drop-in": lambda: generate_neural_gaussians(cam, pc, vis, is_training=True, step=12000),
             "restatement": lambda: hacpp_branch_ref(cam, shadow, vis, 12000)}
    res = {k: ([], []) for k in progs}
    for r in range(warm + rounds):
        for name, run in progs.items():
            torch.cuda.reset_peak_memory_stats()
            fwd, bwd = one_step(run, r)
            if r >= warm:
                res[name][0].append(fwd); res[name][1].append(bwd)
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
            res[name] = (*res[name][:2], peak)
    print(f"\n{pc.get_anchor.shape[0]} anchors, {int(vis.sum())} visible, step 12000 (measured, ms: median [min, max] of {rounds})")
    for name, (fwd, bwd, peak) in res.items():
        print(f"  {name:<12} forward {fmt(fwd)}   backward {fmt(bwd)}   step {fmt([a + b for a, b in zip(fwd, bwd)])}   peak {peak:.2f} GiB")
    d, t = [a + b for a, b in zip(*res["drop-in"][:2])], [a + b for a, b in zip(*res["restatement"][:2])]
    print(f"  step ratio restatement / drop-in: {statistics.median(t) / statistics.median(d):.2f} (spread: drop-in {min(d):.2f}..{max(d):.2f}, restatement {min(t):.2f}..{max(t):.2f})")


def kernels(n=1_000_000, F=50, K=10, reps=20):
    from gauspcc_amd.densify import select_rows
    from gauspcc_amd.neural_gaussians import quant_noise

    widths = (F, 6, 3 * K)
    xs = [torch.randn(n, w, device=DEV) for w in widths]
    us = [torch.rand(n, w, device=DEV) - 0.5 for w in widths]
    grid = torch.randn(n, 3 * F + 12 + 6 * K + 3, device=DEV)
    adj = grid[:, -3:].requires_grad_(True)          # a strided leaf: the backward below is the kernel and nothing else
    gs = [torch.randn(n, w, device=DEV) for w in widths] + [torch.randn(n, 3, device=DEV)]
    fwd, bwd = [], []
    for _ in range(reps):
        out, t = timed(lambda: quant_noise(xs, us, (1, 0.001, 0.2), adj))
        fwd.append(t)
        _, t = timed(lambda: torch.autograd.grad(out, [adj], gs))
        bwd.append(t)
    cols = sum(widths)
    b_f, b_b = 3 * cols * 4 * n, 2 * cols * 4 * n
    print(f"\nthe kernels alone at n = {n}, widths {widths}, adj a view of a {grid.shape[1]}-column matrix (measured, ms: median [min, max] of {reps})")
    print(f"  gsnn_noise_forward   {fmt(fwd)}   bound {b_f / HBM * 1e3:.2f} ms (computed: x, u, y = {b_f / 1e9:.2f} GB at 6.3 TB/s)")
    print(f"  gsnn_noise_backward  {fmt(bwd)}   bound {b_b / HBM * 1e3:.2f} ms (computed: g, u = {b_b / 1e9:.2f} GB at 6.3 TB/s)")
    mask = torch.rand(n, device=DEV) < 0.8
    ts = [torch.randn(n, w, device=DEV).requires_grad_(True) for w in (3, F, 3 * K, 6, K)]
    cf, ef = [], []
    for _ in range(reps):
        out, t = timed(lambda: select_rows(mask, *ts))
        cf.append(t)
        ups = [torch.ones_like(o) for o in out]
        _, t = timed(lambda: torch.autograd.grad(out, ts, ups))
        ef.append(t)
    m = int(mask.sum())
    byt = sum((n + m) * w * 4 for w in (3, F, 3 * K, 6, K))
    print(f"  the five visible gathers, {m} of {n} rows: gpcc_compact_rows {fmt(cf)} (one wait), gpcc_expand_rows {fmt(ef)}   bound {byt / HBM * 1e3:.2f} ms each "
          f"(computed: {byt / 1e9:.2f} GB)")


def steps_only(n, steps=5):
    from gauspcc_amd.hac_plus_renderer import generate_neural_gaussians

    pc, cam, vis = model(n)
    for r in range(steps):
        one_step(lambda: generate_neural_gaussians(cam, pc, vis, is_training=True, step=12000), r)
    torch.cuda.synchronize()
    print(f"{steps} drop-in steps at {n} anchors")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--steps":
        steps_only(int(args[1]) if len(args) > 1 else 100000)
    else:
        for n in [int(a) for a in args] or [100000, 1000000]:
            compare(n)
        kernels()
