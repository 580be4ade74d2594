"""TC-GS's training branch on the device: gauspcc_amd.tcgs_renderer.generate_neural_gaussians(is_training=True) at steps 12000 (the repeat
form) and 20000 (pc.knnanchor, the autoencoder loss) against the float32 torch restatement tests/tcgs_branch_ref.py on the same GPU,
alternating in one process, on SyntheticGaussianModelTC (feat_dim 50, 10 offsets, C = 50, 256 x 256 planes, K = 4, every anchor visible as
train.py calls it, the anchors trainable).  The restatement calls the library's Triplane as the reference calls its own and concatenates:
the parent's sampler + torch.cat.  Then, alone:

  context_rows forward + backward against triplane_sample + torch.cat, in both coordinate forms (the upstream gradient a contiguous
      (N, 603) matrix, as the MLP's backward leaves it)
  quantise_steps against the three ste_multistep calls on the attributes of all anchors
  the step at 12000 with mlp_triplane as nn.Sequential and as gauspcc_amd.mlp.ContextMLP (whose backward for 603-100-175 is the plain kernel)

    python tools/tcgs_train_probe.py [--out FILE] [anchors ...]          (default: 100000 1000000, profiles/r07_tcgs_train.txt)

Times are device events after warm-up: median [min, max] of the timed rounds; a ratio is quoted with both spreads.  The loss of a step is
sum(xyz) + sum(color) + sum(opacity) + sum(scaling) + sum(rot) + bit_per_param (+ lae); `step` is forward + backward.
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
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def model(n):
    from gauspcc_amd import entropy_models
    from gauspcc_amd.synth import SyntheticGaussianModelTC

    class Model(SyntheticGaussianModelTC):
        get_anchor = property(lambda self: self._anchor_leaf)

    pc = Model(n, seed=3, device="cuda:0")
    pc._anchor_leaf = (torch.round(pc._anchor / pc.voxel_size) * pc.voxel_size).detach().requires_grad_(True)
    pc.entropy_gaussian = entropy_models.Entropy_gaussian(Q=1)
    for t in (pc._anchor_feat, pc._offset, pc._scaling, pc._mask):
        t.requires_grad_(True)
    cam = types.SimpleNamespace(camera_center=pc.get_anchor.detach().mean(dim=0) + torch.tensor([0.0, 0.0, -2.0], device=DEV))
    return pc, cam


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
    loss = sum(o.sum() for o in out[:5]) + out[7] + (out[11] if out[11] is not None else 0)
    _, bwd = timed(loss.backward)
    return fwd, bwd


def fmt(v):
    return f"{statistics.median(v):8.2f} [{min(v):.2f}, {max(v):.2f}]"


def ratio(name_a, a, name_b, b):
    r = statistics.median(b) / statistics.median(a)
    apart = min(b) > max(a) or min(a) > max(b)
    return (f"{name_b} / {name_a}: {r:.2f} (spread: {name_a} {min(a):.2f}..{max(a):.2f}, {name_b} {min(b):.2f}..{max(b):.2f}; "
            f"{'beyond' if apart else 'WITHIN'} the spread of the repeated runs)")


def alternate(progs, rounds, warm, measure):
    res = {k: [] for k in progs}
    extra = {}
    for r in range(warm + rounds):
        for name, run in progs.items():
            torch.cuda.reset_peak_memory_stats()
            v = measure(run, r)
            extra[name] = torch.cuda.max_memory_allocated() / 2 ** 30
            if r >= warm:
                res[name].append(v)
    return res, extra


def steps(pc, cam, rounds=5, warm=2):
    from gauspcc_amd.tcgs_renderer import generate_neural_gaussians
    from tests.tcgs_branch_ref import ShadowModel, tcgs_branch_ref

    shadow = ShadowModel(pc, torch.float32, triplane=pc.triplane, tri_mlp=pc.mlp_triplane)
    for step in (12000, 20000):
        progs = {"drop-in": lambda: generate_neural_gaussians(cam, pc, None, is_training=True, step=step),
                 "restatement": lambda: tcgs_branch_ref(cam, shadow, None, step)}
        res, peak = alternate(progs, rounds, warm, one_step)
        say(f"\n{pc.get_anchor.shape[0]} anchors, all visible, step {step} (measured, ms: median [min, max] of {rounds})")
        for name, v in res.items():
            fwd, bwd = [a for a, _ in v], [b for _, b in v]
            say(f"  {name:<12} forward {fmt(fwd)}   backward {fmt(bwd)}   step {fmt([a + b for a, b in v])}   peak {peak[name]:.2f} GiB")
        say("  step " + ratio("drop-in", [a + b for a, b in res["drop-in"]], "restatement", [a + b for a, b in res["restatement"]]))


def rows(pc, rounds=7, warm=2):
    from gauspcc_amd.triplane import triplane_rows, triplane_sample

    tri, anchor = pc.triplane, pc.get_anchor.detach()
    N = anchor.shape[0]
    radii = 0.5 * tri.radii
    width = 4 * 3 * tri.planes.shape[1] + 3
    up = torch.randn(N, width, device=DEV)
    for form, co, rep in (("repeat form (N, 3), K = 4", anchor, 4), ("(N, K, 3) form, pc.knnanchor", pc.knnanchor.contiguous(), None)):
        def run(kind):
            c = co.clone().requires_grad_(True)
            t = c if rep else anchor.clone().requires_grad_(True)
            if kind == "rows":
                out = triplane_rows(tri.planes, c, t, pc.x_bound_max, pc.x_bound_min, radii, repeat=rep)
            else:
                out = torch.cat([triplane_sample(tri.planes, c, pc.x_bound_max, pc.x_bound_min, radii, repeat=rep), t], dim=1)
            out.backward(up)
            tri.planes.grad = None
        progs = {"context_rows": lambda: run("rows"), "sample + cat": lambda: run("cat")}
        res, peak = alternate(progs, rounds, warm, lambda fn, r: timed(fn)[1])
        say(f"\ncontext rows forward + backward, {N} anchors, {form}, rows of {width} floats (measured, ms: median [min, max] of {rounds})")
        for name, v in res.items():
            say(f"  {name:<14} {fmt(v)}   peak {peak[name]:.2f} GiB")
        say("  " + ratio("context_rows", res["context_rows"], "sample + cat", res["sample + cat"]))


def quantise(pc, rounds=7, warm=2):
    from gauspcc_amd.anchor_codec import ste_multistep
    from gauspcc_amd.neural_gaussians import quantise_steps

    N = pc.get_anchor.shape[0]
    with torch.no_grad():
        ctx = torch.randn(N, 175, device=DEV)
        xs = [pc._anchor_feat.detach(), pc.get_scaling.detach(), pc._offset.detach()]
        means = [x.mean() for x in xs]
        q0 = (1, 0.001, 0.3)

        def three():
            qs = [q * (1 + torch.tanh(ctx[:, 172 + j:173 + j])) for j, q in enumerate(q0)]
            return ste_multistep(xs[0], qs[0], means[0]), ste_multistep(xs[1], qs[1], means[1]), ste_multistep(xs[2], qs[2].unsqueeze(1), means[2])
        progs = {"quantise_steps": lambda: quantise_steps(xs, q0, ctx[:, -3:], means=means), "3 x ste_multistep": three}
        res, _ = alternate(progs, rounds, warm, lambda fn, r: timed(fn)[1])
    say(f"\nthe three quantisers on {N} anchors (feat 50, scaling 6, offsets 30 columns; measured, ms: median [min, max] of {rounds})")
    for name, v in res.items():
        say(f"  {name:<18} {fmt(v)}")
    say("  " + ratio("quantise_steps", res["quantise_steps"], "3 x ste_multistep", res["3 x ste_multistep"]))


def context_mlp(pc, cam, rounds=5, warm=2):
    from gauspcc_amd.mlp import ContextMLP
    from gauspcc_amd.tcgs_renderer import generate_neural_gaussians

    seq = pc.mlp_triplane
    fused = ContextMLP.from_sequential(seq)

    def run(m):
        pc.mlp_triplane = m
        return generate_neural_gaussians(cam, pc, None, is_training=True, step=12000)
    progs = {"nn.Sequential": lambda: run(seq), "ContextMLP": lambda: run(fused)}
    res, peak = alternate(progs, rounds, warm, one_step)
    pc.mlp_triplane = seq
    say(f"\nthe drop-in's step 12000 by mlp_triplane (603-100-175), {pc.get_anchor.shape[0]} anchors (measured, ms: median [min, max] of {rounds})")
    for name, v in res.items():
        say(f"  {name:<14} forward {fmt([a for a, _ in v])}   backward {fmt([b for _, b in v])}   step {fmt([a + b for a, b in v])}   peak {peak[name]:.2f} GiB")
    say("  step " + ratio("nn.Sequential", [a + b for a, b in res["nn.Sequential"]], "ContextMLP", [a + b for a, b in res["ContextMLP"]]))


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r07_tcgs_train.txt")
    if args[:1] == ["--out"]:
        out, args = args[1], args[2:]
    say(f"tools/tcgs_train_probe.py on {torch.cuda.get_device_name(0)}: every figure below is measured in this run unless it says computed")
    for n in [int(a) for a in args] or [100000, 1000000]:
        pc, cam = model(n)
        steps(pc, cam)
        rows(pc)
        quantise(pc)
        context_mlp(pc, cam)
        N = pc.get_anchor.shape[0]
        say(f"  (computed, not measured: rows of 603 floats are {N * 603 * 4 / 1e9:.2f} GB; the cat's read + write and the backward's contiguous copy "
            f"are {4 * N * 603 * 4 / 1e9:.2f} GB of traffic, {4 * N * 603 * 4 / 6.3e12 * 1e3:.2f} ms at 6.3 TB/s)")
        del pc
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
