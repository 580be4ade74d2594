"""CAT-3DGS's training branch on the device: gauspcc_amd.cat_renderer.generate_neural_gaussians(is_training=True, step=12000) against the
float32 torch restatement tests/cat_branch_ref.py on the same GPU, alternating in one process, on SyntheticGaussianModelCAT (feat_dim 50,
10 offsets, groups [12, 12, 13, 13], both channel-context flags on, 80 % of the anchors visible); both sides call the model's own
feature_net, the library's TriPlaneField with a torch head.  Then chain_rate forward + backward alone on the 5 % chosen rows of that
shape against the staged path (torch adds, one `rate` per stage) and against the reference's modules' behaviour (tests/rate_ref.py's
RefEntropy_gaussian: Normal's argument validation and Low_bound's host round trip), with the library's launch count of each.

    python tools/cat_train_probe.py [anchors ...]          (default: 100000 1000000)

Times are device events after warm-up: median [min, max] of the timed rounds.  The loss of a step is sum(xyz) + sum(color) + sum(opacity)
+ sum(scaling) + sum(rot) + bit_per_param + feat_rate; `step` is forward + backward.  profiles/r07_cat_train.txt holds a run.
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
STAGED, REFERENCE = "staged (library rate per stage)", "reference's modules"


def model(n):
    from gauspcc_amd import entropy_models
    from gauspcc_amd.synth import SyntheticGaussianModelCAT

    pc = SyntheticGaussianModelCAT(n, seed=3, device="cuda:0", chcm_for_scaling=True, chcm_for_offsets=True)
    pc.entropy_gaussian = entropy_models.Entropy_gaussian(Q=1, q_floor=1e-9)
    for t in (pc._anchor_feat, pc._offset, pc._scaling, pc._mask):
        t.requires_grad_(True)
    cam = types.SimpleNamespace(camera_center=pc.get_anchor.mean(dim=0).detach() + torch.tensor([0.0, 0.0, -2.0], device=DEV))
    vis = torch.rand(pc.get_anchor.shape[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) < 0.8
    return pc, cam, vis


def launches():
    from gauspcc_amd import _lib
    return _lib.lib().gpcc_debug_launches(0)


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
    loss = sum(o.sum() for o in out[:5]) + out[7] + out[11]
    _, bwd = timed(loss.backward)
    return fwd, bwd


def fmt(v):
    return f"{statistics.median(v):8.2f} [{min(v):.2f}, {max(v):.2f}]"


def compare(n, rounds=5, warm=2):
    from gauspcc_amd.cat_renderer import generate_neural_gaussians
    from tests.cat_branch_ref import ShadowModel, cat_branch_ref

    pc, cam, vis = model(n)
    shadow = ShadowModel(pc, torch.float32, feature_net=pc.feature_net)
    progs = {"drop-in": lambda: generate_neural_gaussians(cam, pc, vis, is_training=True, step=12000),
             "restatement": lambda: cat_branch_ref(cam, shadow, vis, 12000)}
    res = {k: ([], [], 0.0, 0) for k in progs}
    for r in range(warm + rounds):
        for name, run in progs.items():
            torch.cuda.reset_peak_memory_stats()
            before = launches()
            fwd, bwd = one_step(run, r)
            if r >= warm:
                res[name][0].append(fwd); res[name][1].append(bwd)
            res[name] = (*res[name][:2], torch.cuda.max_memory_allocated() / 2 ** 30, launches() - before)
    print(f"\n{pc.get_anchor.shape[0]} anchors, {int(vis.sum())} visible, step 12000 (measured, ms: median [min, max] of {rounds})")
    for name, (fwd, bwd, peak, nl) in res.items():
        print(f"  {name:<12} forward {fmt(fwd)}   backward {fmt(bwd)}   step {fmt([a + b for a, b in zip(fwd, bwd)])}   peak {peak:.2f} GiB   "
              f"library launches counted in the forward thread {nl}")
    d, t = [a + b for a, b in zip(*res["drop-in"][:2])], [a + b for a, b in zip(*res["restatement"][:2])]
    print(f"  step ratio restatement / drop-in: {statistics.median(t) / statistics.median(d):.2f} (spread: drop-in {min(d):.2f}..{max(d):.2f}, restatement {min(t):.2f}..{max(t):.2f})")
    return pc


def chain(pc, reps=10, warm=2):
    """chain_rate forward + backward on 5 % of the anchors: one launch each way, against the staged path and the reference's modules"""
    from gauspcc_amd.cat_renderer import _stages
    from gauspcc_amd.entropy_models import chain_rate, rate
    from tests.cat_branch_ref import chain_rate_staged
    from tests.rate_ref import RefEntropy_gaussian

    F, K = pc.feat_dim, pc.n_offsets
    n = pc.get_anchor.shape[0]
    rows = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) <= 0.05
    with torch.no_grad():
        anchor = pc.get_anchor[rows]
        ctx0 = pc.feature_net(anchor, itr=-1)[0]
        feat0, scl0, off0 = pc._anchor_feat[rows], pc.get_scaling[rows], pc._offset[rows].reshape(-1, 3 * K)
        Q0 = torch.tensor([1.0, 0.001, 0.2], device=DEV) * (1.1 + torch.tanh(ctx0[:, -3:]))
        mask0 = pc.get_mask()[rows]
        stages = _stages(pc)
        res0 = [None if st["mlp"] is None else st["mlp"](feat0[:, :st["dep_ch"]]) for st in stages]
        xm = torch.stack([pc._anchor_feat.mean(), pc.get_scaling.mean(), pc._offset.mean()])
    m = feat0.shape[0]
    ref_mod = RefEntropy_gaussian(Q=1)
    ref_rate = lambda x, means, scales, probs, Q, x_mean, q_floor: ref_mod(x, means[0], scales[0], torch.clamp(Q, min=q_floor), x_mean)   # noqa: E731
    progs = {"chain_rate": lambda a: chain_rate(a[0], a[1], a[2], a[3], a[4], xm, stages, a[6], offset_mask=a[5]),
             STAGED: lambda a: chain_rate_staged(a[0], a[1], a[2], a[3], a[4], xm, stages, a[6], a[5], rate_fn=rate),
             REFERENCE: lambda a: chain_rate_staged(a[0], a[1], a[2], a[3], a[4], xm, stages, a[6], a[5], rate_fn=ref_rate)}
    times = {k: [] for k in progs}
    counts = {}
    for r in range(warm + reps):
        for name, run in progs.items():
            leaf = lambda t: t.detach().clone().requires_grad_(True)   # noqa: E731
            a = [leaf(ctx0), leaf(feat0), leaf(scl0), leaf(off0), leaf(Q0), leaf(mask0), [None if t is None else leaf(t) for t in res0]]
            before = launches()
            (bits, t_f) = timed(lambda: run(a))
            counts[name] = launches() - before
            _, t_b = timed(lambda: bits.sum().backward())
            if r >= warm:
                times[name].append(t_f + t_b)
    print(f"\nchain_rate forward + backward on {m} chosen rows of {n} anchors, {len(stages)} stages (measured, ms: median [min, max] of {reps})")
    for name, v in times.items():
        print(f"  {name:<34} {fmt(v)}   library launches in the forward {counts[name]}")
    base = statistics.median(times["chain_rate"])
    print(f"  ratios to chain_rate: staged {statistics.median(times[STAGED]) / base:.2f}, "
          f"reference's modules {statistics.median(times[REFERENCE]) / base:.2f}")


if __name__ == "__main__":
    for n in [int(a) for a in sys.argv[1:]] or [100000, 1000000]:
        pc = compare(n)
        chain(pc)
        del pc
        torch.cuda.empty_cache()
