"""Generate tests/golden/hacpp_train.npz by RUNNING the reference's own HAC-plus/gaussian_renderer/__init__.py
generate_neural_gaussians(is_training=True, step=s), s in 2000, 5000, 10000 and 12000, from a checkout of the reference project (not part
of this repository):

    python tests/golden/make_hacpp_train_golden.py <reference checkout>

The renderer is imported under make_attr_pins.py's stubs (import_renderer, _CpuTorch); the two rate modules are the reference's own
utils/entropy_models.py Entropy_gaussian_mix_prob_2 and Entropy_gaussian, imported as make_rate_golden.py does.  The model and the recorded
random draws come from tests/hacpp_train_cases.py; the renderer's `torch.empty_like(...).uniform_(-0.5, 0.5)` and `torch.rand_like(...)`
are served from the recorded draws, in order, with shape and kind checked.  It runs on the CPU in float64 -- the expectation -- and in
float32, which measures the reference's own rounding.

Stored (no reference source text, no weights: inputs_sha256 covers the model, the weights and the draws): per step the float64 outputs
cast to float32 (xyz, color, opacity, scaling, rot of the kept Gaussians in one (kept, 14) table, neural_opacity, the keep mask, the four
rate scalars, None stored as absent), per output the reference's float32-vs-float64 difference and the tolerance in force,
max(project tolerance, 4 x that difference): NG_TOL of tests/attr_pin_cases.py (neural_opacity: 2e-5) absolute, and for the rate scalars
the relative 1e-5 of tests/test_gpu_ng_train.py::test_generate_training_matches_reference_branch.

Asserted: every candidate has |tanh opacity| >= 1e-4 in what the reference computed, so nothing is excluded from the comparison; the
float32 and float64 runs keep the same candidates; the draws are used up exactly; and at step 12000 three mutations each move some
float64 output by at least 100 x its tolerance -- two draws exchanged (the feat noise of the chosen anchors and the first rows of the visible
anchors' feat noise trade places), the mask_anchor factor dropped (mask_anchor set to ones), and the nine-way split (every head after
`prob` read feat_dim columns early, which is what HAC's nine-way split reads in the same vector).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_attr_pins import MAX_FIXTURE_BYTES, _CpuTorch, import_renderer     # noqa: E402
from make_rate_golden import import_entropy                                   # noqa: E402
from make_wiring import save_npz                                              # noqa: E402
from tests import hacpp_train_cases as hc                                     # noqa: E402


class _ReplayTorch(_CpuTorch):
    """the renderer's torch: the two random calls are served from the recorded draws"""

    def __init__(self, replay):
        self.replay = replay

    def empty_like(self, t, *a, **kw):
        replay = self.replay

        class _Pending:
            def uniform_(self, lo, hi):
                assert (lo, hi) == (-0.5, 0.5)
                return replay.uniform_like(t)
        return _Pending()

    def rand_like(self, t, *a, **kw):
        return self.replay.rand_like(t)


def run(mod, ent, arrays, step, dtype, mutate=None):
    """The reference's branch -> ({name: float64 numpy}, keep mask, {rate name: float or None})"""
    a = dict(arrays)
    if mutate == "swap_draws":
        d0, d4 = arrays[f"draw_{step}_0"].copy(), arrays[f"draw_{step}_4"].copy()
        d0[:len(d4)], d4[:] = arrays[f"draw_{step}_4"], arrays[f"draw_{step}_0"][:len(d4)]
        a[f"draw_{step}_0"], a[f"draw_{step}_4"] = d0, d4
    pc, cam, vis = hc.model(a, torch, "cpu", dtype)
    if mutate == "drop_mask_anchor":
        pc.get_mask_anchor = torch.ones_like(pc.get_mask_anchor)
    if mutate == "nine_way":             # the same weights read through HAC's nine-way split: every head after `prob` is read feat_dim columns early
        lin = pc.get_grid_mlp[2]
        rolled = torch.nn.Linear(lin.in_features, lin.out_features).to(dtype)
        with torch.no_grad():
            order = list(range(3 * hc.F)) + list(range(2 * hc.F, hc.WIDTH - hc.F))
            rolled.weight.copy_(lin.weight[order]); rolled.bias.copy_(lin.bias[order])
        pc.get_grid_mlp[2] = rolled
    pc.EG_mix_prob_2, pc.entropy_gaussian = ent.Entropy_gaussian_mix_prob_2(Q=1).to(dtype), ent.Entropy_gaussian(Q=1).to(dtype)
    replay = hc.Replay(a, step, torch)
    mod.torch = _ReplayTorch(replay)
    with torch.no_grad():
        res = mod.generate_neural_gaussians(cam, pc, vis, is_training=True, step=step)
    assert len(res) == 11 and not replay.queue, (step, len(replay.queue))
    assert pc.bound_updates == (1 if step == 10000 else 0)
    outs = {k: v.double().numpy() for k, v in zip(hc.OUTPUTS, res[:6])}
    rates = {k: None if v is None else float(v) for k, v in zip(hc.RATES, res[7:])}
    return outs, res[6].numpy().copy(), rates


def moves(a, keep_a, ra, b, keep_b, rb, tol):
    """the largest move of any output, in units of its tolerance"""
    if not np.array_equal(keep_a, keep_b):
        return np.inf
    worst = max(float(np.abs(a[k] - b[k]).max()) / tol[k] for k in hc.OUTPUTS)
    for k in hc.RATES:
        if ra[k] is not None:
            worst = max(worst, abs(ra[k] - rb[k]) / (tol[k] * abs(ra[k])))
    return worst


def main(ref):
    torch.manual_seed(0)
    torch.set_num_threads(1)          # one summation order, whatever the machine
    mod = import_renderer(ref, "hac_plus")
    ent = import_entropy(ref, "HAC-plus")
    arrays = hc.inputs()
    out = {"inputs_sha256": np.array(hc.sha256_of(arrays)), "steps": np.array(hc.STEPS)}
    for step in hc.STEPS:
        o64, keep, r64 = run(mod, ent, arrays, step, torch.float64)
        o32, keep32, r32 = run(mod, ent, arrays, step, torch.float32)
        margin = float(np.abs(o64["neural_opacity"]).min())
        assert margin >= hc.OPACITY_MARGIN, f"step {step}: a candidate with |tanh opacity| {margin:.2e}"
        assert np.array_equal(keep, keep32) and keep.any() and not keep.all()
        diff = {k: float(np.abs(o64[k] - o32[k]).max()) for k in hc.OUTPUTS}
        tol = {k: max(hc.OUT_TOL[k], 4 * diff[k]) for k in hc.OUTPUTS}
        for k in hc.RATES:
            if r64[k] is not None:
                diff[k] = abs(r64[k] - r32[k]) / abs(r64[k])
                tol[k] = max(hc.RATE_RTOL, 4 * diff[k])
        pre = f"step{step}/"
        out[pre + "out"] = np.concatenate([o64[k] for k in hc.OUTPUTS[:5]], axis=1).astype(np.float32)      # (kept, 3 + 3 + 1 + 3 + 4)
        out[pre + "neural_opacity"] = o64["neural_opacity"].astype(np.float32)
        out[pre + "keep"] = np.packbits(keep)
        out[pre + "keep_len"] = np.int64(keep.size)
        out[pre + "opacity_margin"] = np.float64(margin)
        names = list(hc.OUTPUTS) + [k for k in hc.RATES if r64[k] is not None]
        out[pre + "names"] = np.array(names)
        out[pre + "f32_vs_f64"] = np.array([diff[k] for k in names])
        out[pre + "tol"] = np.array([tol[k] for k in names])
        if r64[hc.RATES[0]] is not None:
            out[pre + "rates"] = np.array([r64[k] for k in hc.RATES], np.float64).astype(np.float32)
        print(f"step {step}: {int(keep.sum())} of {keep.size} candidates kept, min |tanh opacity| {margin:.2e}")
        print("  reference float32 vs float64: " + " ".join(f"{k} {diff[k]:.2e}" for k in names))
        print("  tolerance in force:           " + " ".join(f"{k} {tol[k]:.2e}" for k in names))
        if step > 10000:
            for mname in ("swap_draws", "drop_mask_anchor", "nine_way"):
                m64, mkeep, mr = run(mod, ent, arrays, step, torch.float64, mname)
                ratio = moves(o64, keep, r64, m64, mkeep, mr, tol)
                assert ratio >= 100, f"mutation {mname} moves the outputs by only {ratio:.1f} x the tolerance"
                out[pre + f"mutation_{mname}"] = np.float64(min(ratio, 1e30))
                print(f"  mutation {mname}: " + ("another set of Gaussians" if np.isinf(ratio) else f"{ratio:.3g} x the tolerance"))
    path = os.path.join(HERE, "hacpp_train.npz")
    save_npz(path, out)
    size = os.path.getsize(path)
    assert size <= MAX_FIXTURE_BYTES, f"hacpp_train.npz: {size} bytes"
    print(f"hacpp_train.npz: {size} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
