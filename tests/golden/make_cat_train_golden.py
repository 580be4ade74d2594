"""Generate tests/golden/cat_train.npz by RUNNING the reference's own CAT-3DGS/gaussian_renderer/__init__.py generate_neural_gaussians
from a checkout of the reference project (not part of this repository):

    python tests/golden/make_cat_train_golden.py <reference checkout>

The runs are tests/cat_train_cases.py's RUNS: training at steps 2000, 5000, 10000, 12000 and -1, one training run under a weighted mask,
one on the small model ([25, 25], flags off), validation at steps 5000, 12000 and -1, and a decoded model.  The renderer is imported under
stubs for diff_gaussian_rasterization, scene.gaussian_model and torchac (make_wiring._module) with its own utils/encodings.py (STE_multistep)
and a torch proxy (make_attr_pins._CpuTorch) whose two random calls are served from the recorded draws, in order, with shape and kind
checked; the rate module is CAT-3DGS's own utils/entropy_models.py Entropy_gaussian.  Everything runs on the CPU in float64 -- the
expectation -- and in float32, which measures the reference's own rounding.

Stored (no reference source text, no weights: inputs_sha256 covers the models, the weights and the draws): per run the float64 outputs cast
to float32 (xyz, color, opacity, scaling, rot of the kept Gaussians in one (kept, 14) table; in training also neural_opacity and the keep
mask), the rate scalars and feat_rate where the reference computes them, per output the reference's float32-vs-float64 difference and the
tolerance in force, max(project tolerance, 4 x that difference): NG_TOL of tests/attr_pin_cases.py (neural_opacity: 2e-5) absolute, and
for the scalars the relative 1e-5.

Asserted: no attribute element can round differently in float32 and float64 (the cap on exclusions is zero); every candidate the mask leaves has
|tanh opacity| >= 1e-4 in what the reference computed (a masked one is exactly 0 in both precisions); the float32 and float64 runs keep the same candidates; the draws are used up exactly;
update_anchor_bound is called once, at step 10000 only; and at training step 12000 five mutations each move some float64 output by at least
100 x its tolerance: means and scales read in HAC's order, base 1.0 instead of 1.1, the second feat group's residual dropped, the offsets
mask dropped, choose_idx not intersected with mask_anchor.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_attr_pins import MAX_FIXTURE_BYTES, _CpuTorch                       # noqa: E402
from make_rate_golden import import_entropy                                   # noqa: E402
from make_wiring import _module, save_npz                                     # noqa: E402
from tests import cat_train_cases as cc                                       # noqa: E402

MUTATIONS = ("hac_order", "base1", "drop_residual", "drop_offset_mask", "no_mask_anchor")


def import_cat_renderer(ref):
    """the reference's renderer with its own utils/encodings.py; call after import_entropy, which leaves a stand-in `utils` behind"""
    sub = os.path.join(ref, "src/gs_compress", "CAT-3DGS")
    for name in [m for m in sys.modules if m == "utils" or m.startswith("utils.") or m == "scene" or m.startswith("scene.")]:
        del sys.modules[name]
    _module("diff_gaussian_rasterization", GaussianRasterizationSettings=object, GaussianRasterizer=object)
    _module("scene", gaussian_model=_module("scene.gaussian_model", GaussianModel=object))
    _module("torchac")
    sys.path.insert(0, sub)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = importlib.util.spec_from_file_location("ref_cat_renderer", os.path.join(sub, "gaussian_renderer/__init__.py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules["ref_cat_renderer"] = mod
            spec.loader.exec_module(mod)
    finally:
        sys.path.remove(sub)
    return mod


class _ReplayTorch(_CpuTorch):
    """the renderer's torch: the two random calls are served from the recorded draws; `tanh` and `split` carry the mutations that change
    the renderer's own expressions"""

    def __init__(self, replay, mutate, F):
        self.replay, self.mutate, self.F = replay, mutate, F

    def empty_like(self, t, *a, **kw):
        replay = self.replay

        class _Pending:
            def uniform_(self, lo, hi):
                assert (lo, hi) == (-0.5, 0.5)
                return replay.uniform_like(t)
        return _Pending()

    def rand_like(self, t, *a, **kw):
        return self.replay.rand_like(t)

    def tanh(self, t):
        return torch.tanh(t) - 0.1 if self.mutate == "base1" else torch.tanh(t)      # 1.1 + (tanh - 0.1) = 1 + tanh

    def split(self, t, split_size_or_sections, dim=0):
        out = torch.split(t, split_size_or_sections, dim=dim)
        if self.mutate == "hac_order" and len(out) == 9:                              # the nine-way split of the context: means first
            out = (out[1], out[0]) + tuple(out[2:])
        return out


def run(mod, ent, arrays, tag, dtype, mutate=None):
    """The reference's function -> ({name: float64 numpy}, keep mask or None, {scalar name: float})"""
    _, name, train, step, wm, decoded = cc.run(tag)
    pc, cam, vis, wmask = cc.model(arrays, name, torch, "cpu", dtype, decoded=decoded)
    pc.entropy_gaussian = ent.Entropy_gaussian(Q=1).to(dtype)
    if mutate == "drop_residual":
        with torch.no_grad():
            for p in pc.get_chcm_mlp_list[0][2].parameters():
                p.zero_()
    if mutate == "drop_offset_mask":       # the rate branch's `binary_grid_masks[choose_idx]` reads ones; the opacity's `.view(-1, 1)` the real mask
        real = pc.get_mask
        pc.get_mask = lambda w=None: _Wrap(real(w))
    if mutate == "no_mask_anchor":
        pc.get_mask_anchor = lambda w=None: torch.ones(pc.get_anchor.shape[0], dtype=torch.bool)
    replay = cc.Replay(arrays, tag, torch)
    mod.torch = _ReplayTorch(replay, mutate, pc.feat_dim)
    with torch.no_grad():
        res = mod.generate_neural_gaussians(cam, pc, vis, is_training=train, step=step, mask=wmask if wm else None)
    assert len(res) == (12 if train else 7) and not replay.queue and replay.served == cc.expected_draws(step, train), (tag, len(replay.queue))
    assert pc.bound_updates == (1 if train and step == 10000 else 0)
    assert pc.feature_net.calls == ([step] if not decoded and (cc.rate_branch(step) if train else (step >= 10000 or step == -1)) else [])
    names = cc.OUTPUTS[:6 if train else 5]
    outs = {k: v.double().numpy() for k, v in zip(names, res)}
    scalars = dict(zip(cc.RATES, res[7:])) if train else dict(feat_rate=res[6])
    scalars = {k: float(v) for k, v in scalars.items() if v is not None and isinstance(v, torch.Tensor)}
    return outs, (res[6].numpy().copy() if train else None), scalars


class _Wrap:
    """get_mask's tensor for the drop_offset_mask mutation: `[visible_mask]` gives an object whose `[choose_idx]` is ones and whose `.view` is the real mask's"""
    def __init__(self, t):
        self.t = t

    def __getitem__(self, idx):
        inner = self.t[idx]

        class _Visible:
            def __getitem__(self, i):
                return torch.ones_like(inner[i])

            def view(self, *a):
                return inner.view(*a)
        return _Visible()


def moves(a, keep_a, ra, b, keep_b, rb, tol):
    """the largest move of any output, in units of its tolerance"""
    if keep_a is not None and not np.array_equal(keep_a, keep_b):
        return np.inf
    worst = max(float(np.abs(a[k] - b[k]).max()) / tol[k] for k in a)
    for k in ra:
        worst = max(worst, abs(ra[k] - rb[k]) / (tol[k] * abs(ra[k])))
    return worst


def main(ref):
    torch.manual_seed(0)
    torch.set_num_threads(1)          # one summation order, whatever the machine
    ent = import_entropy(ref, "CAT-3DGS")
    mod = import_cat_renderer(ref)
    arrays = cc.inputs()
    assert cc.rounding_violations(arrays) == 0
    out = {"inputs_sha256": np.array(cc.sha256_of(arrays)), "runs": np.array([r[0] for r in cc.RUNS])}
    for tag, name, train, step, wm, decoded in cc.RUNS:
        o64, keep, r64 = run(mod, ent, arrays, tag, torch.float64)
        o32, keep32, r32 = run(mod, ent, arrays, tag, torch.float32)
        pre = tag + "/"
        if train:
            margin = float(np.abs(o64["neural_opacity"][o64["neural_opacity"] != 0]).min())
            assert margin >= cc.OPACITY_MARGIN, f"{tag}: a candidate with |tanh opacity| {margin:.2e}"
            assert np.array_equal(keep, keep32) and keep.any() and not keep.all()
            out[pre + "opacity_margin"] = np.float64(margin)
        assert all(o64[k].shape == o32[k].shape for k in o64), tag
        diff = {k: float(np.abs(o64[k] - o32[k]).max()) for k in o64}
        tol = {k: max(cc.OUT_TOL[k], 4 * diff[k]) for k in o64}
        for k in r64:
            diff[k] = abs(r64[k] - r32[k]) / abs(r64[k])
            tol[k] = max(cc.RATE_RTOL, 4 * diff[k])
        out[pre + "out"] = np.concatenate([o64[k] for k in cc.OUTPUTS[:5]], axis=1).astype(np.float32)      # (kept, 3 + 3 + 1 + 3 + 4)
        if train:
            out[pre + "neural_opacity"] = o64["neural_opacity"].astype(np.float32)
            out[pre + "keep"] = np.packbits(keep)
            out[pre + "keep_len"] = np.int64(keep.size)
        names = list(o64) + list(r64)
        out[pre + "names"] = np.array(names)
        out[pre + "f32_vs_f64"] = np.array([diff[k] for k in names])
        out[pre + "tol"] = np.array([tol[k] for k in names])
        out[pre + "rate_names"] = np.array(list(r64), dtype="U32")
        out[pre + "rates"] = np.array([r64[k] for k in r64], np.float64).astype(np.float32)
        print(f"{tag}: {out[pre + 'out'].shape[0]} Gaussians" + (f" of {keep.size} candidates, min |tanh opacity| {margin:.2e}" if train else ""))
        print("  reference float32 vs float64: " + " ".join(f"{k} {diff[k]:.2e}" for k in names))
        print("  tolerance in force:           " + " ".join(f"{k} {tol[k]:.2e}" for k in names))
        if tag == "train12000":
            for mname in MUTATIONS:
                m64, mkeep, mr = run(mod, ent, arrays, tag, torch.float64, mname)
                ratio = moves(o64, keep, r64, m64, mkeep, mr, tol)
                assert ratio >= 100, f"mutation {mname} moves the outputs by only {ratio:.1f} x the tolerance"
                out[pre + f"mutation_{mname}"] = np.float64(min(ratio, 1e30))
                print(f"  mutation {mname}: " + ("another set of Gaussians" if np.isinf(ratio) else f"{ratio:.3g} x the tolerance"))
    path = os.path.join(HERE, "cat_train.npz")
    save_npz(path, out)
    size = os.path.getsize(path)
    assert size <= MAX_FIXTURE_BYTES, f"cat_train.npz: {size} bytes"
    print(f"cat_train.npz: {size} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
