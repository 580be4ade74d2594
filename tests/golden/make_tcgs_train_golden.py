"""Generate tests/golden/tcgs_train.npz by RUNNING the reference's own TC-GS/gaussian_renderer/__init__.py generate_neural_gaussians
from a checkout of the reference project (not part of this repository):

    python tests/golden/make_tcgs_train_golden.py <reference checkout>

The runs are tests/tcgs_train_cases.py's RUNS: training at steps 2000, 5000, 10000, 12000, 15000 and 20000 over all anchors, one training
run with a visible mask at step 12000, validation of an un-decoded and of a decoded model.  The renderer is imported under stubs for
diff_gaussian_rasterization, scene.gaussian_model, torchac and pytorch_wavelets (make_wiring._module) with its own utils/encodings.py
(STE_multistep) and utils/loss_utils.py (l1_loss) and a torch proxy (make_attr_pins._CpuTorch) whose two random calls are served from the
recorded draws, in order, with shape and kind checked; the rate module is TC-GS's own utils/entropy.py Entropy_gaussian.  Everything runs on
the CPU in float64 -- the expectation -- and in float32, which measures the reference's own rounding.

Stored (no reference source text, no weights: inputs_sha256 covers the model, the weights and the draws): per run the float64 outputs cast
to float32 (xyz, color, opacity, scaling, rot of the kept Gaussians in one (kept, 14) table; in training also neural_opacity and the keep
mask), the rate scalars and lae where the reference computes them, per output the reference's float32-vs-float64 difference and the
tolerance in force, max(project tolerance, 4 x that difference): NG_TOL of tests/attr_pin_cases.py (neural_opacity: 2e-5) absolute, and
for the scalars the relative 1e-5.

Asserted: no attribute element can round differently in float32 and float64 (the cap on exclusions is zero); every candidate the mask leaves
has |tanh opacity| >= 1e-4 in what the reference computed; the float32 and float64 runs keep the same candidates; the draws are used up
exactly; updatebbox is called at step 10000 only and init_knn_indice(4) at step 15000 only; and at training step 20000 six mutations each
move some float64 output by at least 100 x its tolerance: Q_offsets 0.2 instead of 0.3, threshold 0.05 instead of 0.15, choose_idx not
intersected with mask_anchor, the offsets mask dropped, the repeat form in place of knnanchor, the mask_anchor_rate factor dropped.
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
from make_wiring import _module, save_npz                                     # noqa: E402
from tests import tcgs_train_cases as tc                                      # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_tcgs(ref):
    """(the reference's renderer with its own utils/encodings.py and utils/loss_utils.py, its utils/entropy.py)"""
    sub = os.path.join(ref, "src/gs_compress", "TC-GS")
    for name in [m for m in sys.modules if m == "utils" or m.startswith("utils.") or m == "scene" or m.startswith("scene.")]:
        del sys.modules[name]
    _module("diff_gaussian_rasterization", GaussianRasterizationSettings=object, GaussianRasterizer=object)
    _module("scene", gaussian_model=_module("scene.gaussian_model", GaussianModel=object))
    _module("torchac")
    _module("pytorch_wavelets", DWTForward=object, DWTInverse=object)
    sys.path.insert(0, sub)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mod = _load(os.path.join(sub, "gaussian_renderer/__init__.py"), "ref_tcgs_renderer")
            ent = _load(os.path.join(sub, "utils/entropy.py"), "ref_tcgs_entropy")
    finally:
        sys.path.remove(sub)
    return mod, ent


class _ReplayTorch(_CpuTorch):
    """the renderer's torch: the two random calls are served from the recorded draws; they carry the mutations that change the renderer's
    own constants (u_offsets x 2 / 3 is the noise of Q_offsets = 0.2; 3 r <= 0.15 is r <= 0.05)"""

    def __init__(self, replay, mutate):
        self.replay, self.mutate, self.uniforms = replay, mutate, 0

    def empty_like(self, t, *a, **kw):
        proxy = self

        class _Pending:
            def uniform_(self, lo, hi):
                assert (lo, hi) == (-0.5, 0.5)
                u = proxy.replay.uniform_like(t)
                proxy.uniforms += 1
                return u * (2.0 / 3.0) if proxy.mutate == "q_offsets02" and proxy.uniforms == 3 else u
        return _Pending()

    def rand_like(self, t, *a, **kw):
        r = self.replay.rand_like(t)
        return r * 3 if self.mutate == "threshold005" else r


class _MaskOnes:
    """get_mask's tensor for drop_offset_mask: `[visible_mask]` gives an object whose `[choose_idx]` is ones and whose `.view` is the real mask's"""
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


class _AnchorMask:
    """get_mask_anchor's tensor with one of its two uses replaced: the bool the chosen are intersected with (ones), or the rate factor (1)"""
    def __init__(self, t, mutate):
        self.t, self.mutate = t, mutate

    def __getitem__(self, idx):
        inner, mutate = self.t[idx], self.mutate

        class _Visible:
            def to(self, *a, **kw):
                return torch.ones_like(inner) if mutate == "no_mask_anchor" else inner.to(*a, **kw)

            def sum(self):
                return torch.tensor(inner.numel()) if mutate == "no_rate_factor" else inner.sum()

            def numel(self):
                return inner.numel()
        return _Visible()


def run(mod, ent, arrays, tag, dtype, mutate=None):
    """The reference's function -> ({name: float64 numpy}, keep mask or None, {scalar name: float})"""
    _, train, step, with_vis, decoded = tc.run(tag)
    pc, cam, vis = tc.model(arrays, torch, "cpu", dtype, decoded=decoded)
    ent_mod = ent.Entropy_gaussian(Q=1).to(dtype)
    pc.entropy_gaussian = ent_mod
    cls = type(pc)
    if mutate == "q_offsets02":      # the third rate term's step: 0.2 (1 + tanh) = 2 / 3 of the renderer's
        calls = []

        class _Ent:
            def forward(self, x, mean, scale, Q=None, x_mean=None):
                calls.append(1)
                return ent_mod.forward(x, mean, scale, Q * (2.0 / 3.0) if len(calls) == 3 else Q, x_mean)
        pc.entropy_gaussian = _Ent()
    if mutate == "drop_offset_mask":
        real = pc.get_mask
        cls.get_mask = property(lambda self: _MaskOnes(real))
    if mutate in ("no_mask_anchor", "no_rate_factor"):
        real_a = pc.get_mask_anchor
        cls.get_mask_anchor = property(lambda self: _AnchorMask(real_a, mutate))
    if mutate == "repeat_form":
        pc.knnanchor = pc.get_anchor.unsqueeze(1).repeat(1, tc.KNN, 1)
    replay = tc.Replay(arrays, tag, torch)
    mod.torch = _ReplayTorch(replay, mutate)
    with torch.no_grad():
        res = mod.generate_neural_gaussians(cam, pc, vis if with_vis else None, is_training=train, step=step)
    assert len(res) == (12 if train else 6) and not replay.queue and replay.served == tc.expected_draws(step, train), (tag, len(replay.queue))
    assert pc.hooks == tc.expected_hooks(step, train), (tag, pc.hooks)
    assert pc.triplane.calls == ([(True, step)] if train and step > 10000 else [(False, 0)] if not train and not decoded else []), (tag, pc.triplane.calls)
    names = tc.OUTPUTS[:6 if train else 5]
    outs = {k: v.double().numpy() for k, v in zip(names, res)}
    scalars = {k: float(v) for k, v in (zip(tc.RATES, res[7:]) if train else ()) if v is not None}
    return outs, (res[6].numpy().copy() if train else None), scalars


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
    mod, ent = import_tcgs(ref)
    assert mod.K == tc.KNN
    arrays = tc.inputs()
    assert tc.rounding_violations(arrays) == 0
    out = {"inputs_sha256": np.array(tc.sha256_of(arrays)), "runs": np.array([r[0] for r in tc.RUNS])}
    for tag, train, step, with_vis, decoded in tc.RUNS:
        o64, keep, r64 = run(mod, ent, arrays, tag, torch.float64)
        o32, keep32, r32 = run(mod, ent, arrays, tag, torch.float32)
        pre = tag + "/"
        if train:
            margin = float(np.abs(o64["neural_opacity"][o64["neural_opacity"] != 0]).min())
            assert margin >= tc.OPACITY_MARGIN, f"{tag}: a candidate with |tanh opacity| {margin:.2e}"
            assert np.array_equal(keep, keep32) and keep.any() and not keep.all()
            out[pre + "opacity_margin"] = np.float64(margin)
            assert set(r64) == (set(tc.RATES) if step > 15000 else set(tc.RATES[:4]) if step > 10000 else set()), (tag, sorted(r64))
        assert all(o64[k].shape == o32[k].shape for k in o64), tag
        diff = {k: float(np.abs(o64[k] - o32[k]).max()) for k in o64}
        tol = {k: max(tc.OUT_TOL[k], 4 * diff[k]) for k in o64}
        for k in r64:
            diff[k] = abs(r64[k] - r32[k]) / abs(r64[k])
            tol[k] = max(tc.RATE_RTOL, 4 * diff[k])
        out[pre + "out"] = np.concatenate([o64[k] for k in tc.OUTPUTS[:5]], axis=1).astype(np.float32)      # (kept, 3 + 3 + 1 + 3 + 4)
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
        if tag == "train20000":
            for mname in tc.MUTATIONS:
                m64, mkeep, mr = run(mod, ent, arrays, tag, torch.float64, mname)
                ratio = moves(o64, keep, r64, m64, mkeep, mr, tol)
                assert ratio >= 100, f"mutation {mname} moves the outputs by only {ratio:.1f} x the tolerance"
                out[pre + f"mutation_{mname}"] = np.float64(min(ratio, 1e30))
                print(f"  mutation {mname}: " + ("another set of Gaussians" if np.isinf(ratio) else f"{ratio:.3g} x the tolerance"))
    path = os.path.join(HERE, "tcgs_train.npz")
    save_npz(path, out)
    size = os.path.getsize(path)
    assert size <= MAX_FIXTURE_BYTES, f"tcgs_train.npz: {size} bytes"
    print(f"tcgs_train.npz: {size} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
