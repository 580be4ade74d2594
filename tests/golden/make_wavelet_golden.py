"""Generate tests/golden/wavelet.npz by IMPORTING the reference's TC-GS/utils/loss_utils.py from a checkout of the reference project (it
is not part of this repository) and running ITS wavelet_loss:

    python tests/golden/make_wavelet_golden.py <reference checkout>

pytorch_wavelets is absent here as everywhere, so the file is imported with sys.modules['pytorch_wavelets'] set to the functional
stand-in of tests/wavelet_ref.py (DWTForward / DWTInverse on the package's published conv2d program).  What this pins is therefore the
reference's own Python -- the branch on step, the weights, the permutes and squeezes -- not the package.

Cases: steps 0, 12000, 25000, 25001 and 30000 on (3, 24, 32), (3, 13, 18) and (3, 37, 41) images of tests/wavelet_ref.make_images with
seeds 1, 1 and 0 (asserted: every |difference coefficient| >= 1e-5 in float64, so no gradient hangs on the sign of a rounded zero).
Every case runs on the CPU in float64 -- the expectation -- and in float32, which measures the reference's own rounding.

Stored (no reference source text): per shape the seed and both float32 images; per case the float64 value and both float64 gradients, the
float32 value, and the largest difference between the float32 run's gradients and the float64 ones.

Asserted: three mutations each change a stored float64 value by more than 1e-6 relative: bands 0 and 1 swapped (step 25001, where their
weights differ), the trailing zero of an odd size dropped (the odd shapes), the `step <= 25000` branch taken at 25001.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_wiring import _module, save_npz      # noqa: E402
from tests import wavelet_ref as wr            # noqa: E402

SHAPES = [(3, 24, 32), (3, 13, 18), (3, 37, 41)]
SEEDS = {(3, 24, 32): 1, (3, 13, 18): 1, (3, 37, 41): 0}
STEPS = [0, 12000, 25000, 25001, 30000]
MAX_FIXTURE_BYTES = 200 * 1024


def key(shape, step):
    return "x".join(map(str, shape)) + f"_s{step}"


def import_loss_utils(ref, **standin):
    """The reference's loss_utils.py with the stand-in (or a mutation of it) in place of pytorch_wavelets."""
    fwd = (lambda J=1, wave="db1", mode="zero": wr.DWTForward(J, wave, mode, **standin))
    _module("pytorch_wavelets", DWTForward=fwd, DWTInverse=wr.DWTInverse)
    path = os.path.join(ref, "src", "gs_compress", "TC-GS", "utils", "loss_utils.py")
    spec = importlib.util.spec_from_file_location("ref_tcgs_loss_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    lu = import_loss_utils(ref)
    out = {}
    values = {}
    for shape in SHAPES:
        name = "x".join(map(str, shape))
        seed = SEEDS[shape]
        x, y = wr.make_images(shape, seed)
        assert wr.min_abs_coef(x, y) >= wr.MIN_COEF, (shape, seed)
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_img1"], out[f"{name}_img2"] = x.numpy(), y.numpy()
        for step in STEPS:
            fn = lambda a, b: lu.wavelet_loss(a, b, step)   # noqa: E731
            v64, g1, g2 = wr.grads(fn, x, y, torch.float64)
            v32, h1, h2 = wr.grads(fn, x, y, torch.float32)
            k = key(shape, step)
            values[k] = float(v64)
            out[f"{k}_value"] = np.float64(v64)
            out[f"{k}_grad1"], out[f"{k}_grad2"] = g1.numpy(), g2.numpy()
            out[f"{k}_value32"] = np.float32(v32)
            out[f"{k}_grad32_err"] = np.array([float((h1.double() - g1).abs().max()), float((h2.double() - g2).abs().max())])
            # the restatement the device is tested against says the same as the reference's own Python
            r64 = float(wr.wavelet_loss64(x, y, step)[0])
            assert abs(r64 - float(v64)) <= 1e-12 * abs(float(v64)), (k, r64, float(v64))

    def moved(mod_fn, k, shape, step):
        x, y = wr.make_images(shape, SEEDS[shape])
        v = float(mod_fn(x.double(), y.double(), step))
        return abs(v - values[k]) > 1e-6 * abs(values[k])

    swapped = import_loss_utils(ref, swap_bands=True)
    assert all(moved(swapped.wavelet_loss, key(s, 25001), s, 25001) for s in SHAPES), "swapping bands 0 and 1 goes unnoticed"
    cropped = import_loss_utils(ref, pad_odd=False)
    assert all(moved(cropped.wavelet_loss, key(s, 12000), s, 12000) for s in SHAPES[1:]), "dropping the odd-size padding goes unnoticed"
    early = lambda a, b, step: wr.wavelet_loss(a, b, step, late_after=25001)   # noqa: E731
    assert all(moved(early, key(s, 25001), s, 25001) for s in SHAPES), "the other branch at 25001 goes unnoticed"
    assert not moved(lambda a, b, step: wr.wavelet_loss(a, b, step), key(SHAPES[0], 25001), SHAPES[0], 25001)

    path = os.path.join(HERE, "wavelet.npz")
    save_npz(path, out)
    assert os.path.getsize(path) <= MAX_FIXTURE_BYTES, os.path.getsize(path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, seeds {[int(out['x'.join(map(str, s)) + '_seed']) for s in SHAPES]}")


if __name__ == "__main__":
    main(sys.argv[1])
