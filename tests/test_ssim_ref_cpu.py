"""The float64 restatement of loss_utils.ssim and its closed-form backward (tests/ssim_ref.py), checked on the CPU before any GPU test
relies on them: against the reference's own float32 values and autograd gradients (tests/golden/ssim.npz), against gradcheck, and
against autograd of the float32 formula."""
import os

import numpy as np
import pytest
import torch

from tests import ssim_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim.npz")
CASES = {"a": (11, True), "b": (11, False), "c": (11, True), "d": (7, True)}


def _golden(key):
    g = np.load(GOLDEN)
    src = "a" if key == "d" else key
    x = torch.tensor(g[f"{src}_img1"], dtype=torch.float32) / 255
    y = torch.tensor(g[f"{src}_img2"], dtype=torch.float32) / 255
    return g, x, y


@pytest.mark.parametrize("key", sorted(CASES))
def test_restatement_matches_reference_golden(key):
    ws, sa = CASES[key]
    g, x, y = _golden(key)
    val = ssim_ref.ssim64(x, y, ws, sa)
    assert val.shape == g[f"{key}_ssim"].shape
    np.testing.assert_allclose(val.numpy(), g[f"{key}_ssim"], rtol=0, atol=1e-5)   # the reference's own float32 error on noisy images is ~5e-6
    d1, d2 = ssim_ref.ssim64_grad(x, y, ws, sa, torch.tensor(g[f"{key}_weights"]))
    for name, d in (("grad1", d1), ("grad2", d2)):
        if f"{key}_{name}" not in g:
            continue
        ref = g[f"{key}_{name}"]
        scale = np.abs(ref).max()
        assert np.abs(d.numpy() - ref).max() <= 1e-4 * scale, (key, name)


@pytest.mark.parametrize("shape,ws,sa", [((2, 5, 6), 5, True), ((2, 1, 4, 7), 3, False), ((1, 3, 3), 7, True), ((1, 9, 12), 11, True)])
def test_closed_form_backward_gradcheck(shape, ws, sa):
    x, y = ssim_ref.make_images(shape, seed=7)
    x = x.double().requires_grad_(True)
    y = y.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ssim_ref.SSIM64.apply(a, b, ws, sa), (x, y), eps=1e-6, atol=1e-8, rtol=1e-6)


def test_closed_form_equals_autograd_of_restatement():
    x, y = ssim_ref.make_images((3, 17, 23), seed=1)
    x, y = x.double().requires_grad_(True), y.double().requires_grad_(True)
    ssim_ref.ssim64(x, y, 11).backward()
    d1, d2 = ssim_ref.ssim64_grad(x.detach(), y.detach(), 11)
    assert torch.allclose(d1, x.grad, rtol=0, atol=1e-12 * x.grad.abs().max())
    assert torch.allclose(d2, y.grad, rtol=0, atol=1e-12 * y.grad.abs().max())


def test_float32_formula_near_restatement():
    x, y = ssim_ref.make_images((2, 3, 33, 47), seed=2)
    for sa in (True, False):
        a = ssim_ref.ssim_torch32(x, y, 11, sa)
        b = ssim_ref.ssim64(x, y, 11, sa)
        assert torch.allclose(a.double(), b, rtol=0, atol=1e-5)


def test_taps_are_symmetric_and_normalised():
    for ws in range(1, 32, 2):
        w = ssim_ref.taps(ws)
        assert torch.equal(w, w.flip(0))
        assert abs(float(w.double().sum()) - 1.0) < 1e-6


def test_loss_utils_checks_and_has_no_cpu_path():
    """The drop-in's argument checks run before the device is touched; CPU tensors raise (no CPU fallback)."""
    from gauspcc_amd import loss_utils

    x, y = ssim_ref.make_images((3, 8, 9), seed=0)
    with pytest.raises(RuntimeError):
        loss_utils.ssim(x, y)
    with pytest.raises(RuntimeError):
        loss_utils.photometric_loss(x.requires_grad_(True), y)
    with pytest.raises(TypeError):
        loss_utils.ssim(x.double(), y.double())
    for ws in (0, 4, 33):
        with pytest.raises(ValueError):
            loss_utils.ssim(x, y, ws)
    with pytest.raises(ValueError):
        loss_utils.ssim(x, y[:, :4])
    x, y = x.detach(), y.detach()
    assert torch.equal(loss_utils.l1_loss(x, y), (x - y).abs().mean())
    assert torch.equal(loss_utils.l2_loss(x, y), ((x - y) ** 2).mean())
