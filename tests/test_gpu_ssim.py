"""gsr_ssim_forward / gsr_ssim_backward (gauspcc_amd.loss_utils) on the device: values, derivative maps and gradients against the float64
restatement (tests/ssim_ref.py) with a tolerance calibrated by the float32 torch formula's own error on the same inputs; the reference's
golden values; bitwise repeatability; edge cases and errors; photometric_loss; a short optimisation against the torch formula."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gauspcc_amd import loss_utils
from gauspcc_amd.loss_utils import photometric_loss, ssim
from tests import ssim_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(3, 1060, 1600), (3, 800, 800), (3, 37, 53), (1, 1, 61, 95), (4, 3, 67, 45)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim.npz")


def _maps32(x, y, ws):
    """The closed-form maps from float32 conv2d moments: the float32 torch formula's own error, for calibration."""
    C = x.shape[1]
    w1 = ssim_ref.taps(ws).unsqueeze(1)
    win = w1.mm(w1.t()).expand(C, 1, ws, ws).contiguous().to(x.device)
    conv = lambda t: F.conv2d(t, win, padding=ws // 2, groups=C)   # noqa: E731
    mu1, mu2, e11, e22, e12 = conv(x), conv(y), conv(x * x), conv(y * y), conv(x * y)
    A = 2 * (mu1 * mu2) + ssim_ref.C1
    B = 2 * (e12 - mu1 * mu2) + ssim_ref.C2
    Cc = (mu1 * mu1 + mu2 * mu2) + ssim_ref.C1
    D = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + ssim_ref.C2
    S = A * B / (Cc * D)
    return [2 * mu2 * (B - A) / (Cc * D) + 2 * mu1 * S * (1 / D - 1 / Cc), -S / D, 2 * A / (Cc * D),
            2 * mu1 * (B - A) / (Cc * D) + 2 * mu2 * S * (1 / D - 1 / Cc)]


def _err(a, ref):
    return float((a.double() - ref).abs().max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_float64(shape):
    x, y = ssim_ref.make_images(shape, seed=sum(shape), device=DEV)
    ws = 11
    sa = len(shape) == 3
    x4, y4 = ssim_ref._bchw(x), ssim_ref._bchw(y)
    # values
    v64 = ssim_ref.ssim64(x, y, ws, sa)
    v = ssim(x, y, ws, sa)
    assert v.shape == v64.shape and v.dtype == torch.float32
    assert _err(v, v64) <= 1e-6
    # maps
    _, _, m64 = ssim_ref.ssim64(x, y, ws, sa, maps=True)
    _, _, _, maps = loss_utils._forward(x4.contiguous(), y4.contiguous(), ws, sa, 4)
    m32 = _maps32(x4, y4, ws)
    for k in range(4):
        assert _err(maps[k], m64[k]) <= 2 * _err(m32[k], m64[k]) + 1e-6, k
    # gradients: HIP against the closed form, calibrated by float32 autograd of the torch formula
    g = torch.tensor(1.0) if sa else torch.linspace(-1.0, 2.0, shape[0])
    d64 = ssim_ref.ssim64_grad(x, y, ws, sa, g.to(DEV))
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (ssim(a, b, ws, sa) * g.to(DEV)).sum().backward()
    a32, b32 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (ssim_ref.ssim_torch32(a32, b32, ws, sa) * g.to(DEV)).sum().backward()
    for hip, t32, ref in ((a.grad, a32.grad, d64[0]), (b.grad, b32.grad, d64[1])):
        scale = float(ref.abs().max())
        assert _err(hip, ref) <= 2 * _err(t32, ref) + 1e-6 * scale


def test_reference_golden():
    g = np.load(GOLDEN)
    for key, (ws, sa) in {"a": (11, True), "b": (11, False), "c": (11, True), "d": (7, True)}.items():
        src = "a" if key == "d" else key
        x = (torch.tensor(g[f"{src}_img1"], dtype=torch.float32) / 255).to(DEV).requires_grad_(True)
        y = (torch.tensor(g[f"{src}_img2"], dtype=torch.float32) / 255).to(DEV).requires_grad_(True)
        s = ssim(x, y, ws, sa)
        assert tuple(s.shape) == g[f"{key}_ssim"].shape
        np.testing.assert_allclose(s.detach().cpu().numpy(), g[f"{key}_ssim"], rtol=0, atol=1e-5)
        (s * torch.tensor(g[f"{key}_weights"], device=DEV)).sum().backward()
        for name, t in (("grad1", x), ("grad2", y)):
            if f"{key}_{name}" in g:
                ref = g[f"{key}_{name}"]
                assert np.abs(t.grad.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max(), (key, name)


def _run(x, y, sa=True):
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    s = ssim(a, b, 11, sa)
    s.sum().backward()
    return s.detach(), a.grad, b.grad


def test_bitwise_repeatable_and_across_streams():
    x, y = ssim_ref.make_images((2, 3, 300, 410), seed=5, device=DEV)
    ref = _run(x, y, False)
    again = _run(x, y, False)
    for u, v in zip(ref, again):
        assert torch.equal(u, v)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    torch.cuda.synchronize()
    for i in range(4):
        with torch.cuda.stream(s1 if i % 2 == 0 else s2):
            outs.append(_run(x, y, False))
    torch.cuda.synchronize()
    for o in outs:
        for u, v in zip(ref, o):
            assert torch.equal(u, v)
    loss = [photometric_loss(x.clone().requires_grad_(True), y) for _ in range(2)]
    assert all(torch.equal(p, q) for p, q in zip(loss[0], loss[1]))


def test_identical_images_give_one_and_zero_gradient():
    x, _ = ssim_ref.make_images((2, 3, 70, 90), seed=3, device=DEV)
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    s = ssim(a, b)
    assert float(s.detach()) == 1.0
    s.backward()
    assert torch.equal(a.grad, torch.zeros_like(x)) and torch.equal(b.grad, torch.zeros_like(x))
    a = x.clone().requires_grad_(True)
    loss, l1, sv = photometric_loss(a, x)
    assert float(loss.detach()) == 0.0 and float(l1) == 0.0 and float(sv) == 1.0
    loss.backward()
    assert torch.equal(a.grad, torch.zeros_like(x))


def test_zero_images_nan_and_small_images():
    z = torch.zeros((3, 20, 30), device=DEV)
    assert float(ssim(z, z)) == 1.0
    x, y = ssim_ref.make_images((3, 20, 30), seed=4, device=DEV)
    xn = x.clone()
    xn[1, 5, 7] = float("nan")
    a = xn.clone().requires_grad_(True)
    s = ssim(a, y)
    assert torch.isnan(s)
    s.backward()
    torch.cuda.synchronize()
    assert torch.isnan(a.grad).any()
    for shape, ws in (((3, 5, 7), 11), ((1, 1, 1, 1), 11), ((2, 2, 3, 40), 31), ((1, 4, 9), 1)):
        x, y = ssim_ref.make_images(shape, seed=6, device=DEV)
        sa = len(shape) == 3
        v = ssim(x, y, ws, sa)
        assert _err(v, ssim_ref.ssim64(x, y, ws, sa)) <= 1e-6, (shape, ws)


def test_shapes_and_non_contiguous():
    x, y = ssim_ref.make_images((4, 3, 40, 50), seed=8, device=DEV)
    assert ssim(x, y).shape == () and ssim(x, y, size_average=False).shape == (4,)
    assert ssim(x[0], y[0]).shape == ()
    r = torch.cat([x, torch.ones_like(x[:, :1])], dim=1)   # render[:, :3] of a 4-channel render
    assert torch.equal(ssim(r[:, :3], y), ssim(x, y))
    a = r.clone().requires_grad_(True)
    ssim(a[:, :3], y).backward()
    b = x.clone().requires_grad_(True)
    ssim(b, y).backward()
    assert torch.equal(a.grad[:, :3], b.grad) and not a.grad[:, 3].any()
    with torch.no_grad():
        assert torch.equal(ssim(x.clone().requires_grad_(True), y), ssim(x, y))


def test_errors():
    x, y = ssim_ref.make_images((3, 16, 16), seed=9, device=DEV)
    with pytest.raises(IndexError):
        ssim(x, y, size_average=False)
    for ws in (0, 2, 10, 33):
        with pytest.raises(ValueError):
            ssim(x, y, ws)
    with pytest.raises(TypeError):
        ssim(x.double(), y.double())
    with pytest.raises(TypeError):
        ssim(x.half(), y)
    with pytest.raises(RuntimeError):
        ssim(x.cpu(), y.cpu())
    with pytest.raises(ValueError):
        ssim(x, y[:, :8])


def test_photometric_loss_matches_parts():
    x, y = ssim_ref.make_images((3, 123, 211), seed=10, device=DEV)
    for lam in (0.2, 0.0, 1.0, 0.35):
        a = x.clone().requires_grad_(True)
        loss, l1, sv = photometric_loss(a, y, lam)
        assert not l1.requires_grad and not sv.requires_grad and loss.requires_grad
        assert torch.equal(sv, ssim(x, y))
        assert float((l1 - loss_utils.l1_loss(x, y)).abs()) <= 1e-7
        assert torch.equal(loss, (1.0 - lam) * l1 + lam * (1.0 - sv))
        loss.backward()
        b = x.clone().requires_grad_(True)
        ref = (1.0 - lam) * loss_utils.l1_loss(b, y) + lam * (1.0 - ssim(b, y))
        ref.backward()
        assert float((a.grad - b.grad).abs().max()) <= 1e-6 * float(b.grad.abs().max())


def test_short_optimisation_follows_torch_formula():
    target, start = ssim_ref.make_images((3, 96, 128), seed=11, device=DEV)
    start = (0.5 * start + 0.25).contiguous()
    runs = []
    for formula in ("hip", "torch"):
        p = start.clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=1e-2)
        losses = []
        for _ in range(100):
            opt.zero_grad()
            if formula == "hip":
                loss = photometric_loss(p, target)[0]
            else:
                loss = 0.8 * loss_utils.l1_loss(p, target) + 0.2 * (1.0 - ssim_ref.ssim_torch32(p, target))
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        runs.append((p.detach(), losses))
    (ph, lh), (pt, lt) = runs
    assert lh[-1] < 0.5 * lh[0]
    assert abs(lh[-1] - lt[-1]) <= 1e-2 * lt[-1], (lh[-1], lt[-1])
    # Adam divides by sqrt(v): where the L1 sign flips at the target a last-bit difference becomes a step of up to lr, so the images agree
    # to about 1 % of a step on average and to about one step at worst (measured: 1.4e-4 and 6.6e-3 at lr 1e-2)
    d = (ph - pt).abs()
    assert float(d.mean()) <= 5e-4 and float(d.max()) <= 2e-2, (float(d.mean()), float(d.max()))
