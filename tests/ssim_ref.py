"""Restatements of loss_utils.ssim (HAC/utils/loss_utils.py; the same in HAC++, TC-GS, CAT-3DGS) for the tests of gsr_ssim_*.

* `ssim64` / `ssim64_grad`: the formula in float64 with torch ops only (a separable correlation of zero-padded planes by shifted slices,
  no convolution library), and the closed-form backward of include/gauspcc.h:
      dS/dE[xy] = 2A / (CD),  dS/dE[x^2] = dS/dE[y^2] = -S / D,
      dS/dmu1 = 2 mu2 (B - A) / (CD) + 2 mu1 S (1/D - 1/C),  dS/dmu2 = the same with mu1 and mu2 swapped,
      dL/dx(p) = sum_q w(q - p) g(q) [dS/dmu1(q) + 2 x(p) dS/dE[x^2](q) + y(p) dS/dE[xy](q)]   (q in the image, g = dL/dS).
* `ssim_torch32`: the reference's float32 formula (depthwise conv2d with the 2-D window), on any device, differentiable by autograd:
  the yardstick for the device's float32 error and the torch side of tools/ssim_probe.py.
Taps: float32 exp(-(x - ws // 2)^2 / 4.5) normalised by their float32 sum, as the reference builds them.
"""
import math

import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def taps(window_size):
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def _bchw(t):
    return t if t.dim() == 4 else t.unsqueeze(0)


def correlate(t, w):
    """sum_k w[k] sum_l w[l] t[..., i + k - R, j + l - R] with zeros outside: rows first, then columns (float64 if t is)."""
    R = (w.numel() - 1) // 2
    w = w.to(t.dtype).tolist()
    H, W = t.shape[-2:]
    p = F.pad(t, (R, R, 0, 0))
    h = sum(wk * p[..., :, k:k + W] for k, wk in enumerate(w))
    p = F.pad(h, (0, 0, R, R))
    return sum(wk * p[..., k:k + H, :] for k, wk in enumerate(w))


def moments64(img1, img2, window_size=11):
    x, y = _bchw(img1).double(), _bchw(img2).double()
    w = taps(window_size).double()
    return x, y, w, [correlate(t, w) for t in (x, y, x * x, y * y, x * y)]


def _parts(mu1, mu2, e11, e22, e12):
    A = 2 * mu1 * mu2 + C1
    B = 2 * (e12 - mu1 * mu2) + C2
    C = mu1 * mu1 + mu2 * mu2 + C1
    D = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    return A, B, C, D


def ssim64(img1, img2, window_size=11, size_average=True, maps=False):
    """float64: the mean (0-d) or per-item means (B,); with maps=True also (S map, [dS/dmu1, dS/dE[x^2], dS/dE[xy], dS/dmu2]) in (B, C, H, W)."""
    x, y, w, (mu1, mu2, e11, e22, e12) = moments64(img1, img2, window_size)
    A, B, C, D = _parts(mu1, mu2, e11, e22, e12)
    S = A * B / (C * D)
    val = S.mean() if size_average else S.mean(dim=(1, 2, 3))
    if not maps:
        return val
    m1 = 2 * mu2 * (B - A) / (C * D) + 2 * mu1 * S * (1 / D - 1 / C)
    m2 = -S / D
    m3 = 2 * A / (C * D)
    m4 = 2 * mu1 * (B - A) / (C * D) + 2 * mu2 * S * (1 / D - 1 / C)
    return val, S, [m1, m2, m3, m4]


def ssim64_grad(img1, img2, window_size=11, size_average=True, grad=1.0):
    """Closed-form (dL/dimg1, dL/dimg2) in float64 for L = <grad, ssim64(...)> (grad: a scalar, or (B,) without size_average)."""
    x, y, w, _ = moments64(img1, img2, window_size)
    _, _, (m1, m2, m3, m4) = ssim64(img1, img2, window_size, size_average, maps=True)
    Bn = x.shape[0]
    g = torch.as_tensor(grad, dtype=torch.float64, device=x.device).reshape(-1).expand(1 if size_average else Bn)
    n = x.numel() if size_average else x[0].numel()
    g = (g / n).reshape(-1, 1, 1, 1)
    c1, c2, c3, c4 = (correlate(g * m, w) for m in (m1, m2, m3, m4))
    d1 = c1 + 2 * x * c2 + y * c3
    d2 = c4 + 2 * y * c2 + x * c3
    return d1.reshape(img1.shape), d2.reshape(img2.shape)


class SSIM64(torch.autograd.Function):
    """ssim64 with the closed-form backward, for gradcheck."""

    @staticmethod
    def forward(ctx, img1, img2, window_size, size_average):
        ctx.save_for_backward(img1, img2)
        ctx.ws, ctx.sa = window_size, size_average
        return ssim64(img1, img2, window_size, size_average)

    @staticmethod
    def backward(ctx, grad):
        img1, img2 = ctx.saved_tensors
        d1, d2 = ssim64_grad(img1, img2, ctx.ws, ctx.sa, grad)
        return d1, d2, None, None


def ssim_map_torch32(img1, img2, window_size=11):
    """The reference's float32 S map, (B, C, H, W): five depthwise conv2d with the 2-D window, then the elementwise chain."""
    C = img1.size(-3)
    w1 = taps(window_size).unsqueeze(1)
    win = w1.mm(w1.t()).float().expand(C, 1, window_size, window_size).contiguous().to(img1.device)
    conv = lambda t: F.conv2d(_bchw(t), win, padding=window_size // 2, groups=C)   # noqa: E731
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = conv(img1 * img1) - mu1_sq
    s2 = conv(img2 * img2) - mu2_sq
    s12 = conv(img1 * img2) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def ssim_torch32(img1, img2, window_size=11, size_average=True):
    """The reference's float32 formula: the mean (0-d) or per-item means (B,)."""
    S = ssim_map_torch32(img1, img2, window_size)
    return S.mean() if size_average else S.mean(1).mean(1).mean(1)


def make_images(shape, seed=0, device="cpu"):
    """Deterministic image pairs with structure (smooth gradients, edges, flat bright and dark patches) and noise: (img1, img2) float32."""
    gen = torch.Generator().manual_seed(seed)
    *lead, H, W = shape
    yy = torch.linspace(0, 1, H).view(H, 1)
    xx = torch.linspace(0, 1, W).view(1, W)
    base = 0.5 + 0.3 * torch.sin(6.0 * xx + 4.0 * yy) * torch.cos(3.0 * yy)
    base = base.expand(*lead, H, W).clone()
    base[..., : H // 3, : W // 4] = 0.95                                   # flat bright patch (sigma^2 cancellation)
    base[..., H // 2:, W // 2: W // 2 + max(W // 8, 1)] = 0.02             # dark bar with edges
    img1 = (base + 0.05 * torch.rand(base.shape, generator=gen)).clamp(0, 1)
    img2 = (base + 0.08 * torch.randn(base.shape, generator=gen)).clamp(0, 1)
    return img1.to(device), img2.to(device)
