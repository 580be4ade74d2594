"""Restatements of TC-GS's wavelet_loss (TC-GS/utils/loss_utils.py:66-83) and of the two pytorch_wavelets modules it is built on, for the
tests of gsr_wavelet_l1_* / gsr_haar_* (gauspcc_amd.loss_utils.wavelet_loss, gauspcc_amd.wavelets).

* `dwt_quads`: the Haar DWT (zero mode) by its 2 x 2 quads, a b / c d -> LL = (a+b+c+d)/2, band0 = (a+b-c-d)/2, band1 = (a-b+c-d)/2,
  band2 = (a-b-c+d)/2, level after level on a plane zero-filled to an even size: the restatement, meant for float64.
* `dwt_conv` / `idwt_conv`: the program pytorch_wavelets would execute as its published algorithm reads (lowlevel.afb1d / sfb1d: a
  grouped stride-2 conv2d with the reversed two-tap filters per pass, row pass first, one trailing zero when a dimension is odd), in the
  input's dtype: in float32 the yardstick of the device's float32 error and the torch side of tools/wavelet_probe.py.
* `DWTForward` / `DWTInverse`: a functional stand-in for the package's modules on that program (filters are made per call in the input's
  dtype and on its device, so `.to('cuda')` moves nothing), for importing the reference's loss_utils.py where the package is absent.
* `wavelet_loss`: the reference's formula on any such pair of modules; `wavelet_loss64`: it on `dwt_quads` in float64.
The package itself cannot be imported here: its arithmetic, the sign of the high-pass filter and the band order are stated, not pinned.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

S = 0.7071067811865476   # pywt.Wavelet('haar').dec_lo[0]
MIN_COEF = 1e-5          # gradient comparisons need every |difference coefficient| at least this (20 x the float32 coefficient error)


# ------------------------------------------------------------------ the restatement: quads
def _quads(x):
    H, W = x.shape[-2:]
    p = F.pad(x, (0, W % 2, 0, H % 2))
    return p[..., 0::2, 0::2], p[..., 0::2, 1::2], p[..., 1::2, 0::2], p[..., 1::2, 1::2]


def dwt_quads(x, J=2):
    """(Yl (..., h_J, w_J), [Yh_j (..., 3, h_j, w_j)], finest first) of x (..., H, W), in x's dtype."""
    yh = []
    ll = x
    for _ in range(J):
        a, b, c, d = _quads(ll)
        ll = (a + b + c + d) / 2
        yh.append(torch.stack([(a + b - c - d) / 2, (a - b + c - d) / 2, (a - b - c + d) / 2], dim=-3))
    return ll, yh


def idwt_quads(ll, yh):
    """The inverse of dwt_quads, not cropped: (..., 2 h_1, 2 w_1)."""
    for high in yh[::-1]:
        h, w = high.shape[-2:]
        ll = ll[..., :h, :w]
        b0, b1, b2 = high.unbind(dim=-3)
        out = ll.new_zeros(ll.shape[:-2] + (2 * h, 2 * w))
        out[..., 0::2, 0::2] = (ll + b0 + b1 + b2) / 2
        out[..., 0::2, 1::2] = (ll + b0 - b1 - b2) / 2
        out[..., 1::2, 0::2] = (ll - b0 + b1 - b2) / 2
        out[..., 1::2, 1::2] = (ll - b0 - b1 + b2) / 2
        ll = out
    return ll


# ------------------------------------------------------------------ the conv2d program
def _filters(x, dim):
    """[lo, hi] per channel for one pass along `dim` of a (B, C, H, W): the reversed decomposition filters, dec_hi = [-s, s]."""
    C = x.shape[1]
    lo = torch.tensor([S, S], dtype=x.dtype, device=x.device)
    hi = torch.tensor([S, -S], dtype=x.dtype, device=x.device)
    shape = [1, 1, 1, 1]
    shape[dim] = 2
    return torch.cat([lo.reshape(shape), hi.reshape(shape)] * C, dim=0)


def afb1d(x, dim, pad_odd=True):
    """One analysis pass of (B, C, H, W) along dim 2 or 3: (B, 2C, ., .) with channels [lo, hi] per input channel."""
    if x.shape[dim] % 2 and pad_odd:
        x = F.pad(x, (0, 0, 0, 1) if dim == 2 else (0, 1, 0, 0))
    return F.conv2d(x, _filters(x, dim), stride=(2, 1) if dim == 2 else (1, 2), groups=x.shape[1])


def sfb1d(lo, hi, dim):
    """One synthesis pass: the transposed convolutions of lo and hi with the reconstruction filters, summed."""
    C = lo.shape[1]
    shape = [1, 1, 1, 1]
    shape[dim] = 2
    g0 = torch.tensor([S, S], dtype=lo.dtype, device=lo.device).reshape(shape).repeat(C, 1, 1, 1)
    g1 = torch.tensor([S, -S], dtype=lo.dtype, device=lo.device).reshape(shape).repeat(C, 1, 1, 1)
    stride = (2, 1) if dim == 2 else (1, 2)
    return F.conv_transpose2d(lo, g0, stride=stride, groups=C) + F.conv_transpose2d(hi, g1, stride=stride, groups=C)


def dwt_conv(x, J=2, swap_bands=False, pad_odd=True):
    """(Yl, [Yh_j]) of x (B, C, H, W) by the conv2d program.  swap_bands / pad_odd=False are the mutations of the fixture generator."""
    yh = []
    ll = x
    for _ in range(J):
        y = afb1d(afb1d(ll, 3, pad_odd), 2, pad_odd)       # channels per input channel: [lo lo, lo hi(height), hi(width) lo, hi hi]
        B, C4, h, w = y.shape
        y = y.reshape(B, C4 // 4, 4, h, w)
        ll = y[:, :, 0].contiguous()
        high = y[:, :, 1:].contiguous()
        if swap_bands:
            high = high[:, :, [1, 0, 2]].contiguous()
        yh.append(high)
    return ll, yh


def idwt_conv(yl, yh):
    ll = yl
    for high in yh[::-1]:
        if high is None:
            high = ll.new_zeros(ll.shape[:2] + (3,) + ll.shape[2:])
        if ll.shape[-2] > high.shape[-2]:
            ll = ll[..., :-1, :]
        if ll.shape[-1] > high.shape[-1]:
            ll = ll[..., :-1]
        b0, b1, b2 = high.unbind(dim=2)
        lo = sfb1d(ll, b0, 2)
        hi = sfb1d(b1, b2, 2)
        ll = sfb1d(lo, hi, 3)
    return ll


class DWTForward:
    """The stand-in for pytorch_wavelets.DWTForward (Haar, zero mode)."""

    def __init__(self, J=1, wave="db1", mode="zero", swap_bands=False, pad_odd=True):
        assert wave in ("haar", "db1") and mode == "zero"
        self.J, self.swap_bands, self.pad_odd = J, swap_bands, pad_odd

    def to(self, *args, **kwargs):
        return self

    def __call__(self, x):
        return dwt_conv(x, self.J, self.swap_bands, self.pad_odd)


class DWTInverse:
    """The stand-in for pytorch_wavelets.DWTInverse (Haar, zero mode)."""

    def __init__(self, wave="db1", mode="zero"):
        assert wave in ("haar", "db1") and mode == "zero"

    def to(self, *args, **kwargs):
        return self

    def __call__(self, coeffs):
        return idwt_conv(*coeffs)


# ------------------------------------------------------------------ the loss
def band_weights(step, late_after=25000):
    """The weight of each band's L1 mean in the order LL2, level-1 bands 0..2, level-2 bands 0..2."""
    fine, coarse = 1.0 - step / 30000, step / 30000
    if step > late_after:
        return [0.0] + [k * fine for k in (0.4, 0.3, 0.3)] + [k * coarse for k in (0.4, 0.3, 0.3)]
    return [fine] + [0.2 * coarse] * 6


def band_l1(yl1, yh1, yl2, yh2):
    """The seven L1 means between two transforms of one image each ((1, C, ...) coefficients)."""
    out = [(yl1 - yl2).abs().mean()]
    for level in (0, 1):
        out += [(yh1[level][:, :, k] - yh2[level][:, :, k]).abs().mean() for k in range(3)]
    return out


def wavelet_loss(img1, img2, step=0, xfm=None, late_after=25000):
    """The reference's formula on (C, H, W) images with `xfm` a two-level DWTForward (default: the conv2d program)."""
    xfm = xfm or DWTForward(J=2, wave="haar", mode="zero")
    yl1, yh1 = xfm(img1.unsqueeze(0))
    yl2, yh2 = xfm(img2.unsqueeze(0))
    means = band_l1(yl1, yh1, yl2, yh2)
    return sum(w * m for w, m in zip(band_weights(step, late_after), means) if w != 0.0)


def wavelet_loss64(img1, img2, step=0):
    """float64, on the quads: (loss, the seven band means)."""
    yl1, yh1 = dwt_quads(img1.double().unsqueeze(0))
    yl2, yh2 = dwt_quads(img2.double().unsqueeze(0))
    means = band_l1(yl1, yh1, yl2, yh2)
    return sum(w * m for w, m in zip(band_weights(step), means) if w != 0.0), torch.stack(means)


def grads(fn, img1, img2, dtype):
    """(value, d/d img1, d/d img2) of fn(img1, img2) by autograd in `dtype`."""
    a = img1.detach().to(dtype).requires_grad_(True)
    b = img2.detach().to(dtype).requires_grad_(True)
    v = fn(a, b)
    v.backward()
    return v.detach(), a.grad, b.grad


# ------------------------------------------------------------------ inputs
def make_images(shape, seed=0, device="cpu"):
    """tests/golden/make_ssim_golden.images without its rounding to 1/255: (img1, img2) float32."""
    rng = np.random.default_rng(seed)
    *lead, H, W = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = 0.5 + 0.35 * np.sin(7 * xx + 3 * yy)
    base = np.broadcast_to(base, shape).copy()
    base[..., : H // 3, : W // 4] = 0.9
    a = np.clip(base + 0.06 * rng.standard_normal(shape), 0, 1)
    b = np.clip(base + 0.1 * rng.standard_normal(shape), 0, 1)
    return torch.tensor(a, dtype=torch.float32).to(device), torch.tensor(b, dtype=torch.float32).to(device)


def diff_coefs64(img1, img2):
    """The float64 two-level coefficients of img1 - img2 (the transform is linear): (LL2, level-1 bands, level-2 bands)."""
    ll, yh = dwt_quads(img1.double().cpu() - img2.double().cpu())
    return ll, yh[0], yh[1]


def min_abs_coef(img1, img2):
    return min(float(t.abs().min()) for t in diff_coefs64(img1, img2))


@functools.lru_cache(maxsize=None)
def pick_seed(shape):
    """The first seed in 0..15 whose images have every |difference coefficient| >= MIN_COEF in float64."""
    for seed in range(16):
        if min_abs_coef(*make_images(shape, seed)) >= MIN_COEF:
            return seed
    raise AssertionError(f"no seed in 0..15 keeps the difference coefficients of {shape} away from zero")


def unsafe_pixels(img1, img2, tol=MIN_COEF):
    """A bool mask in the images' shape: the pixels of every 4 x 4 block that holds a coefficient with |float64 difference| < tol (where
    float32 may give the coefficient the other sign)."""
    H, W = img1.shape[-2:]
    ll2, d1, d2 = diff_coefs64(img1, img2)
    h2, w2 = ll2.shape[-2:]
    small1 = (d1.abs() < tol).any(dim=-3)
    small1 = F.pad(small1, (0, 2 * w2 - small1.shape[-1], 0, 2 * h2 - small1.shape[-2]))
    bad = small1[..., 0::2, 0::2] | small1[..., 0::2, 1::2] | small1[..., 1::2, 0::2] | small1[..., 1::2, 1::2]
    bad = bad | (ll2.abs() < tol) | (d2.abs() < tol).any(dim=-3)
    return bad.repeat_interleave(4, dim=-2).repeat_interleave(4, dim=-1)[..., :H, :W]
