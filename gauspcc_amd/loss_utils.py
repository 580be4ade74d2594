"""The photometric loss of the 3DGS training step on the device (gsr_ssim_forward / gsr_ssim_backward): a drop-in for utils/loss_utils.py,
the same file in HAC, HAC++, TC-GS and CAT-3DGS:

    from utils.loss_utils import l1_loss, ssim   ->   from gauspcc_amd.loss_utils import l1_loss, ssim

`ssim` keeps the reference's signature and values (Gaussian window, sigma 1.5, zero padding, sigma^2 = E - mu^2 in float32) and is
differentiable in whichever of its two images requires grad.  `photometric_loss` is train.py's `(1 - lambda_dssim) * Ll1 + lambda_dssim *
(1 - ssim)` in the same two launches forward and one backward.  Results are bitwise reproducible: no float atomics.

TC-GS's loss_utils.py also has `wavelet_loss` (built on pytorch_wavelets' DWTForward); its swap is

    from utils.loss_utils import l1_loss, ssim, wavelet_loss   ->   from gauspcc_amd.loss_utils import l1_loss, ssim, wavelet_loss

and `tcgs_photometric_loss` is that train.py's loss with the wavelet term (gsr_wavelet_l1_forward / gsr_wavelet_l1_backward).

Differences from the reference: `window_size` must be odd and at most 31 (an even window gives the reference an (H+1) x (W+1) map; ValueError
here), inputs must be float32 CUDA tensors of the same shape (TypeError for another dtype, RuntimeError for CPU tensors: there is no CPU path).
"""
import ctypes
import functools
import math

import torch

from . import _lib, runtime
from .runtime import ptr

MAX_WINDOW = 31


@functools.lru_cache(maxsize=None)
def _taps(window_size):
    """loss_utils.gaussian(window_size, 1.5) as a host float array: float32 taps divided by their float32 sum, built by torch as the
    reference builds them (the kernels take them as arguments; their sum's last bit shows in flat bright regions)."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)], dtype=torch.float32)
    return (ctypes.c_float * window_size)(*(g / g.sum()).tolist())


def l1_loss(network_output, gt):
    return torch.abs((network_output - gt)).mean()


def l2_loss(network_output, gt):
    return ((network_output - gt) ** 2).mean()


def _check(img1, img2, window_size, who):
    for t in (img1, img2):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: images must be torch.Tensors, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: images must be float32, got {t.dtype}")
    if isinstance(window_size, bool) or not isinstance(window_size, int):
        raise TypeError(f"{who}: window_size must be an int, got {type(window_size).__name__}")
    if window_size < 1 or window_size > MAX_WINDOW or window_size % 2 == 0:
        raise ValueError(f"{who}: window_size {window_size} is not odd in [1, {MAX_WINDOW}]")
    if img1.dim() not in (3, 4):
        raise ValueError(f"{who}: images must be (C, H, W) or (B, C, H, W), got {tuple(img1.shape)}")
    if img1.shape != img2.shape:
        raise ValueError(f"{who}: image shapes differ: {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.numel() == 0:
        raise ValueError(f"{who}: empty images {tuple(img1.shape)}")
    if not img1.is_cuda or not img2.is_cuda:
        raise RuntimeError(f"{who}: images must be CUDA tensors (got {img1.device}, {img2.device}); gauspcc_amd has no CPU path")
    if img1.device != img2.device:
        raise ValueError(f"{who}: images on {img1.device} and {img2.device}")


def _bchw(t):
    t = t.detach().contiguous()
    return t if t.dim() == 4 else t.unsqueeze(0)


def _forward(x, y, window_size, size_average, nmaps, lam=None):
    """gsr_ssim_forward on contiguous (B, C, H, W) images: (ssim (1,) or (B,), l1 (1,) or None, loss (1,) or None, maps or None)."""
    B, C, H, W = x.shape
    dev = x.device
    out = torch.empty(1 if size_average else B, dtype=torch.float32, device=dev)
    l1 = torch.empty(1, dtype=torch.float32, device=dev) if lam is not None else None
    loss = torch.empty(1, dtype=torch.float32, device=dev) if lam is not None else None
    maps = torch.empty((nmaps,) + tuple(x.shape), dtype=torch.float32, device=dev) if nmaps else None
    _lib.check(_lib.lib().gsr_ssim_forward(runtime.context(dev), x.data_ptr(), y.data_ptr(), B, C, H, W, window_size, _taps(window_size),
                                           int(size_average), out.data_ptr(), ptr(l1), ptr(loss), 0.0 if lam is None else float(lam), ptr(maps), nmaps,
                                           runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
    return out, l1, loss, maps


def _backward(x, y, window_size, size_average, maps, g_ssim, ssim_scale, g_l1, l1_scale, need1, need2):
    B, C, H, W = x.shape
    dev = x.device
    d1 = torch.empty_like(x) if need1 else None
    d2 = torch.empty_like(x) if need2 else None
    _lib.check(_lib.lib().gsr_ssim_backward(runtime.context(dev), x.data_ptr(), y.data_ptr(), B, C, H, W, window_size, _taps(window_size),
                                            int(size_average), maps.data_ptr(), maps.shape[0], g_ssim.data_ptr(), float(ssim_scale), ptr(g_l1), float(l1_scale),
                                            ptr(d1), ptr(d2), runtime.stream_ptr(dev)))
    return d1, d2


def _grad_value(g, n, dev):
    """An upstream gradient as n contiguous float32 device values (zeros when autograd passes None)."""
    if g is None:
        return torch.zeros(n, dtype=torch.float32, device=dev)
    return g.detach().to(torch.float32).reshape(-1).expand(n).contiguous()


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, window_size, size_average):
        x, y = _bchw(img1), _bchw(img2)
        nmaps = 4 if ctx.needs_input_grad[1] else 3
        out, _, _, maps = _forward(x, y, window_size, size_average, nmaps)
        ctx.save_for_backward(x, y, maps)
        ctx.window_size, ctx.size_average, ctx.shape = window_size, size_average, img1.shape
        return out[0] if size_average else out

    @staticmethod
    def backward(ctx, grad):
        x, y, maps = ctx.saved_tensors
        g = _grad_value(grad, 1 if ctx.size_average else x.shape[0], x.device)
        d1, d2 = _backward(x, y, ctx.window_size, ctx.size_average, maps, g, 1.0, None, 0.0, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        view = lambda d: None if d is None else d.view(ctx.shape)   # noqa: E731
        return view(d1), view(d2), None, None


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lambda_dssim):
        x, y = _bchw(image), _bchw(gt)
        nmaps = 4 if ctx.needs_input_grad[1] else 3
        s, l1, loss, maps = _forward(x, y, 11, True, nmaps, lam=lambda_dssim)
        ctx.save_for_backward(x, y, maps)
        ctx.lam, ctx.shape = float(lambda_dssim), image.shape
        l1, s = l1[0], s[0]
        ctx.mark_non_differentiable(l1, s)
        return loss[0], l1, s

    @staticmethod
    def backward(ctx, grad, _g_l1, _g_ssim):
        x, y, maps = ctx.saved_tensors
        g = _grad_value(grad, 1, x.device)
        d1, d2 = _backward(x, y, 11, True, maps, g, -ctx.lam, g, 1.0 - ctx.lam, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        view = lambda d: None if d is None else d.view(ctx.shape)   # noqa: E731
        return view(d1), view(d2), None


def ssim(img1, img2, window_size=11, size_average=True):
    """loss_utils.ssim: the mean SSIM of (C, H, W) or (B, C, H, W) images as a 0-d tensor, or with size_average=False the (B,) per-item
    means ((C, H, W) images then raise IndexError, as the reference's third .mean(1) does).  Differentiable in img1 and img2."""
    _check(img1, img2, window_size, "ssim")
    if not size_average and img1.dim() == 3:
        raise IndexError("ssim: size_average=False needs (B, C, H, W) images (the reference's ssim_map.mean(1).mean(1).mean(1) fails on (C, H, W))")
    if torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad):
        return _SSIM.apply(img1, img2, window_size, bool(size_average))
    out = _forward(_bchw(img1), _bchw(img2), window_size, size_average, 0)[0]
    return out[0] if size_average else out


def photometric_loss(image, gt, lambda_dssim=0.2):
    """train.py's loss: (loss, l1, ssim_value) with loss = (1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt)),
    differentiable in image (and in gt if it requires grad); l1 and ssim_value are detached 0-d tensors (for training_report)."""
    _check(image, gt, 11, "photometric_loss")
    if torch.is_grad_enabled() and (image.requires_grad or gt.requires_grad):
        return _Photometric.apply(image, gt, float(lambda_dssim))
    s, l1, loss, _ = _forward(_bchw(image), _bchw(gt), 11, True, 0, lam=float(lambda_dssim))
    return loss[0], l1[0], s[0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# TC-GS's wavelet term (TC-GS/utils/loss_utils.py:66-83): the weighted L1 of the bands of a two-level Haar DWT (zero mode), one launch
# over 4 x 4 pixel blocks forward and one backward (gsr_wavelet_l1_forward / gsr_wavelet_l1_backward, csrc/wavelet.hip)

def wavelet_weights(step=0):
    """The seven band weights of wavelet_loss at `step`, in the order LL2, level-1 bands 0..2, level-2 bands 0..2 (host floats, formed
    as the reference forms them)."""
    lmbda1, lmbda2 = 1.0 - step / 30000, step / 30000
    if step > 25000:
        return [0.0, 0.4 * lmbda1, 0.3 * lmbda1, 0.3 * lmbda1, 0.4 * lmbda2, 0.3 * lmbda2, 0.3 * lmbda2]
    return [lmbda1] + [0.2 * lmbda2] * 6


def _wavelet_forward(x, y, weights):
    """gsr_wavelet_l1_forward on contiguous (C, H, W) images: (loss (1,), the seven band means (7,))."""
    C, H, W = x.shape
    dev = x.device
    out = torch.empty(1, dtype=torch.float32, device=dev)
    bands = torch.empty(7, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().gsr_wavelet_l1_forward(runtime.context(dev), x.data_ptr(), y.data_ptr(), C, H, W, (ctypes.c_double * 7)(*weights),
                                                 out.data_ptr(), bands.data_ptr(), runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
    return out, bands


class _Wavelet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, weights):
        x, y = img1.detach().contiguous(), img2.detach().contiguous()
        ctx.save_for_backward(x, y)
        ctx.weights = weights
        return _wavelet_forward(x, y, weights)[0][0]

    @staticmethod
    def backward(ctx, grad):
        x, y = ctx.saved_tensors
        C, H, W = x.shape
        dev = x.device
        g = _grad_value(grad, 1, dev)
        d1 = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        d2 = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().gsr_wavelet_l1_backward(runtime.context(dev), x.data_ptr(), y.data_ptr(), C, H, W, (ctypes.c_double * 7)(*ctx.weights),
                                                      g.data_ptr(), ptr(d1), ptr(d2), runtime.stream_ptr(dev)))
        return d1, d2, None


def wavelet_loss(img1, img2, step=0):
    """TC-GS's loss_utils.wavelet_loss: (C, H, W) float32 CUDA images to a 0-d tensor, differentiable in img1 and img2.  The reference
    takes DWTForward(J=2, mode='zero', wave='haar') from pytorch_wavelets; here both levels of both images and the seven L1 means are one
    launch.  With step <= 25000 the loss is (1 - step/30000) L1(LL2) + 0.2 step/30000 (sum of the six detail bands' L1), beyond that
    0.4 / 0.3 / 0.3 of the level-1 bands times (1 - step/30000) plus the same of the level-2 bands times step/30000."""
    _check(img1, img2, 11, "wavelet_loss")
    if img1.dim() != 3:
        raise ValueError(f"wavelet_loss: images must be (C, H, W), got {tuple(img1.shape)}")
    weights = wavelet_weights(step)
    if torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad):
        return _Wavelet.apply(img1, img2, weights)
    return _wavelet_forward(img1.detach().contiguous(), img2.detach().contiguous(), weights)[0][0]


def tcgs_photometric_loss(image, gt, lambda_dssim=0.2, wavelet=0.02, step=0):
    """TC-GS's train.py:180-183 without scaling_reg: (loss, l1, ssim_value, wavelet_value) with loss = photometric_loss(image, gt,
    lambda_dssim)[0] + wavelet * wavelet_loss(image, gt, step); l1, ssim_value and wavelet_value are detached 0-d tensors."""
    loss, l1, s = photometric_loss(image, gt, lambda_dssim)
    w = wavelet_loss(image, gt, step)
    return loss + wavelet * w, l1, s, w.detach()
