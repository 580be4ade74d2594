"""The Haar DWT on the device (gsr_haar_forward / gsr_haar_inverse): a drop-in for the two modules TC-GS/utils/loss_utils.py takes from
pytorch_wavelets:

    from pytorch_wavelets import DWTForward, DWTInverse   ->   from gauspcc_amd.wavelets import DWTForward, DWTInverse

`DWTForward(J, wave, mode)(x)` takes (B, C, H, W) and returns `(Yl, Yh)`: Yl (B, C, h_J, w_J) and Yh a list of J tensors
(B, C, 3, h_j, w_j), finest first, h_j = ceil(h_{j-1} / 2); Yh[j][:, :, 0] is low along the width and high along the height.
`DWTInverse(wave, mode)((Yl, Yh))` returns (B, C, 2 h_1, 2 w_1): as in the package it does not crop to an odd original size (the caller
does), it drops Yl's last row or column where Yl has one more than a level's Yh, and a None in Yh stands for zeros.  Both are
differentiable: Haar is orthonormal, so each kernel is the other's backward.  One launch per level.

Served: wave 'haar' (= 'db1'), mode 'zero'; anything else raises NotImplementedError.  Inputs must be float32 CUDA tensors (TypeError for
another dtype, RuntimeError for CPU tensors: there is no CPU path).  The modules have no parameters or buffers, so `.to('cuda')` does
nothing.  The loss TC-GS builds from them is gauspcc_amd.loss_utils.wavelet_loss, one launch for both levels of both images.
"""
import torch
from torch import nn

from . import _lib, runtime
from .runtime import ptr

WAVES = ("haar", "db1")
MODES = ("zero",)


def _served(wave, mode, who):
    if wave not in WAVES:
        raise NotImplementedError(f"{who}: wave {wave!r} is not served (served: {', '.join(WAVES)})")
    if mode not in MODES:
        raise NotImplementedError(f"{who}: mode {mode!r} is not served (served: {', '.join(MODES)})")


def _check(t, who, what, dims=(4,)):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {what} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {what} must be float32, got {t.dtype}")
    if t.dim() not in dims:
        raise ValueError(f"{who}: {what} must have {' or '.join(str(d) for d in dims)} dimensions, got {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"{who}: empty {what} {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {what} must be a CUDA tensor (got {t.device}); gauspcc_amd has no CPU path")


def _level_forward(x):
    """gsr_haar_forward on a contiguous (B, C, H, W): (ll (B, C, h, w), high (B, C, 3, h, w))."""
    B, C, H, W = x.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    ll = torch.empty((B, C, h, w), dtype=torch.float32, device=x.device)
    high = torch.empty((B, C, 3, h, w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().gsr_haar_forward(runtime.context(x.device), x.data_ptr(), B * C, H, W, ll.data_ptr(), high.data_ptr(), runtime.stream_ptr(x.device)))
    return ll, high


def _level_inverse(ll, high, Ho, Wo):
    """gsr_haar_inverse on a contiguous ll (B, C, h, w) and high (B, C, 3, h, w) or None: (B, C, Ho, Wo)."""
    B, C, h, w = ll.shape
    out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=ll.device)
    _lib.check(_lib.lib().gsr_haar_inverse(runtime.context(ll.device), ll.data_ptr(), ptr(high), B * C, h, w, out.data_ptr(), Ho, Wo, runtime.stream_ptr(ll.device)))
    return out


def _grad(g, shape, like):
    return torch.zeros(shape, dtype=torch.float32, device=like.device) if g is None else g.detach().to(torch.float32).contiguous()


class _Analysis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.size = x.shape[-2:]
        return _level_forward(x.detach().contiguous())

    @staticmethod
    def backward(ctx, g_ll, g_high):
        if g_ll is None and g_high is None:
            return None
        ref = g_ll if g_ll is not None else g_high
        B, C = ref.shape[:2]
        h, w = ref.shape[-2:]
        return _level_inverse(_grad(g_ll, (B, C, h, w), ref), None if g_high is None else _grad(g_high, None, ref), *ctx.size)


class _Synthesis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ll, high, Ho, Wo):
        ctx.with_high = high is not None
        return _level_inverse(ll.detach().contiguous(), None if high is None else high.detach().contiguous(), Ho, Wo)

    @staticmethod
    def backward(ctx, g):
        g_ll, g_high = _level_forward(_grad(g, None, g))
        return g_ll, (g_high if ctx.with_high and ctx.needs_input_grad[1] else None), None, None


class DWTForward(nn.Module):
    """pytorch_wavelets.DWTForward for the Haar wavelet and zero padding: J levels, one launch each."""

    def __init__(self, J=1, wave="db1", mode="zero"):
        super().__init__()
        _served(wave, mode, "DWTForward")
        if isinstance(J, bool) or not isinstance(J, int) or J < 1:
            raise ValueError(f"DWTForward: J must be an int >= 1, got {J!r}")
        self.J, self.wave, self.mode = J, wave, mode

    def forward(self, x):
        _check(x, "DWTForward", "x")
        yh = []
        ll = x
        for _ in range(self.J):
            ll, high = _Analysis.apply(ll)
            yh.append(high)
        return ll, yh


class DWTInverse(nn.Module):
    """pytorch_wavelets.DWTInverse for the Haar wavelet and zero padding: one launch per level, coarsest first."""

    def __init__(self, wave="db1", mode="zero"):
        super().__init__()
        _served(wave, mode, "DWTInverse")
        self.wave, self.mode = wave, mode

    def forward(self, coeffs):
        yl, yh = coeffs
        _check(yl, "DWTInverse", "Yl")
        ll = yl
        for high in yh[::-1]:
            if high is not None:
                _check(high, "DWTInverse", "a Yh entry", dims=(5,))
                if high.shape[:2] != ll.shape[:2] or high.shape[2] != 3:
                    raise ValueError(f"DWTInverse: Yh entry {tuple(high.shape)} does not belong to a low band {tuple(ll.shape)}")
                if high.device != ll.device:
                    raise ValueError(f"DWTInverse: coefficients on {ll.device} and {high.device}")
                # the level below was odd: its padded row / column is not part of this level's low band
                if ll.shape[-2] > high.shape[-2]:
                    ll = ll[..., :-1, :]
                if ll.shape[-1] > high.shape[-1]:
                    ll = ll[..., :-1]
                if ll.shape[-2:] != high.shape[-2:]:
                    raise ValueError(f"DWTInverse: low band {tuple(ll.shape)} and Yh entry {tuple(high.shape)} differ in size")
            ll = _Synthesis.apply(ll, high, 2 * ll.shape[-2], 2 * ll.shape[-1])
        return ll
