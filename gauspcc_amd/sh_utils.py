"""Spherical-harmonic colours on the device (gsr_sh_forward / gsr_sh_backward): the drop-in for each framework's utils/sh_utils.py

    from utils.sh_utils import eval_sh, RGB2SH, SH2RGB   ->   from gauspcc_amd.sh_utils import eval_sh, RGB2SH, SH2RGB

and the colour pass behind `GaussianRasterizer(...)(shs=...)`.

`eval_sh(deg, sh, dirs)` takes sh (..., C, M) with M >= (deg + 1)^2 and dirs (..., 3) and returns (..., C), deg 0..4; the directions are
used as given.  float32 CUDA tensors with C = 3 and equal leading shapes run the kernel (differentiable in sh and dirs, bitwise
reproducible); anything else -- CPU tensors, float64, another C, broadcast leading shapes -- is the torch expression over `sh_basis`.
`sh_colors(shs, means3D, campos, degree)` is the clamping form the rasteriser uses: shs (P, M, 3), direction (mean - campos) normalised,
max(value + 0.5, 0), differentiable in shs and means3D; float32 CUDA only (RuntimeError for CPU tensors: no CPU path).
`RGB2SH` / `SH2RGB` convert between a colour and its DC coefficient, on torch tensors, numpy arrays and numbers.

The basis is the real spherical harmonics up to degree 4 with the Condon-Shortley sign, polynomials in the direction's components; degree
4 is written for unit directions (r = 1), which is what frameworks evaluate.
"""
from math import pi, sqrt

import torch

from . import _lib, runtime
from .runtime import ptr

MAX_DEGREE = 4

C0 = 0.5 * sqrt(1 / pi)
C1 = sqrt(3 / (4 * pi))
C2 = (0.5 * sqrt(15 / pi), 0.25 * sqrt(5 / pi), 0.25 * sqrt(15 / pi))
C3 = (0.25 * sqrt(35 / (2 * pi)), 0.5 * sqrt(105 / pi), 0.25 * sqrt(21 / (2 * pi)), 0.25 * sqrt(7 / pi), 0.25 * sqrt(105 / pi))
C4 = (0.75 * sqrt(35 / pi), 0.75 * sqrt(35 / (2 * pi)), 0.75 * sqrt(5 / pi), 0.75 * sqrt(5 / (2 * pi)), (3 / 16) * sqrt(1 / pi),
      (3 / 8) * sqrt(5 / pi), (3 / 16) * sqrt(35 / pi))


def RGB2SH(rgb):
    return (rgb - 0.5) / C0


def SH2RGB(sh):
    return sh * C0 + 0.5


def _degree(deg):
    if isinstance(deg, bool) or int(deg) != deg or not 0 <= int(deg) <= MAX_DEGREE:
        raise ValueError(f"SH degree must be an integer in 0..{MAX_DEGREE}, got {deg!r}")
    return int(deg)


def sh_basis(deg, dirs):
    """The (deg + 1)^2 basis values at dirs (..., 3): (..., (deg + 1)^2), in dirs' dtype, differentiable."""
    deg = _degree(deg)
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    b = [torch.full_like(x, C0)]
    if deg >= 1:
        b += [-C1 * y, C1 * z, -C1 * x]
    if deg >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        xmy = xx - yy
        b += [C2[0] * xy, -C2[0] * yz, C2[1] * (2 * zz - xx - yy), -C2[0] * xz, C2[2] * xmy]
    if deg >= 3:
        p, q, r, s = 3 * xx - yy, 4 * zz - xx - yy, 2 * zz - 3 * xx - 3 * yy, xx - 3 * yy
        b += [-C3[0] * (y * p), C3[1] * (xy * z), -C3[2] * (y * q), C3[3] * (z * r), -C3[2] * (x * q), C3[4] * (z * xmy), -C3[0] * (x * s)]
    if deg >= 4:
        u, v = 7 * zz - 1, 7 * zz - 3
        b += [C4[0] * (xy * xmy), -C4[1] * (yz * p), C4[2] * (xy * u), -C4[3] * (yz * v), C4[4] * (zz * (35 * zz - 30) + 3), -C4[3] * (xz * v),
              C4[5] * (xmy * u), -C4[1] * (xz * s), C4[6] * (xx * s - yy * p)]
    return torch.stack(b, dim=-1)


def _eval_sh_torch(deg, sh, dirs):
    basis = sh_basis(deg, dirs)
    return (sh[..., : basis.shape[-1]] * basis.unsqueeze(-2)).sum(-1)


class _SHColors(torch.autograd.Function):
    """colours (P, 3) from coefficients: sh is (P, M, 3) (coef_dim 1) or (P, 3, M) (coef_dim 2), any strides; vec the means (campos given:
    the clamping form) or the directions (campos None)."""

    @staticmethod
    def forward(ctx, sh, vec, campos, degree, coef_dim):
        sh, vec = sh.detach(), vec.detach().contiguous()
        P, dev = vec.shape[0], vec.device
        colors = torch.empty((P, 3), dtype=torch.float32, device=dev)
        clamped = None if campos is None else torch.empty((P, 3), dtype=torch.uint8, device=dev)
        strides = (sh.stride(coef_dim), sh.stride(3 - coef_dim), sh.stride(0))
        means, dirs = (vec, None) if campos is not None else (None, vec)
        if P:
            _lib.check(_lib.lib().gsr_sh_forward(runtime.context(dev), P, degree, sh.data_ptr(), *strides, ptr(means), ptr(campos), ptr(dirs),
                                                 colors.data_ptr(), ptr(clamped), runtime.stream_ptr(dev)))
        ctx.degree, ctx.coef_dim, ctx.campos = degree, coef_dim, campos
        ctx.save_for_backward(sh, vec, clamped)
        return colors

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        sh, vec, clamped = ctx.saved_tensors
        P, dev, cd = vec.shape[0], vec.device, ctx.coef_dim
        need_sh, need_vec = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_sh = torch.empty(sh.shape, dtype=torch.float32, device=dev) if need_sh else None
        g_vec = torch.empty((P, 3), dtype=torch.float32, device=dev) if need_vec else None
        if P and (need_sh or need_vec):
            grad = grad.detach().to(torch.float32).contiguous()
            strides = (sh.stride(cd), sh.stride(3 - cd), sh.stride(0))
            g_strides = (0, 0, 0) if g_sh is None else (g_sh.stride(cd), g_sh.stride(3 - cd), g_sh.stride(0))
            means, dirs = (vec, None) if ctx.campos is not None else (None, vec)
            _lib.check(_lib.lib().gsr_sh_backward(
                runtime.context(dev), P, ctx.degree, sh.shape[cd], sh.data_ptr(), *strides, ptr(means), ptr(ctx.campos), ptr(dirs), ptr(clamped),
                grad.data_ptr(), ptr(g_sh), *g_strides, ptr(g_vec if means is not None else None), ptr(g_vec if dirs is not None else None),
                runtime.stream_ptr(dev)))
        return g_sh, g_vec, None, None, None


def _check_cuda(t, who, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {what} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {what} must be a CUDA tensor (got {t.device}); gauspcc_amd has no CPU path")


def check_shs(shs, P, degree, who):
    """The rasteriser's shape rules for shs: (P, M, 3) with M >= (degree + 1)^2, degree 0..4."""
    degree = _degree(degree)
    if shs.dim() != 3 or shs.shape[2] != 3:
        raise ValueError(f"{who}: shs must be (P, M, 3), got {tuple(shs.shape)}")
    if shs.shape[0] != P:
        raise ValueError(f"{who}: shs {tuple(shs.shape)} for {P} Gaussians")
    if shs.shape[1] < (degree + 1) ** 2:
        raise ValueError(f"{who}: shs holds {shs.shape[1]} coefficients, SH degree {degree} needs {(degree + 1) ** 2}")
    return degree


def sh_colors(shs, means3D, campos, degree):
    """max(sum_k basis_k(d) shs[:, k] + 0.5, 0) with d = (means3D - campos) / |means3D - campos|: (P, 3) float32, what the rasteriser
    computes for `shs=`.  A Gaussian exactly at campos gets its DC term and a zero means3D gradient.  campos: 3 values, read on the device."""
    who = "sh_colors"
    for t, what in ((shs, "shs"), (means3D, "means3D")):
        _check_cuda(t, who, what)
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError(f"{who}: means3D must be (P, 3), got {tuple(means3D.shape)}")
    degree = check_shs(shs, means3D.shape[0], degree, who)
    cam = torch.as_tensor(campos).detach().to(device=means3D.device, dtype=torch.float32).reshape(-1).contiguous()
    if cam.numel() != 3:
        raise ValueError(f"{who}: campos must hold 3 values, got {tuple(torch.as_tensor(campos).shape)}")
    return _SHColors.apply(shs.to(torch.float32), means3D.to(torch.float32), cam, degree, 1)


def eval_sh(deg, sh, dirs):
    """Spherical harmonics of degree `deg` at the directions `dirs`: sh (..., C, M), M >= (deg + 1)^2, dirs (..., 3) -> (..., C)."""
    deg = _degree(deg)
    if sh.shape[-1] < (deg + 1) ** 2:
        raise ValueError(f"eval_sh: sh holds {sh.shape[-1]} coefficients, degree {deg} needs {(deg + 1) ** 2}")
    kernel = (isinstance(sh, torch.Tensor) and isinstance(dirs, torch.Tensor) and sh.is_cuda and dirs.is_cuda and sh.dtype == torch.float32
              and dirs.dtype == torch.float32 and sh.dim() >= 2 and sh.shape[-2] == 3 and dirs.shape[-1] == 3 and sh.shape[:-2] == dirs.shape[:-1]
              and sh.device == dirs.device and sh.numel() > 0)
    if not kernel:
        return _eval_sh_torch(deg, sh, dirs)
    lead = sh.shape[:-2]
    out = _SHColors.apply(sh.reshape(-1, 3, sh.shape[-1]), dirs.reshape(-1, 3), None, deg, 2)
    return out.reshape(*lead, 3)
