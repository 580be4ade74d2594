"""Mirror of `diff_gaussian_rasterization` as the reference uses it
(HAC/gaussian_renderer/__init__.py:20, 187-225, 268-303): GaussianRasterizationSettings,
GaussianRasterizer(...)(means3D, means2D, opacities, shs, colors_precomp, scales, rotations,
cov3D_precomp) -> (image (3,H,W), radii (P,) int32) and .visible_filter(...) -> radii.

Differentiable like the module it stands in for: with grad mode on and any of means3D, means2D, opacities,
colors_precomp, scales, rotations, cov3D_precomp requiring grad, the call goes through _RasterizeGaussians
(gsr_forward_train + gsr_backward: the same image, and gradients for those seven inputs; means2D's gradient is
dL/d(NDC x, y) of the projected centre, z column 0, what training_statis reads).  Otherwise -- RD evaluation,
torch.no_grad() -- the forward-only gsr_forward runs, as before.  No background gradient, no double backward;
colours must be precomputed (`shs=None` at every call site of the reference).
"""
import ctypes as C
from typing import NamedTuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, runtime
from .runtime import ptr


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _f32(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


def _check_args(shs, colors_precomp, scales, rotations, cov3D_precomp):
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    if shs is not None:
        raise NotImplementedError("gauspcc_amd.rasterizer: SH evaluation is not on the reference's path (shs=None everywhere); pass colors_precomp")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')


class _RasterizeGaussians(torch.autograd.Function):
    """Training path.  The frame state the backward needs lives in uint8 tensors handed to the library through its allocator callback and
    kept on the autograd context: it dies with the graph, and other rasteriser calls may run between forward and backward."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, colors_precomp, scales, rotations, cov3D_precomp, raster_settings, info):
        rs = raster_settings
        m, col, op = _f32(means3D), _f32(colors_precomp), _f32(opacities)
        sc, rot, cov = _f32(scales), _f32(rotations), _f32(cov3D_precomp)
        P = m.shape[0]
        dev = m.device
        H, W = int(rs.image_height), int(rs.image_width)
        color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        view, proj, bg = _f32(rs.viewmatrix), _f32(rs.projmatrix), _f32(rs.bg)
        work = runtime.Workspace(dev)
        state = (C.c_uint64 * _lib.GSR_STATE_WORDS)()
        n = C.c_int64()
        _lib.check(_lib.lib().gsr_forward_train(
            runtime.context(dev), P, bg.data_ptr(), W, H, m.data_ptr(), col.data_ptr(), op.data_ptr(), ptr(sc), float(rs.scale_modifier), ptr(rot),
            ptr(cov), view.data_ptr(), proj.data_ptr(), float(rs.tanfovx), float(rs.tanfovy), int(bool(rs.prefiltered)), color.data_ptr(), radii.data_ptr(),
            work.fn(), None, state, C.byref(n), runtime.stream_ptr(dev)))
        info["num_rendered"] = n.value
        ctx.rs = rs
        ctx.frame = (work, state)
        ctx.save_for_backward(means3D, means2D, opacities, colors_precomp, scales, rotations, cov3D_precomp, radii)
        ctx.mark_non_differentiable(radii)
        return color, radii

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_color, grad_radii):
        means3D, means2D, opacities, colors_precomp, scales, rotations, cov3D_precomp, radii = ctx.saved_tensors
        rs = ctx.rs
        state = ctx.frame[1]
        m, col, op = _f32(means3D), _f32(colors_precomp), _f32(opacities)
        sc, rot, cov = _f32(scales), _f32(rotations), _f32(cov3D_precomp)
        P = m.shape[0]
        dev = m.device
        H, W = int(rs.image_height), int(rs.image_width)
        view, proj, bg = _f32(rs.viewmatrix), _f32(rs.projmatrix), _f32(rs.bg)
        dout = _f32(grad_color)
        g = {k: torch.empty(shape, dtype=torch.float32, device=dev)
             for k, shape in (("m3", (P, 3)), ("m2", (P, 3)), ("col", (P, 3)), ("op", (P,)))}
        if cov is None:
            g["sc"], g["rot"] = torch.empty((P, 3), dtype=torch.float32, device=dev), torch.empty((P, 4), dtype=torch.float32, device=dev)
        else:
            g["cov"] = torch.empty((P, 6), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gsr_backward(
            runtime.context(dev), state, P, bg.data_ptr(), W, H, m.data_ptr(), col.data_ptr(), op.data_ptr(), ptr(sc), float(rs.scale_modifier), ptr(rot),
            ptr(cov), view.data_ptr(), proj.data_ptr(), float(rs.tanfovx), float(rs.tanfovy), radii.data_ptr(), dout.data_ptr(),
            runtime.Workspace(dev).fn(), None, g["m3"].data_ptr(), g["m2"].data_ptr(), g["col"].data_ptr(), g["op"].data_ptr(), ptr(g.get("sc")),
            ptr(g.get("rot")), ptr(g.get("cov")), runtime.stream_ptr(dev)))
        ctx.frame = None   # the frame state goes with its workspace

        def out(key, t):
            if t is None or not ctx.needs_input_grad[["m3", "m2", "op", "col", "sc", "rot", "cov"].index(key)]:
                return None
            return g[key].view(t.shape).to(t.dtype)

        return (out("m3", means3D), out("m2", means2D), out("op", opacities), out("col", colors_precomp), out("sc", scales),
                out("rot", rotations), out("cov", cov3D_precomp), None, None)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    @torch.no_grad()
    def visible_filter(self, means3D, scales=None, rotations=None, cov3D_precomp=None):
        rs = self.raster_settings
        means3D, scales, rotations, cov3D_precomp = _f32(means3D), _f32(scales), _f32(rotations), _f32(cov3D_precomp)
        P = means3D.shape[0]
        radii = torch.empty(P, dtype=torch.int32, device=means3D.device)       # k_preprocess writes every entry
        view, proj = _f32(rs.viewmatrix), _f32(rs.projmatrix)
        _lib.check(_lib.lib().gsr_visible_filter(
            runtime.context(means3D.device), P, int(rs.image_width), int(rs.image_height), means3D.data_ptr(),
            None if scales is None else scales.data_ptr(), float(rs.scale_modifier), None if rotations is None else rotations.data_ptr(),
            None if cov3D_precomp is None else cov3D_precomp.data_ptr(), view.data_ptr(), proj.data_ptr(), float(rs.tanfovx), float(rs.tanfovy),
            int(bool(rs.prefiltered)), radii.data_ptr(), runtime.stream_ptr(means3D.device)))
        return radii

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        _check_args(shs, colors_precomp, scales, rotations, cov3D_precomp)
        diff = (means3D, means2D, opacities, colors_precomp, scales, rotations, cov3D_precomp)
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in diff):
            info = {}
            color, radii = _RasterizeGaussians.apply(*diff, self.raster_settings, info)
            self.num_rendered = info["num_rendered"]
            return color, radii
        return self._forward_inference(means3D, opacities, colors_precomp, scales, rotations, cov3D_precomp)

    @torch.no_grad()
    def _forward_inference(self, means3D, opacities, colors_precomp, scales, rotations, cov3D_precomp):
        rs = self.raster_settings
        means3D, colors, opac = _f32(means3D), _f32(colors_precomp), _f32(opacities)
        scales, rotations, cov3D_precomp = _f32(scales), _f32(rotations), _f32(cov3D_precomp)
        P = means3D.shape[0]
        dev = means3D.device
        H, W = int(rs.image_height), int(rs.image_width)
        color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty(P, dtype=torch.int32, device=dev)       # k_preprocess writes every entry
        view, proj, bg = _f32(rs.viewmatrix), _f32(rs.projmatrix), _f32(rs.bg)
        n = C.c_int64()
        _lib.check(_lib.lib().gsr_forward(
            runtime.context(dev), P, bg.data_ptr(), W, H, means3D.data_ptr(), colors.data_ptr(), opac.data_ptr(),
            None if scales is None else scales.data_ptr(), float(rs.scale_modifier), None if rotations is None else rotations.data_ptr(),
            None if cov3D_precomp is None else cov3D_precomp.data_ptr(), view.data_ptr(), proj.data_ptr(), float(rs.tanfovx), float(rs.tanfovy),
            int(bool(rs.prefiltered)), color.data_ptr(), radii.data_ptr(), C.byref(n), runtime.stream_ptr(dev)))
        self.num_rendered = n.value
        return color, radii


def psnr(img1, img2):
    """HAC/utils/image_utils.py:17-19 (per leading-dim PSNR)."""
    mse = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))
