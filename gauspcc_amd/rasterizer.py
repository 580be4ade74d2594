"""Mirror of `diff_gaussian_rasterization` as the reference uses it
(HAC/gaussian_renderer/__init__.py:20, 187-225, 268-303): GaussianRasterizationSettings,
GaussianRasterizer(...)(means3D, means2D, opacities, shs, colors_precomp, scales, rotations,
cov3D_precomp) -> (image (3,H,W), radii (P,) int32) and .visible_filter(...) -> radii.

Differentiable like the module it stands in for: with grad mode on and any of means3D, means2D, opacities,
colors_precomp, scales, rotations, cov3D_precomp requiring grad, the call goes through _RasterizeGaussians
(gsr_forward_train + gsr_backward: the same image, and gradients for those seven inputs; means2D's gradient is
dL/d(NDC x, y) of the projected centre, z column 0, what training_statis reads).  Otherwise -- RD evaluation,
torch.no_grad() -- the forward-only gsr_forward runs, as before.  No background gradient, no double backward.

Colours come as `colors_precomp` (P, 3) or as `shs` (P, M, 3) spherical-harmonic coefficients with M >= (sh_degree + 1)^2, sh_degree 0..4:
sh_utils.sh_colors turns those into colours from means3D and raster_settings.campos (gsr_sh_forward; gsr_sh_backward under autograd, which
then adds the colour pass's means3D gradient to the rasteriser's) and the frame goes on exactly as with colors_precomp.

`extras=("invdepth", "alpha")` (either, any order) asks for the frame's inverse-depth and accumulated-opacity maps next to the image, on both
paths (gsr_forward_aux; gsr_forward_train_aux + gsr_backward_aux); without it the call, its 2-tuple and its kernels are what they were.
"""
import ctypes as C
from typing import NamedTuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, runtime, sh_utils
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
    if ((scales is None or rotations is None) and cov3D_precomp is None) or ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')


EXTRAS = ("invdepth", "alpha")


def _check_extras(extras):
    """extras -> a tuple of distinct names from EXTRAS (None: none); anything else is a ValueError, raised before any device call."""
    if extras is None:
        return ()
    if not isinstance(extras, tuple):
        raise ValueError(f"extras must be a tuple of names from {EXTRAS}, got {extras!r}")
    for k, name in enumerate(extras):
        if name not in EXTRAS:
            raise ValueError(f"unknown extra {name!r}: choose from {EXTRAS}")
        if name in extras[:k]:
            raise ValueError(f"extra {name!r} asked for twice")
    return extras


class _Frame:
    """The frame arguments every entry point marshals: the float32 contiguous tensors (held here until the call has returned: their
    pointers cross the ABI) and the leading C arguments the gsr_* calls share."""

    def __init__(self, rs, means3D, colors=None, opacities=None, scales=None, rotations=None, cov3D_precomp=None):
        self.means, self.colors, self.opac = _f32(means3D), _f32(colors), _f32(opacities)
        self.scales, self.rots, self.cov = _f32(scales), _f32(rotations), _f32(cov3D_precomp)
        self.view, self.proj, self.bg = _f32(rs.viewmatrix), _f32(rs.projmatrix), _f32(rs.bg)
        self.P, self.dev = self.means.shape[0], self.means.device
        self.H, self.W = int(rs.image_height), int(rs.image_width)
        self.scale_modifier, self.prefiltered = float(rs.scale_modifier), int(bool(rs.prefiltered))
        self.camera = (self.view.data_ptr(), self.proj.data_ptr(), float(rs.tanfovx), float(rs.tanfovy))
        # P, background, W, H, means3D, colors, opacities, scales, scale_modifier, rotations, cov3D_precomp, view, proj, tan_fovx, tan_fovy
        self.args = (self.P, ptr(self.bg), self.W, self.H, self.means.data_ptr(), ptr(self.colors), ptr(self.opac), ptr(self.scales),
                     self.scale_modifier, ptr(self.rots), ptr(self.cov), *self.camera)

    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.dev)


class _RasterizeGaussians(torch.autograd.Function):
    """Training path.  The frame state the backward needs lives in uint8 tensors handed to the library through its allocator callback and
    kept on the autograd context: it dies with the graph, and other rasteriser calls may run between forward and backward."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, colors_precomp, scales, rotations, cov3D_precomp, raster_settings, info, extras=()):
        f = _Frame(raster_settings, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp)
        color, radii = f.empty(3, f.H, f.W), f.empty(f.P, dtype=torch.int32)
        work = runtime.Workspace(f.dev)
        state = (C.c_uint64 * _lib.GSR_STATE_WORDS)()
        n = C.c_int64()
        tail = (work.fn(), None, state, C.byref(n), runtime.stream_ptr(f.dev))
        maps = {name: f.empty(1, f.H, f.W) for name in extras}     # the kernel writes every pixel
        if extras:
            _lib.check(_lib.lib().gsr_forward_train_aux(runtime.context(f.dev), *f.args, f.prefiltered, color.data_ptr(), radii.data_ptr(),
                                                        ptr(maps.get("invdepth")), ptr(maps.get("alpha")), *tail))
        else:
            _lib.check(_lib.lib().gsr_forward_train(runtime.context(f.dev), *f.args, f.prefiltered, color.data_ptr(), radii.data_ptr(), *tail))
        info["num_rendered"] = n.value
        ctx.rs, ctx.extras = raster_settings, extras
        ctx.frame = (work, state)
        ctx.save_for_backward(means3D, means2D, opacities, colors_precomp, scales, rotations, cov3D_precomp, radii)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)     # a map (or the image) that the loss does not reach arrives as None, not as a tensor of zeros
        return (color, radii, *(maps[name] for name in extras))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_color, grad_radii, *grad_maps):
        means3D, means2D, opacities, colors_precomp, scales, rotations, cov3D_precomp, radii = ctx.saved_tensors
        f = _Frame(ctx.rs, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp)
        dout = f.empty(3, f.H, f.W).zero_() if grad_color is None else _f32(grad_color)
        dmap = {name: _f32(gm) for name, gm in zip(ctx.extras, grad_maps) if gm is not None}     # a missing gradient counts as zero
        g = {"m3": f.empty(f.P, 3), "m2": f.empty(f.P, 3), "col": f.empty(f.P, 3), "op": f.empty(f.P)}
        if f.cov is None:
            g["sc"], g["rot"] = f.empty(f.P, 3), f.empty(f.P, 4)
        else:
            g["cov"] = f.empty(f.P, 6)
        head = (runtime.context(f.dev), ctx.frame[1], *f.args, radii.data_ptr(), dout.data_ptr())
        tail = (runtime.Workspace(f.dev).fn(), None, g["m3"].data_ptr(), g["m2"].data_ptr(), g["col"].data_ptr(), g["op"].data_ptr(), ptr(g.get("sc")),
                ptr(g.get("rot")), ptr(g.get("cov")), runtime.stream_ptr(f.dev))
        if dmap:
            _lib.check(_lib.lib().gsr_backward_aux(*head, ptr(dmap.get("invdepth")), ptr(dmap.get("alpha")), *tail))
        else:
            _lib.check(_lib.lib().gsr_backward(*head, *tail))
        ctx.frame = None   # the frame state goes with its workspace

        def out(key, t):
            if t is None or not ctx.needs_input_grad[["m3", "m2", "op", "col", "sc", "rot", "cov"].index(key)]:
                return None
            return g[key].view(t.shape).to(t.dtype)

        return (out("m3", means3D), out("m2", means2D), out("op", opacities), out("col", colors_precomp), out("sc", scales),
                out("rot", rotations), out("cov", cov3D_precomp), None, None, None)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    @torch.no_grad()
    def visible_filter(self, means3D, scales=None, rotations=None, cov3D_precomp=None):
        f = _Frame(self.raster_settings, means3D, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
        radii = f.empty(f.P, dtype=torch.int32)       # k_preprocess writes every entry
        _lib.check(_lib.lib().gsr_visible_filter(runtime.context(f.dev), f.P, f.W, f.H, f.means.data_ptr(), ptr(f.scales), f.scale_modifier,
                                                 ptr(f.rots), ptr(f.cov), *f.camera, f.prefiltered, radii.data_ptr(), runtime.stream_ptr(f.dev)))
        return radii

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, extras=None):
        """-> (image, radii), or with extras, a tuple from EXTRAS, (image, radii, *maps) in the order asked, (1, H, W) float32 each and
        differentiable like the image: "invdepth" = sum_i w_i / tz_i over the Gaussians a pixel blends (the colour's weights; no background
        term, not normalised: the inverse-depth map of the public rasteriser), "alpha" = 1 - T_final, the accumulated opacity."""
        extras = _check_extras(extras)
        _check_args(shs, colors_precomp, scales, rotations, cov3D_precomp)
        if shs is not None:
            colors_precomp = sh_utils.sh_colors(shs, means3D, self.raster_settings.campos, self.raster_settings.sh_degree)
        diff = (means3D, means2D, opacities, colors_precomp, scales, rotations, cov3D_precomp)
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in diff):
            info = {}
            out = _RasterizeGaussians.apply(*diff, self.raster_settings, info, extras)
            self.num_rendered = info["num_rendered"]
            return tuple(out)
        return self._forward_inference(means3D, opacities, colors_precomp, scales, rotations, cov3D_precomp, extras)

    @torch.no_grad()
    def _forward_inference(self, means3D, opacities, colors_precomp, scales, rotations, cov3D_precomp, extras=()):
        f = _Frame(self.raster_settings, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp)
        color, radii = f.empty(3, f.H, f.W), f.empty(f.P, dtype=torch.int32)       # k_preprocess writes every entry
        n = C.c_int64()
        maps = {name: f.empty(1, f.H, f.W) for name in extras}
        if extras:
            _lib.check(_lib.lib().gsr_forward_aux(runtime.context(f.dev), *f.args, f.prefiltered, color.data_ptr(), radii.data_ptr(), ptr(maps.get("invdepth")),
                                                  ptr(maps.get("alpha")), C.byref(n), runtime.stream_ptr(f.dev)))
        else:
            _lib.check(_lib.lib().gsr_forward(runtime.context(f.dev), *f.args, f.prefiltered, color.data_ptr(), radii.data_ptr(), C.byref(n), runtime.stream_ptr(f.dev)))
        self.num_rendered = n.value
        return (color, radii, *(maps[name] for name in extras))


def psnr(img1, img2):
    """HAC/utils/image_utils.py:17-19 (per leading-dim PSNR)."""
    mse = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))
