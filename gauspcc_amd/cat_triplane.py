"""CAT-3DGS's multi-scale tri-plane features on the device (gsge_msplane_forward / gsge_msplane_backward): a drop-in for
scene/triplane.py,

    from scene.triplane import TriPlaneField   ->   from gauspcc_amd.cat_triplane import TriPlaneField      (CAT-3DGS/scene/attribute.py:13)

`ms_triplane_sample` is the native form: the PCA / contraction / aabb transform, the six border-padded bilinear reads, the /16 quantiser
and the level sums of one call in one kernel, (N, n_levels * 3 * C) out.  `interpolate_ms_features` keeps the reference's signature and
takes already normalised points.  `TriPlaneField` is a plain nn.Module with the reference's parameter names, shapes and initialisation
(`aabb`, `rotation_matrix`, `pca_mean`, `variance`, `con_aabb`, `log_2_encoder_gains`, `grids.<level>.<plane>`, `arm{,2,3}.mlp.<i>.{w,b}`),
so state dicts load either way; its rate term is gauspcc_amd.arm.arm_rate and gauspcc_amd.arm_codec's encode_triplane / decode_triplane
accept it.  The call is differentiable in the planes and, on the normalize_aabb path, in the points; the backward uses no float atomics,
so plane gradients are bitwise reproducible from run to run and across streams (the reference's grid_sample backward is not).

Differences from the reference: only grid_dimensions=2 with concat_features=True (ValueError otherwise); one channel count for all planes;
1 to 8 levels; float32 CUDA tensors only (TypeError for another dtype, RuntimeError for CPU tensors: there is no CPU path); a point
whose normalised coordinate is not finite yields a zero row and no gradient, where the reference yields NaN (a point that the PCA step
maps exactly to the origin: 1 / mag = inf in contract_to_unisphere's blend); with contract the points get no gradient (the reference
detaches them); the transform's parameters get none (the reference detaches rotation and variance; pca_mean, aabb and con_aabb are
never in CAT-3DGS's optimiser).  `grid_encode_forward` is not provided: its only caller is the reference's encode_triplane, which
gauspcc_amd.arm_codec.encode_triplane replaces; `contract_to_unisphere` takes (x, aabb) only (the reference's `derivative` branch has
no caller).  `set_aabb` prints nothing.
"""
import ctypes
import os

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, runtime
from .arm import ArmMLP, arm_rate
from .runtime import ptr, ptrs

MAX_CHANNELS, MAX_SIZE, MAX_LEVELS = 256, 4096, 8   # gsge_msplane_forward's limits
QUANT = 16.0                                        # the reference's quant_step, 2 ** 4


def _f32(t, name, who):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
    return t


def _same_cuda(named, who):
    """after the dtype and shape checks, so that a malformed call is reported as such wherever its tensors live"""
    first = named[0][1]
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a CUDA tensor (got {t.device}); gauspcc_amd has no CPU path")
        if t.device != first.device:
            raise ValueError(f"{who}: {name} on {t.device}, {named[0][0]} on {first.device}")


NORMALIZE, CONTRACT, CON_NORMALIZE, NONE = 0, 1, 2, 3   # gsge_msplane_forward's `contract` argument
_XFORM = (("pca_mean", 3), ("rotation", 9), ("variance", 3), ("aabb", 6), ("con_aabb", 6))
_READS = {NORMALIZE: ("aabb",), CONTRACT: tuple(k for k, _ in _XFORM), CON_NORMALIZE: ("aabb", "con_aabb"), NONE: ()}


class _Plan:
    """What one call reads besides the tensors: the planes' shapes and the flags."""
    def __init__(self, shapes, level, quantise, mode):
        self.shapes, self.level, self.quantise, self.mode = shapes, int(level), bool(quantise), mode
        self.L, self.C = len(shapes) // 3, shapes[0][0]

    def args(self, planes, xform):
        ints = lambda vs: (ctypes.c_int * len(vs))(*vs)   # noqa: E731
        return (self.L, ptrs(planes), self.C, ints([s[1] for s in self.shapes]), ints([s[2] for s in self.shapes]), self.level,
                int(self.quantise), self.mode, *[ptr(t) for t in xform])


def _check(pts, grids, level, who):
    _f32(pts, "pts", who)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"{who}: pts must be (N, 3), got {tuple(pts.shape)}")
    levels = [list(g) for g in grids]
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"{who}: {len(levels)} levels outside [1, {MAX_LEVELS}]")
    if isinstance(level, bool) or not isinstance(level, int):
        raise ValueError(f"{who}: level must be an int, got {level!r}")
    planes, shapes, named = [], [], [("pts", pts)]
    for l, g in enumerate(levels):
        if len(g) != 3:
            raise ValueError(f"{who}: level {l} has {len(g)} planes; 3 expected (grid_dimensions=2 of 3 coordinates)")
        for p, t in enumerate(g):
            name = f"plane {p} of level {l}"
            _f32(t, name, who)
            named.append((name, t))
            if t.dim() == 4 and t.shape[0] == 1:
                shape = tuple(t.shape[1:])
            elif t.dim() == 3:
                shape = tuple(t.shape)
            else:
                raise ValueError(f"{who}: {name} of shape {tuple(t.shape)}; [1, C, H, W] expected")
            C, H, W = shape
            if not 1 <= C <= MAX_CHANNELS:
                raise ValueError(f"{who}: {name}: {C} channels outside [1, {MAX_CHANNELS}]")
            if shapes and C != shapes[0][0]:
                raise ValueError(f"{who}: {name} has {C} channels, plane 0 of level 0 has {shapes[0][0]}")
            if not (2 <= H <= MAX_SIZE and 2 <= W <= MAX_SIZE):
                raise ValueError(f"{who}: {name} of {H} x {W} outside [2, {MAX_SIZE}]")
            planes.append(t)
            shapes.append(shape)
    if pts.shape[0] * 3 * len(levels) * 4 >= 1 << 32:
        raise ValueError(f"{who}: {pts.shape[0]} points x {len(levels)} levels: more than 2^32 (point, level, plane, corner) slots")
    return planes, shapes, named


def _transform(contract, aabb, named, who):
    """(mode, (pca_mean, rotation, variance, aabb, con_aabb)): contiguous detached tensors, None where the mode does not read one."""
    if contract is None:
        mode, given = (NONE, {}) if aabb is None else (NORMALIZE, {"aabb": aabb})
    else:
        if aabb is not None:
            raise ValueError(f"{who}: with contract the aabb is part of it")
        given = dict(contract) if isinstance(contract, dict) else dict(zip([k for k, _ in _XFORM], contract))
        if sorted(given) == sorted(_READS[CONTRACT]):
            mode = CONTRACT
        elif sorted(given) == sorted(_READS[CON_NORMALIZE]):
            mode = CON_NORMALIZE
        else:
            raise ValueError(f"{who}: contract must hold pca_mean, rotation, variance, aabb, con_aabb (or aabb, con_aabb alone)")
    out = []
    for name, size in _XFORM:
        t = given.get(name) if name in _READS[mode] else None
        if t is not None:
            _f32(t, name, who)
            if t.numel() != size:
                raise ValueError(f"{who}: {name} must hold {size} values, got {tuple(t.shape)}")
            named.append((name, t))
            t = t.detach().reshape(size).contiguous()
        out.append(t)
    return mode, tuple(out)


def _forward(plan, pts, planes, xform):
    dev = pts.device
    N = pts.shape[0]
    out = torch.empty((N, plan.L * 3 * plan.C), dtype=torch.float32, device=dev)
    if N:
        _lib.check(_lib.lib().gsge_msplane_forward(runtime.context(dev), pts.data_ptr(), N, *plan.args(planes, xform), out.data_ptr(),
                                                   runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
    return out


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, pts, xform, *planes):
        p = pts.detach().contiguous()
        ps = [t.detach().reshape(s).contiguous() for t, s in zip(planes, plan.shapes)]
        out = _forward(plan, p, ps, xform)
        ctx.plan, ctx.plane_shapes = plan, [t.shape for t in planes]
        ctx.n_xform = [t is not None for t in xform]
        ctx.save_for_backward(p, *[t for t in xform if t is not None], *ps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        plan = ctx.plan
        p, *rest = ctx.saved_tensors
        it = iter(rest)
        xform = tuple(next(it) if has else None for has in ctx.n_xform)
        ps = list(it)
        dev, N = p.device, p.shape[0]
        gps = [torch.empty_like(t) for t in ps]
        gpts = torch.empty_like(p) if ctx.needs_input_grad[1] else None
        g = grad.to(torch.float32).contiguous()
        if N == 0:
            for t in gps:
                t.zero_()
        else:
            _lib.check(_lib.lib().gsge_msplane_backward(runtime.context(dev), g.data_ptr(), p.data_ptr(), N, *plan.args(ps, xform), ptrs(gps), ptr(gpts),
                                                        runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
        need = ctx.needs_input_grad[3:]
        return (None, gpts, None, *[t.view(s) if n else None for t, s, n in zip(gps, ctx.plane_shapes, need)])


class _RoundSTE(torch.autograd.Function):
    """torch.round with the gradient passed unchanged: the reference's quantisers at evaluation time"""
    @staticmethod
    def forward(ctx, x):
        return torch.round(x)

    @staticmethod
    def backward(ctx, grad):
        return grad


def ms_triplane_sample(pts, grids, level=2, quantise=False, contract=None, aabb=None):
    """The (N, n_levels * 3 * C) multi-scale features of pts (N, 3): out[n, l * 3 C + p * C + ch].  grids: a list of levels, each a list of
    three [1, C, H, W] (or [C, H, W]) planes read at the components (0, 1), (0, 2), (1, 2) of the normalised point g; level l > 0 is
    added to the running sum while `level` > l and the sum is repeated otherwise.  quantise: read round(v * 16) / 16 (ties to even) for
    a texel v.  The transform from pts to g:
      contract=None, aabb (2, 3)   normalize_aabb: g = (pts - aabb[0]) * (2 / (aabb[1] - aabb[0])) - 1
      contract=None, aabb=None     g = pts (already normalised, as interpolate_ms_features takes them)
      contract=(pca_mean, rotation, variance, aabb, con_aabb), or a dict of these names: TriPlaneField.forward's PCA step,
                                   contract_to_unisphere and con_normalize_aabb
      contract=dict(aabb=, con_aabb=)   con_normalize_aabb alone (get_density on points that are contracted already)
    Differentiable in the planes and, with contract=None, in pts; nothing is saved when no gradient is pending."""
    who = "ms_triplane_sample"
    planes, shapes, named = _check(pts, grids, level, who)
    mode, xform = _transform(contract, aabb, named, who)
    _same_cuda(named, who)
    plan = _Plan(shapes, level, quantise, mode)
    pts_grad = pts.requires_grad and contract is None
    if torch.is_grad_enabled() and (pts_grad or any(t.requires_grad for t in planes)):
        return _Sample.apply(plan, pts if pts_grad else pts.detach(), xform, *planes)
    return _forward(plan, pts.detach().contiguous(), [t.detach().reshape(s).contiguous() for t, s in zip(planes, shapes)], xform)


def interpolate_ms_features(pts, ms_grids, grid_dimensions, concat_features, num_levels, level=1):
    """scene/triplane.py's interpolate_ms_features for points that are already normalised to [-1, 1] (leading dimensions are
    flattened, as the reference's .view(-1, C) does).  Only grid_dimensions=2 with concat_features=True, what TriPlaneField uses."""
    if grid_dimensions != 2 or concat_features is not True:
        raise ValueError(f"interpolate_ms_features: only grid_dimensions=2, concat_features=True (got {grid_dimensions!r}, {concat_features!r})")
    grids = list(ms_grids)
    if num_levels is not None:
        grids = grids[:num_levels]
    if isinstance(pts, torch.Tensor) and pts.dim() > 2:
        pts = pts.reshape(-1, pts.shape[-1])
    return ms_triplane_sample(pts, grids, level=level)


_PAIRS = ((0, 1), (0, 2), (1, 2))   # plane p spans these two coordinates, the first along W


def contract_to_unisphere(x, lo, hi):
    """The scene contraction in torch, for set_aabb (forward runs the same arithmetic inside the kernel): x is mapped so that the
    box [lo, hi] becomes [-1, 1]^3, the unit ball stays where it is and everything outside it is drawn into the shell of radius 1 to 2;
    the result is shifted into [0, 1]^3.  Both branches are evaluated and blended with a 0 / 1 factor, so the origin (1 / r = inf)
    comes out NaN, as in the reference."""
    u = (x - lo) / (hi - lo) * 2 - 1
    r = torch.linalg.norm(u, dim=-1, keepdim=True)
    outside = (r > 1).to(u.dtype)
    u = (2 - 1 / r) * (u / r) * outside + u * (1 - outside)
    return u / 4 + 0.5


def _level_planes(channels, reso, device):
    """The three planes of one level, [1, C, reso[j], reso[i]] for the coordinate pair (i, j), drawn from U(-0.01, 0.01) in plane order."""
    return nn.ParameterList(nn.Parameter(torch.empty(1, channels, reso[j], reso[i], device=device).uniform_(-0.01, 0.01)) for i, j in _PAIRS)


class TriPlaneField(nn.Module):
    """scene/triplane.py's TriPlaneField.  planeconfig: {"grid_dimensions": 2, "input_coordinate_dim": 3, "output_coordinate_dim": C,
    "resolution": [rx, ry, rz]}.  `device`: where the parameters are created (default: the GPU when there is one; a CPU module only
    holds state, as gauspcc_amd.triplane.Triplane)."""

    def __init__(self, bounds, planeconfig, multires, contract, comp_iter, layers_arm=[16, 16, 16, 16], n_ctx_rowcol=2, device=None):
        super().__init__()
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        config = dict(planeconfig)
        if config["grid_dimensions"] != 2 or config["input_coordinate_dim"] != 3 or len(config["resolution"]) != 3:
            raise ValueError("TriPlaneField: only grid_dimensions=2 over 3 coordinates (three planes per level)")
        self.aabb = nn.Parameter(torch.tensor([[bounds, bounds, bounds], [-bounds, -bounds, -bounds]], dtype=torch.float32, device=device),
                                 requires_grad=False)
        self.grid_config = [planeconfig]
        self.multiscale_res_multipliers = multires
        self.concat_features = True
        self.total_bits = 0
        self.resolutions = config["resolution"]
        self.init_itr = comp_iter
        self.out_channels = config["output_coordinate_dim"]
        self.rotation_matrix = nn.Parameter(torch.eye(3, device=device), requires_grad=True)
        self.pca_mean = nn.Parameter(torch.zeros(3, device=device), requires_grad=True)
        self.variance = nn.Parameter(torch.ones(3, device=device), requires_grad=True)
        self.con_aabb = nn.Parameter(torch.ones([2, 3], device=device), requires_grad=True)
        self.grids = nn.ModuleList()
        self.feat_dim = 0
        reso = list(self.resolutions)
        for res in self.multiscale_res_multipliers:
            reso = [r * res for r in self.resolutions]
            self.grids.append(_level_planes(config["output_coordinate_dim"], reso, device))
            self.feat_dim += 3 * config["output_coordinate_dim"]
        self.log_2_encoder_gains = nn.Parameter(torch.arange(0., 5, device=device), requires_grad=True)
        non_zero_pixel_ctx = int((5 ** 2 - 1) / 2)
        self.arm = ArmMLP(non_zero_pixel_ctx, layers_arm).to(device)
        self.arm2 = ArmMLP(non_zero_pixel_ctx, layers_arm).to(device)
        self.arm3 = ArmMLP(non_zero_pixel_ctx, layers_arm).to(device)
        self.contract = contract
        self.num_param = (reso[-1] ** 2) * 1.5 * config["output_coordinate_dim"]
        self.n_ctx_rowcol = n_ctx_rowcol
        self.output_dim = config["output_coordinate_dim"]
        self.mask_size = 2 * n_ctx_rowcol + 1

    def set_aabb(self, rotated_points, xyz_max, xyz_min):
        """With contract: con_aabb becomes the bounding box of the contracted points and aabb the unit box [-1, 1]^3; otherwise aabb
        becomes (xyz_min, xyz_max).  Both are replaced by new parameters, as in the reference."""
        dev = self.aabb.device
        if self.contract:
            one = torch.ones(3, device=rotated_points.device)
            y = contract_to_unisphere(rotated_points.detach(), -one, one)
            self.con_aabb = nn.Parameter(torch.stack([y.min(dim=0).values, y.max(dim=0).values]).to(dev), requires_grad=True)
            box = torch.stack([-one, one])
        else:
            box = torch.stack([xyz_min.detach().reshape(3), xyz_max.detach().reshape(3)])
        self.aabb = nn.Parameter(box.to(device=dev, dtype=torch.float32), requires_grad=True)

    def set_rotation_matrix(self, rotation_matrix, mean, variance):
        self.rotation_matrix = nn.Parameter(rotation_matrix, requires_grad=False)
        self.pca_mean = nn.Parameter(mean, requires_grad=False)
        self.variance = nn.Parameter(variance, requires_grad=False)

    def contract_to_unisphere(self, x, aabb):
        """aabb: the six values (lo, hi) of the box that becomes [-1, 1]^3, as the reference passes them."""
        return contract_to_unisphere(x, aabb[..., :3], aabb[..., 3:])

    def _sent_latents(self, noise):
        """[latents of plane 0 per level, of plane 1, of plane 2]: latent * 16 rounded, or with U(-0.5, 0.5) noise drawn level by level,
        plane by plane (the reference's order, one rand_like per latent); the gradient is one either way, as UniformNoiseQuantizer's."""
        sent = ([], [], [])
        for level in self.grids:
            for ii, latent in enumerate(level):
                y = latent * QUANT
                sent[ii].append(y + (torch.rand_like(y) - 0.5) if noise else _RoundSTE.apply(y))
        return sent

    def _features(self, pts, itr, contract):
        grids = [list(g) for g in self.grids]
        pts = pts.reshape(-1, pts.shape[-1])
        quantise = itr > self.init_itr or itr == -1
        if quantise:
            sent = self._sent_latents(noise=itr != -1)
            self.total_bits = arm_rate(sent[0], self.arm) + arm_rate(sent[1], self.arm2) + arm_rate(sent[2], self.arm3)
        if contract is None:
            features = ms_triplane_sample(pts, grids, level=2, quantise=quantise, aabb=self.aabb)
        else:
            features = ms_triplane_sample(pts, grids, level=2, quantise=quantise, contract=contract)
        return (features, self.total_bits) if quantise else (features, 0)

    def get_density(self, pts, timestamps=None, itr=-1):
        """(features, total_bits) as the reference's get_density: with contract, pts are contract_to_unisphere's output and only
        con_normalize_aabb is applied (they get no gradient); otherwise normalize_aabb.  itr <= comp_iter and not -1: raw planes and
        the integer 0; otherwise planes quantised to 1 / 16 and the three ARMs' summed rate (itr == -1: of the rounded latents; in
        training: of latent * 16 + U(-0.5, 0.5))."""
        if self.contract == True:   # noqa: E712
            return self._features(pts, itr, dict(aabb=self.aabb, con_aabb=self.con_aabb))
        return self._features(pts, itr, None)

    def forward(self, pts, timestamps=None, itr=-1):
        """get_density behind the PCA step and the contraction (with contract), all in one kernel."""
        if self.contract:
            return self._features(pts, itr, (self.pca_mean, self.rotation_matrix, self.variance, self.aabb, self.con_aabb))
        return self._features(pts, itr, None)

    def save_latent(self, save_path, itr):
        grids_hat = [[torch.round(latent * QUANT) for latent in level] for level in self.grids]
        torch.save(grids_hat, os.path.join(save_path, f'grids_hat_{itr}.pth'))
