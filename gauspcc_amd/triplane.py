"""TC-GS's tri-plane context sampler on the device (gsge_plane_forward / gsge_plane_backward, and the context rows gsge_plane_rows_forward /
_backward: the features with a row-aligned tail behind them, `triplane_rows` / `Triplane.context_rows`): a drop-in for utils/triplane.py,

    from utils.triplane import Triplane   ->   from gauspcc_amd.triplane import Triplane      (TC-GS/scene/gaussian_model.py:27)

`sample_from_planes` keeps the reference's signature and (N, K, 3, C) result; `triplane_sample` is the native form that returns the
(N, K * 3 * C) tensor `Triplane.sample` reshapes it to.  Both are differentiable in the planes and, when they require grad, in the
coordinates; the backward uses no float atomics, so gradients are bitwise reproducible from run to run and across streams.

The repeat form: three of the reference's call sites sample `anchor.unsqueeze(1).repeat(1, K, 1)`, K identical samples per anchor.
Pass the (N, 3) anchors with `repeat=K` instead: each anchor is sampled once and written K times (the same bits as the materialised
call), and the backward adds the K gradient copies before they are scattered.

Differences from the reference: only mode='bilinear', padding_mode='zeros', box_warp=1 and the three fixed plane axes of
`generate_planes` (ValueError otherwise); `radii=None` raises as it fails there; float32 CUDA tensors only (TypeError for another dtype,
RuntimeError for CPU tensors: there is no CPU path); a sample whose pixel coordinate is not finite (NaN / inf coordinates) yields zeros
and no gradient, where torch would index with it.  The module imports no `nvdiffrast`; `TriMipEncoding`, which TC-GS never instantiates,
is not provided.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, runtime
from .runtime import ptr

MAX_CHANNELS, MAX_SIZE, MAX_REPEAT = 256, 4096, 64   # gsge_plane_forward's limits

_AXES = (((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((1, 0, 0), (0, 0, 1), (0, 1, 0)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)))


def generate_planes(device=None):
    """The three fixed plane axes of the reference, (3, 3, 3) float32."""
    return torch.tensor(_AXES, dtype=torch.float32, device=device)


def _f32_cuda(t, name, who):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a CUDA tensor (got {t.device}); gauspcc_amd has no CPU path")
    return t


def _check(planes, coordinates, max_coords, min_coords, radii, repeat, who):
    for t, name in ((planes, "planes"), (coordinates, "coordinates"), (max_coords, "max_coords"), (min_coords, "min_coords")):
        _f32_cuda(t, name, who)
        if t.device != planes.device:
            raise ValueError(f"{who}: {name} on {t.device}, planes on {planes.device}")
    if radii is None:
        raise ValueError(f"{who}: radii is None (the reference fails there too: mag_sq is undefined)")
    if planes.dim() != 4 or planes.shape[0] != 3:
        raise ValueError(f"{who}: planes must be (3, C, H, W), got {tuple(planes.shape)}")
    _, C, H, W = planes.shape
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"{who}: {C} channels outside [1, {MAX_CHANNELS}]")
    if not (2 <= H <= MAX_SIZE and 2 <= W <= MAX_SIZE):
        raise ValueError(f"{who}: planes of {H} x {W} outside [2, {MAX_SIZE}]")
    if max_coords.numel() != 3 or min_coords.numel() != 3:
        raise ValueError(f"{who}: max_coords / min_coords must hold 3 values, got {tuple(max_coords.shape)} and {tuple(min_coords.shape)}")
    if repeat is None:
        if coordinates.dim() != 3 or coordinates.shape[2] != 3 or coordinates.shape[1] < 1:
            raise ValueError(f"{who}: coordinates must be (N, K, 3) with K >= 1, got {tuple(coordinates.shape)}")
        return coordinates.shape[0], coordinates.shape[1]
    if isinstance(repeat, bool) or not isinstance(repeat, int) or not 1 <= repeat <= MAX_REPEAT:
        raise ValueError(f"{who}: repeat must be an int in [1, {MAX_REPEAT}], got {repeat!r}")
    if coordinates.dim() != 2 or coordinates.shape[1] != 3:
        raise ValueError(f"{who}: with repeat, coordinates must be (N, 3), got {tuple(coordinates.shape)}")
    return coordinates.shape[0], repeat


def _forward(planes, coords, mx, mn, radii, N, K, repeat):
    dev = planes.device
    C, H, W = planes.shape[1:]
    out = torch.empty((N, K * 3 * C), dtype=torch.float32, device=dev)
    if N:
        _lib.check(_lib.lib().gsge_plane_forward(runtime.context(dev), planes.data_ptr(), coords.data_ptr(), mx.data_ptr(), mn.data_ptr(), float(radii),
                                                 N, K, int(repeat), C, H, W, out.data_ptr(), runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
    return out


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, planes, coordinates, mx, mn, radii, N, K, repeat):
        p, c = planes.detach().contiguous(), coordinates.detach().contiguous()
        out = _forward(p, c, mx, mn, radii, N, K, repeat)
        ctx.save_for_backward(p, c, mx, mn)
        ctx.args = (radii, N, K, repeat)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        p, c, mx, mn = ctx.saved_tensors
        radii, N, K, repeat = ctx.args
        dev = p.device
        C, H, W = p.shape[1:]
        g = grad.to(torch.float32).contiguous()
        gp = torch.empty_like(p)
        gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        if N == 0:
            return gp.zero_(), gc, None, None, None, None, None, None
        _lib.check(_lib.lib().gsge_plane_backward(runtime.context(dev), g.data_ptr(), p.data_ptr(), c.data_ptr(), mx.data_ptr(), mn.data_ptr(), float(radii),
                                                  N, K, int(repeat), C, H, W, gp.data_ptr(), ptr(gc), runtime.Workspace(dev).fn(), None,
                                                  runtime.stream_ptr(dev)))
        return (gp if ctx.needs_input_grad[0] else None), gc, None, None, None, None, None, None


def triplane_sample(planes, coordinates, max_coords, min_coords, radii, repeat=None):
    """The (N, K * 3 * C) tri-plane features of `coordinates` (N, K, 3), or of (N, 3) coordinates written `repeat` = K times:
    out[n, (k * 3 + p) * C + ch].  planes (3, C, H, W); max_coords, min_coords 3 values; radii a float (Triplane passes
    0.5 * spatial_lr_scale).  Differentiable in planes and coordinates; nothing is saved when no gradient is pending."""
    N, K = _check(planes, coordinates, max_coords, min_coords, radii, repeat, "triplane_sample")
    mx, mn = max_coords.detach().reshape(3).contiguous(), min_coords.detach().reshape(3).contiguous()
    if torch.is_grad_enabled() and (planes.requires_grad or coordinates.requires_grad):
        return _Sample.apply(planes, coordinates, mx, mn, float(radii), N, K, repeat is not None)
    return _forward(planes.detach().contiguous(), coordinates.detach().contiguous(), mx, mn, float(radii), N, K, repeat is not None)


MAX_TAIL = 16   # gsge_plane_rows_forward's limit


def _rows_forward(planes, coords, tail, mx, mn, radii, N, K, repeat):
    dev = planes.device
    C, H, W = planes.shape[1:]
    T = tail.shape[1]
    out = torch.empty((N, K * 3 * C + T), dtype=torch.float32, device=dev)
    if N:
        _lib.check(_lib.lib().gsge_plane_rows_forward(runtime.context(dev), planes.data_ptr(), coords.data_ptr(), mx.data_ptr(), mn.data_ptr(), float(radii),
                                                      N, K, int(repeat), C, H, W, ptr(tail) if T else None, T, out.data_ptr(),
                                                      runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
    return out


class _Rows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, planes, coordinates, tail, mx, mn, radii, N, K, repeat):
        p, c = planes.detach().contiguous(), coordinates.detach().contiguous()
        out = _rows_forward(p, c, tail.detach().contiguous(), mx, mn, radii, N, K, repeat)
        ctx.save_for_backward(p, c, mx, mn)
        ctx.args = (radii, N, K, repeat, tail.shape[1])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        p, c, mx, mn = ctx.saved_tensors
        radii, N, K, repeat, T = ctx.args
        dev = p.device
        C, H, W = p.shape[1:]
        g = grad.to(torch.float32).contiguous()      # the whole (N, K 3 C + T) gradient as it arrives: the kernels read its feature columns in place
        row = K * 3 * C
        gp = gc = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gp = torch.empty_like(p)
            gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
            if N == 0:
                gp.zero_()
            else:
                _lib.check(_lib.lib().gsge_plane_rows_backward(runtime.context(dev), g.data_ptr(), p.data_ptr(), c.data_ptr(), mx.data_ptr(), mn.data_ptr(),
                                                               float(radii), N, K, int(repeat), C, H, W, T, gp.data_ptr(), ptr(gc),
                                                               runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
        gt = g[:, row:] if ctx.needs_input_grad[2] else None      # the tail's gradient: a column view, no kernel
        return (gp if ctx.needs_input_grad[0] else None), gc, gt, None, None, None, None, None, None


def triplane_rows(planes, coordinates, tail, max_coords, min_coords, radii, repeat=None):
    """The context rows (gsge_plane_rows_forward): the (N, K * 3 * C + T) tensor whose first K * 3 * C columns are `triplane_sample`'s, bit for
    bit, and whose last T are `tail` (N, T), T in [0, 16] -- torch.cat([triplane_sample(...), tail], dim=1) written once (TC-GS: the anchor,
    T = 3, the input of mlp_triplane).  Coordinates as `triplane_sample` takes them, (N, K, 3) or (N, 3) with `repeat=K`; K <= 64 in both
    forms.  Differentiable in planes, coordinates and tail: the backward reads the upstream gradient in place (no contiguous copy of the
    feature columns) and the tail's gradient is the column view grad[:, K * 3 * C:].  When tail and coordinates are the same tensor (the
    repeat form with the anchor) autograd adds the two."""
    who = "triplane_rows"
    N, K = _check(planes, coordinates, max_coords, min_coords, radii, repeat, who)
    _f32_cuda(tail, "tail", who)
    if tail.device != planes.device:
        raise ValueError(f"{who}: tail on {tail.device}, planes on {planes.device}")
    if tail.dim() != 2 or tail.shape[0] != N or tail.shape[1] > MAX_TAIL:
        raise ValueError(f"{who}: tail must be ({N}, T) with T <= {MAX_TAIL}, got {tuple(tail.shape)}")
    if K > MAX_REPEAT:
        raise ValueError(f"{who}: K = {K} above {MAX_REPEAT} (a workgroup owns whole rows)")
    mx, mn = max_coords.detach().reshape(3).contiguous(), min_coords.detach().reshape(3).contiguous()
    if torch.is_grad_enabled() and (planes.requires_grad or coordinates.requires_grad or tail.requires_grad):
        return _Rows.apply(planes, coordinates, tail, mx, mn, float(radii), N, K, repeat is not None)
    return _rows_forward(planes.detach().contiguous(), coordinates.detach().contiguous(), tail.detach().contiguous(), mx, mn, float(radii), N, K,
                         repeat is not None)


def sample_from_planes(plane_axes, plane_features, coordinates, max_coords, min_coords, mode='bilinear', padding_mode='zeros', box_warp=1, radii=None):
    """utils/triplane.py's sample_from_planes: the (N, K, 3, C) features of coordinates (N, K, 3)."""
    if mode != 'bilinear' or padding_mode != 'zeros':
        raise ValueError(f"sample_from_planes: only mode='bilinear', padding_mode='zeros' (got {mode!r}, {padding_mode!r})")
    if box_warp != 1:
        raise ValueError(f"sample_from_planes: only box_warp=1 (got {box_warp!r})")
    if radii is None:
        raise ValueError("sample_from_planes: radii is None (the reference fails there too: mag_sq is undefined)")
    if plane_axes is not None:
        ax = torch.as_tensor(plane_axes).detach().cpu().to(torch.float32)
        if tuple(ax.shape) != (3, 3, 3) or not torch.equal(ax, generate_planes()):
            raise ValueError("sample_from_planes: plane_axes must be the three fixed axis matrices of generate_planes()")
    out = triplane_sample(plane_features, coordinates, max_coords, min_coords, radii)
    return out.view(coordinates.shape[0], coordinates.shape[1], 3, plane_features.shape[1])


class Autoencoder(nn.Module):
    """The reference's small conv autoencoder over one plane (torch modules; names as in utils/triplane.py)."""

    def __init__(self, feat, res, compressed_dim):
        super().__init__()
        self.encoder = nn.Sequential(
            nn.Conv2d(feat, 16, kernel_size=3, stride=2, padding=1), nn.ReLU(),
            nn.Conv2d(16, 32, kernel_size=3, stride=2, padding=1), nn.ReLU(),
            nn.Conv2d(32, compressed_dim, kernel_size=3, stride=2, padding=1), nn.ReLU())
        self.decoder = nn.Sequential(
            nn.ConvTranspose2d(compressed_dim, 32, kernel_size=3, stride=2, padding=1, output_padding=1), nn.ReLU(),
            nn.ConvTranspose2d(32, 16, kernel_size=3, stride=2, padding=1, output_padding=1), nn.ReLU(),
            nn.ConvTranspose2d(16, feat, kernel_size=3, stride=2, padding=1, output_padding=1), nn.Sigmoid())

    def forward(self, x):
        compressed = self.encoder(x)
        reconstructed = self.decoder(compressed)
        return compressed.squeeze(), reconstructed.squeeze()


class Triplane(nn.Module):
    """utils/triplane.py's Triplane with the reference's parameter and submodule names (`planes`, `autoencoder.encoder.*`,
    `autoencoder.decoder.*`, attribute `compressed_plane`): state dicts load either way.  `forward` and `sample` also take (N, 3)
    coordinates with `repeat=K` (the repeat form)."""

    def __init__(self, feature_dim, resolution, radii, device=None):
        super().__init__()
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"   # the reference creates the planes on the GPU; a CPU module only holds state
        self.radii = radii
        self.autoencoder = Autoencoder(feature_dim, resolution, 8)
        plane = torch.empty(3, feature_dim, resolution, resolution, device=device)
        torch.nn.init.uniform_(plane, -1e-2, 1e-2)
        self.compressed_plane = torch.empty(0)
        self.planes = nn.Parameter(plane.requires_grad_(True))

    @property
    def plane_axes(self):
        return generate_planes(self.planes.device)

    def get_encode(self):
        return self.compressed_plane

    def forward(self, sample_coordinates, max_coords, min_coords, is_training=0, step=0, repeat=None):
        return self._with_autoencoder(self.sample(self.planes, sample_coordinates, max_coords, min_coords, repeat=repeat), is_training, step)

    def context_rows(self, sample_coordinates, tail, max_coords, min_coords, is_training=0, step=0, repeat=None):
        """`forward` with the context rows [features | tail] (triplane_rows) in place of the features: the same return convention."""
        rows = triplane_rows(self.planes, sample_coordinates, tail, max_coords, min_coords, 0.5 * self.radii, repeat=repeat)
        return self._with_autoencoder(rows, is_training, step)

    def _with_autoencoder(self, out, is_training, step):
        if is_training and step > 15000:
            pairs = [self.autoencoder(self.planes[i].unsqueeze(0)) for i in range(3)]
            compressed = torch.stack([c for c, _ in pairs], dim=0)        # (3, 8, H / 8, W / 8)
            reconstructed = torch.stack([r for _, r in pairs], dim=0)     # (3, C, H, W)
            self.compressed_plane = compressed
            return out, compressed, reconstructed
        if is_training:
            return out, None, None
        return out

    def sample(self, planes, sample_coordinates, max_coords, min_coords, repeat=None):
        return triplane_sample(planes, sample_coordinates, max_coords, min_coords, 0.5 * self.radii, repeat=repeat)
