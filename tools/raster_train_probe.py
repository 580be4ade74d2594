#!/usr/bin/env python3
"""Developer probe: the rasteriser's training path on the 1 M-anchor synthetic RD frame of tools/rd_frame_probe.py (1600 x 1060) -- the
inference forward, the training forward (gsr_forward_train) and the backward (gsr_backward: k_render_backward + k_preprocess_backward) timed
apart with events on the stream, median of `reps` after warm-up.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel table.
    python tools/raster_train_probe.py [anchors] [reps]"""
import math
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gauspcc_amd.neural_gaussians import generate_neural_gaussians  # noqa: E402
from gauspcc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, _RasterizeGaussians  # noqa: E402
from gauspcc_amd.synth import SyntheticGaussianModel  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
W, H = 1600, 1060
dev = torch.device("cuda", 0)
enc = SyntheticGaussianModel(n, seed=0, device="cuda:0")
with torch.no_grad():
    enc._anchor, enc._scaling, enc._mask = enc.get_anchor.clone(), enc.get_scaling.clone(), enc.get_mask.clone()
enc.decoded_version = True
ctr = enc._anchor.mean(dim=0); ext = float((enc._anchor.max(dim=0).values - enc._anchor.min(dim=0).values).max())
eye = ctr + torch.tensor([0.0, 0.0, -1.4 * ext], device=dev)
Rt = torch.eye(4, device=dev); Rt[:3, 3] = -eye
fovx = math.radians(60); fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
zn, zf = 0.01, 100.0
P = torch.zeros(4, 4, device=dev)
P[0, 0] = 1 / math.tan(fovx / 2); P[1, 1] = 1 / math.tan(fovy / 2); P[3, 2] = 1.0; P[2, 2] = zf / (zf - zn); P[2, 3] = -(zf * zn) / (zf - zn)
view = Rt.T.contiguous(); full = (view @ P.T).contiguous()
settings = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(fovx / 2), tanfovy=math.tan(fovy / 2), bg=torch.zeros(3, device=dev),
                                         scale_modifier=1.0, viewmatrix=view, projmatrix=full, sh_degree=1, campos=eye, prefiltered=False, debug=False)
rast = GaussianRasterizer(settings)
with torch.no_grad():
    xyz, color, opacity, scaling, rot, _ = generate_neural_gaussians(types.SimpleNamespace(camera_center=eye), enc, None)
R = torch.randn((3, H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(0))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


inf, fwd, bwd = [], [], []
for it in range(reps + 3):
    with torch.no_grad():
        t_inf, _ = timed(lambda: rast(means3D=xyz, means2D=None, shs=None, colors_precomp=color, opacities=opacity, scales=scaling, rotations=rot, cov3D_precomp=None))
    leaves = [t.detach().clone().requires_grad_(True) for t in (xyz, opacity, color, scaling, rot)]
    t_fwd, (img, radii) = timed(lambda: _RasterizeGaussians.apply(leaves[0], None, leaves[1], leaves[2], leaves[3], leaves[4], None, settings, {}))
    loss = (img * R).sum()
    torch.cuda.synchronize()
    t_bwd, _ = timed(lambda: torch.autograd.grad(loss, leaves))
    if it >= 3:
        inf.append(t_inf); fwd.append(t_fwd); bwd.append(t_bwd)
mi, mf, mb = statistics.median(inf), statistics.median(fwd), statistics.median(bwd)
print(f"{xyz.shape[0]} Gaussians, {int((radii > 0).sum())} visible, {rast.num_rendered} tile instances (reference count), {W}x{H}")
print(f"inference forward  {mi:.3f} ms (median of {reps}; min {min(inf):.3f})")
print(f"training forward   {mf:.3f} ms (min {min(fwd):.3f})  = {mf / mi:.3f} x inference")
print(f"backward           {mb:.3f} ms (min {min(bwd):.3f})  (autograd.grad of <image, R>: the loss's own backward, gsr_backward and the grads' casts)")
