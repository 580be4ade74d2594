"""Differentiable float64 restatement of the rasteriser forward (gauspcc_amd/csrc/rasterizer.hip), the yardstick of its backward.

It follows the forward's math and the gradient conventions of diff_gaussian_rasterization: each Gaussian is binned into every tile of
its rectangle (the device's exact tile culling drops only pairs that never blend), the tile's list is sorted by depth (ties by index),
and the blend skips power > 0 and alpha < 1/255 and stops in front of the Gaussian that would take T below 1e-4.  alpha = min(0.99, o G)
passes the gradient as if the min were not there; a view-space coordinate clamped at +-1.3 tan(fov) enters the Jacobian as a constant.
The discrete decisions are not differentiated; `keep` (from a first call) freezes them for gradcheck.
"""
import numpy as np
import torch

BX = BY = 16


def scene(n, seed, W, H):
    """The scene generator of tests/test_gpu_rasterizer.py (camera at z = -6 looking down +z, a twentieth behind the camera)."""
    from tests.test_gpu_rasterizer import _scene

    return _scene(n, seed, W, H)


def training_scene(n, seed, W, H, cluster=0):
    """scene(), plus what the backward has to get right: Gaussians past the frustum's side that the +-1.3 tan(fov) clamp catches but that
    still reach the image, opacities at the 0.99 cap (saturation), and optionally `cluster` small Gaussians inside one tile (lists longer
    than two LDS batches)."""
    sc = scene(n, seed, W, H)
    rng = np.random.RandomState(seed + 1)
    m, s, o = sc["means"], sc["scales"], sc["opac"]
    k = max(4, n // 40)
    z = rng.uniform(1.0, 3.0, k).astype(np.float32)                       # view depth z + 6
    side = np.where(rng.rand(k) < 0.5, -1.0, 1.0).astype(np.float32)
    m[n // 20: n // 20 + k, 0] = side * 1.6 * sc["tx"] * (z + 6.0)          # |x / z| = 1.6 tan(fov_x) > 1.3 tan(fov_x)
    m[n // 20: n // 20 + k, 1] = rng.uniform(-0.5, 0.5, k) * (z + 6.0) * sc["ty"]
    m[n // 20: n // 20 + k, 2] = z
    s[n // 20: n // 20 + k] = np.float32(0.25 * (z + 6.0) * sc["tx"])[:, None] * np.ones((1, 3), np.float32)
    hi = rng.rand(n) < 0.15
    o[hi, 0] = rng.uniform(0.97, 1.0, hi.sum()).astype(np.float32)
    if cluster:
        c = slice(n - cluster, n)
        # inside the tile (1, 1): pixels 16..31; x_pix = (x / z) focal + W / 2
        fx = W / (2 * sc["tx"])
        zz = rng.uniform(3.0, 8.0, cluster).astype(np.float32)
        px = rng.uniform(18, 30, cluster).astype(np.float32)
        py = rng.uniform(18, 30, cluster).astype(np.float32)
        fy = H / (2 * sc["ty"])
        m[c, 0] = (px - W / 2) / fx * zz
        m[c, 1] = (py - H / 2) / fy * zz
        m[c, 2] = zz - 6.0
        s[c] = np.exp(rng.randn(cluster, 3).astype(np.float32) * 0.3 - 4.0)
        o[c, 0] = rng.uniform(0.02, 0.2, cluster).astype(np.float32)
    return sc


def project(means3D, scales, rots, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H):
    """k_preprocess in float64: pixel centre, conic (A, B, C) and depth of every Gaussian."""
    V, M = view.reshape(-1).double(), proj.reshape(-1).double()
    p = means3D.double()
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    tx0 = V[0] * px + V[4] * py + V[8] * pz + V[12]
    ty0 = V[1] * px + V[5] * py + V[9] * pz + V[13]
    tz = V[2] * px + V[6] * py + V[10] * pz + V[14]
    hx = M[0] * px + M[4] * py + M[8] * pz + M[12]
    hy = M[1] * px + M[5] * py + M[9] * pz + M[13]
    hw = M[3] * px + M[7] * py + M[11] * pz + M[15]
    pw = 1.0 / (hw + 1e-7)
    ix = ((hx * pw + 1.0) * W - 1.0) * 0.5
    iy = ((hy * pw + 1.0) * H - 1.0) * 0.5
    if cov3D is not None:
        c = cov3D.double()
        Sig = torch.stack([torch.stack([c[:, 0], c[:, 1], c[:, 2]], -1), torch.stack([c[:, 1], c[:, 3], c[:, 4]], -1),
                           torch.stack([c[:, 2], c[:, 4], c[:, 5]], -1)], -2)
    else:
        s = scale_modifier * scales.double()
        r, x, y, z = [rots.double()[:, k] for k in range(4)]
        R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                         torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                         torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
        Sig = R @ torch.diag_embed(s * s) @ R.transpose(1, 2)
    limx, limy = 1.3 * tanfx, 1.3 * tanfy
    txtz, tytz = tx0 / tz, ty0 / tz
    clx, cly = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
    tx = torch.where(clx, (txtz.clamp(-limx, limx) * tz).detach(), tx0)
    ty = torch.where(cly, (tytz.clamp(-limy, limy) * tz).detach(), ty0)
    fx, fy = W / (2.0 * tanfx), H / (2.0 * tanfy)
    Vr = torch.stack([V[[0, 4, 8]], V[[1, 5, 9]], V[[2, 6, 10]]])            # rows: view-space x, y, z of a world direction
    a0 = (fx / tz)[:, None] * Vr[0] + (-(fx * tx) / (tz * tz))[:, None] * Vr[2]
    a1 = (fy / tz)[:, None] * Vr[1] + (-(fy * ty) / (tz * tz))[:, None] * Vr[2]
    s0, s1 = (Sig @ a0[:, :, None])[:, :, 0], (Sig @ a1[:, :, None])[:, :, 0]
    cxx = (a0 * s0).sum(1) + 0.3
    cxy = (a0 * s1).sum(1)
    cyy = (a1 * s1).sum(1) + 0.3
    det = cxx * cyy - cxy * cxy
    return ix, iy, cyy / det, -cxy / det, cxx / det, tz


def render(means3D, opacities, colors, scales, rotations, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H, bg, radii, keep=None):
    """Image (3, H, W) float64 and the per-tile decisions {tile: keep (pixels, entries)}; radii: the device's (or the oracle's)."""
    ix, iy, A, B, C, tz = project(means3D, scales, rotations, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H)
    op = opacities.double().reshape(-1)
    col = colors.double()
    bgd = torch.as_tensor(bg).double().reshape(3)
    gx, gy = (W + BX - 1) // BX, (H + BY - 1) // BY
    r = torch.as_tensor(radii).reshape(-1).to(torch.float64)
    vis = r > 0
    ixd, iyd = ix.detach(), iy.detach()
    rx0 = torch.trunc((ixd - r) / BX).clamp(0, gx)
    ry0 = torch.trunc((iyd - r) / BY).clamp(0, gy)
    rx1 = torch.trunc((ixd + r + BX - 1) / BX).clamp(0, gx)
    ry1 = torch.trunc((iyd + r + BY - 1) / BY).clamp(0, gy)
    order = np.lexsort((np.arange(len(tz)), tz.detach().float().numpy()))   # depth (the device's fp32 keys), then index
    order = torch.as_tensor(order)
    img = bgd[None, None, :].expand(H, W, 3).clone()
    decisions = {}
    for ty in range(gy):
        for tx in range(gx):
            inside = vis & (rx0 <= tx) & (tx < rx1) & (ry0 <= ty) & (ty < ry1)
            ids = order[inside[order]]
            ys = torch.arange(ty * BY, min(H, ty * BY + BY))
            xs = torch.arange(tx * BX, min(W, tx * BX + BX))
            yy, xx = torch.meshgrid(ys, xs, indexing="ij")
            yy, xx = yy.reshape(-1), xx.reshape(-1)
            if len(ids) == 0:
                continue
            dx = ix[ids][None, :] - xx[:, None].double()
            dy = iy[ids][None, :] - yy[:, None].double()
            power = -0.5 * (A[ids][None, :] * dx * dx + C[ids][None, :] * dy * dy) - B[ids][None, :] * dx * dy
            G = torch.exp(power)
            a_raw = op[ids][None, :] * G
            a = a_raw - (a_raw - 0.99).clamp(min=0).detach()
            if keep is None:
                inc = (power.detach() <= 0) & (a.detach() >= 1.0 / 255.0)
                ae = torch.where(inc, a.detach(), torch.zeros_like(a))
                tin = torch.cumprod(1 - ae, 1)
                sat = inc & (tin < 1e-4)
                k = inc & (torch.cumsum(sat.to(torch.int64), 1) == 0)
            else:
                k = keep[(ty, tx)]
            decisions[(ty, tx)] = k
            ak = torch.where(k, a, torch.zeros_like(a))
            om = 1 - ak
            tex = torch.cat([torch.ones_like(om[:, :1]), torch.cumprod(om, 1)[:, :-1]], 1)
            w = ak * tex
            out = w @ col[ids] + torch.prod(om, 1)[:, None] * bgd[None, :]
            img = img.index_put((yy, xx), out)
    return img.permute(2, 0, 1), decisions


def tensors(sc, device, dtype=torch.float32):
    return {k: torch.tensor(v, dtype=dtype, device=device) for k, v in sc.items() if isinstance(v, np.ndarray)}


def camera(sc):
    return sc["view"], sc["proj"], float(sc["tx"]), float(sc["ty"])

