"""Float64 restatement of the rasteriser's depth and opacity maps (extras= of gauspcc_amd.rasterizer), on top of tests/raster_ref.py: the
same projection, tile rectangles, list order and blend decisions, and the image in raster_ref.render's own operations.  Per pixel, over the
Gaussians it blends in list order with w_i = alpha_i T_i:  invdepth = sum_i w_i / tz_i (no background term, not normalised) and
alpha = 1 - T_end, the transmittance the colour's background term uses; pixels no Gaussian reaches hold 0 in both."""
import numpy as np
import torch

from tests import raster_ref as rr

BX, BY = rr.BX, rr.BY


def _tiles(ix, iy, A, B, C, tz, op, radii, W, H):
    """Per non-empty tile: (ty, tx), the list's Gaussian ids, the tile's pixel rows and columns, power and alpha (pixels, entries) --
    raster_ref.render's expressions."""
    gx, gy = (W + BX - 1) // BX, (H + BY - 1) // BY
    vis = torch.as_tensor(radii).reshape(-1) > 0
    rx0, ry0, rx1, ry1 = rr.tile_rects(ix, iy, radii, W, H)
    order = np.lexsort((np.arange(len(tz)), tz.detach().float().numpy()))   # depth (the device's fp32 keys), then index
    order = torch.as_tensor(order)
    for ty in range(gy):
        for tx in range(gx):
            inside = vis & (rx0 <= tx) & (tx < rx1) & (ry0 <= ty) & (ty < ry1)
            ids = order[inside[order]]
            if len(ids) == 0:
                continue
            ys = torch.arange(ty * BY, min(H, ty * BY + BY))
            xs = torch.arange(tx * BX, min(W, tx * BX + BX))
            yy, xx = torch.meshgrid(ys, xs, indexing="ij")
            yy, xx = yy.reshape(-1), xx.reshape(-1)
            dx = ix[ids][None, :] - xx[:, None].double()
            dy = iy[ids][None, :] - yy[:, None].double()
            power = -0.5 * (A[ids][None, :] * dx * dx + C[ids][None, :] * dy * dy) - B[ids][None, :] * dx * dy
            G = torch.exp(power)
            a_raw = op[ids][None, :] * G
            a = a_raw - (a_raw - 0.99).clamp(min=0).detach()
            yield (ty, tx), ids, yy, xx, power, a


def _decide(power, a):
    """The forward's decisions: included entries, T after each of them, and the entry a pixel stops in front of."""
    inc = (power.detach() <= 0) & (a.detach() >= 1.0 / 255.0)
    ae = torch.where(inc, a.detach(), torch.zeros_like(a))
    tin = torch.cumprod(1 - ae, 1)
    sat = inc & (tin < 1e-4)
    return inc, tin, sat


def render_aux(means3D, opacities, colors, scales, rotations, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H, bg, radii, keep=None,
               project=rr.project):
    """raster_ref.render's arguments -> image (3, H, W), invdepth (1, H, W), alpha (1, H, W), float64, and the per-tile decisions."""
    ix, iy, A, B, C, tz = project(means3D, scales, rotations, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H)
    op = opacities.double().reshape(-1)
    col = colors.double()
    bgd = torch.as_tensor(bg).double().reshape(3)
    img = bgd[None, None, :].expand(H, W, 3).clone()
    inv = torch.zeros(H, W, dtype=torch.float64)
    alp = torch.zeros(H, W, dtype=torch.float64)
    decisions = {}
    for tile, ids, yy, xx, power, a in _tiles(ix, iy, A, B, C, tz, op, radii, W, H):
        if keep is None:
            inc, _, sat = _decide(power, a)
            k = inc & (torch.cumsum(sat.to(torch.int64), 1) == 0)
        else:
            k = keep[tile]
        decisions[tile] = k
        ak = torch.where(k, a, torch.zeros_like(a))
        om = 1 - ak
        tex = torch.cat([torch.ones_like(om[:, :1]), torch.cumprod(om, 1)[:, :-1]], 1)
        w = ak * tex
        t_end = torch.prod(om, 1)
        out = w @ col[ids] + t_end[:, None] * bgd[None, :]
        img = img.index_put((yy, xx), out)
        inv = inv.index_put((yy, xx), w @ (1.0 / tz[ids]))
        alp = alp.index_put((yy, xx), 1 - t_end)
    return img.permute(2, 0, 1), inv[None], alp[None], decisions


def stop_stats(means3D, opacities, scales, rotations, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H, radii, project=rr.project):
    """(share of the pixels whose list runs into the stop rule, min |T_after / 1e-4 - 1| over every (pixel, included entry) up to and
    including the one the pixel stops in front of): how far the scene keeps from the 1e-4 threshold that fp32 and fp64 must decide alike."""
    ix, iy, A, B, C, tz = project(means3D, scales, rotations, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H)
    op = opacities.double().reshape(-1)
    stopped, margin = 0, float("inf")
    for _, _, _, _, power, a in _tiles(ix, iy, A, B, C, tz, op, radii, W, H):
        inc, tin, sat = _decide(power, a)
        nsat = torch.cumsum(sat.to(torch.int64), 1)
        upto = inc & ((nsat == 0) | (sat & (nsat == 1)))
        stopped += int(sat.any(1).sum())
        if upto.any():
            margin = min(margin, float((tin[upto] / 1e-4 - 1).abs().min()))
    return stopped / (W * H), margin


def wall_scene(seed, n=40, W=32, H=32):
    """A wall in front of the camera of raster_ref.scene(): n wide Gaussians (sigma about 12 pixels, opacity 0.6 .. 0.95) at sorted view depths
    3 .. 9 with centres in the middle 16 pixels, so that every pixel's list runs into the stop rule (T below 1e-4) well before its end."""
    sc = rr.scene(n, seed, W, H)
    rng = np.random.RandomState(seed)
    fx, fy = W / (2 * sc["tx"]), H / (2 * sc["ty"])
    z = np.sort(rng.uniform(3.0, 9.0, n)).astype(np.float32)
    px, py = rng.uniform(W / 2 - 8, W / 2 + 8, n), rng.uniform(H / 2 - 8, H / 2 + 8, n)
    sc["means"][:, 0] = ((px + 0.5 - W / 2) / fx * z).astype(np.float32)
    sc["means"][:, 1] = ((py + 0.5 - H / 2) / fy * z).astype(np.float32)
    sc["means"][:, 2] = z - 6.0
    sigma = rng.uniform(11.0, 13.0, (n, 1))
    sc["scales"][:] = (sigma * z[:, None] / fx * np.exp(rng.uniform(-0.1, 0.1, (n, 3)))).astype(np.float32)
    sc["opac"][:, 0] = rng.uniform(0.6, 0.95, n).astype(np.float32)
    return sc


WALL_SEED = 6           # chosen on the CPU for stop_stats' margin and raster_ref.blend_margin (tests/test_raster_aux_ref_cpu.py)
