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


def training_scene(n, seed, W, H, cluster=0, tanfov=None):
    """scene(), plus what the backward has to get right: Gaussians past the frustum's side that the +-1.3 tan(fov) clamp catches but that
    still reach the image, opacities at the 0.99 cap (saturation), and optionally `cluster` small Gaussians inside one tile (lists longer
    than two LDS batches).  tanfov = (tan(FoVx / 2), tan(FoVy / 2)): place them for these instead of scene()'s own (scene_for_camera)."""
    sc = scene(n, seed, W, H)
    if tanfov is not None:
        sc["tx"], sc["ty"] = float(tanfov[0]), float(tanfov[1])
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


def _sigma(scales, rots, cov3D, scale_modifier):
    """The world-space covariances (P, 3, 3): from the six numbers of cov3D_precomp, or R diag((scale_modifier s)^2) R^T of the quaternion (r, x, y, z)."""
    if cov3D is not None:
        c = cov3D.double()
        return torch.stack([torch.stack([c[:, 0], c[:, 1], c[:, 2]], -1), torch.stack([c[:, 1], c[:, 3], c[:, 4]], -1),
                            torch.stack([c[:, 2], c[:, 4], c[:, 5]], -1)], -2)
    s = scale_modifier * scales.double()
    r, x, y, z = [rots.double()[:, k] for k in range(4)]
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                     torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                     torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    return R @ torch.diag_embed(s * s) @ R.transpose(1, 2)


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
    Sig = _sigma(scales, rots, cov3D, scale_modifier)
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


MUTANTS = ("W_transposed", "focal_y_is_focal_x", "view_untransposed")


def _project_matrices(means3D, scales, rots, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H, mutant=None):
    view, proj = view.double().reshape(4, 4), proj.double().reshape(4, 4)
    if mutant == "view_untransposed":                       # the stored matrix read as a column-vector matrix
        view = view.transpose(0, 1)
    p = means3D.double()
    ph = torch.cat([p, torch.ones_like(p[:, :1])], 1)
    t = (ph @ view)[:, :3]
    clip = ph @ proj
    size = torch.tensor([W, H], dtype=torch.float64)
    pix = ((clip[:, :2] / (clip[:, 3:] + 1e-7) + 1.0) * size - 1.0) * 0.5
    tz = t[:, 2]
    Wm = view[:3, :3].transpose(0, 1)
    if mutant == "W_transposed":
        Wm = Wm.transpose(0, 1)
    tan = torch.tensor([tanfx, tanfy], dtype=torch.float64)
    focal = size / (2.0 * tan)
    if mutant == "focal_y_is_focal_x":
        focal = focal[[0, 0]]
    lim = 1.3 * tan
    ratio = t[:, :2] / tz[:, None]
    clamped = (ratio < -lim) | (ratio > lim)
    txy = torch.where(clamped, (torch.minimum(torch.maximum(ratio, -lim), lim) * tz[:, None]).detach(), t[:, :2])
    J = torch.cat([torch.diag_embed(focal / tz[:, None]), (-(focal * txy) / (tz * tz)[:, None])[:, :, None]], 2)      # (P, 2, 3)
    T = J @ Wm
    cov = T @ _sigma(scales, rots, cov3D, scale_modifier) @ T.transpose(1, 2) + 0.3 * torch.eye(2, dtype=torch.float64)
    con = torch.linalg.inv(cov)
    return pix[:, 0], pix[:, 1], con[:, 0, 0], con[:, 0, 1], con[:, 1, 1], tz


def project_matrix_form(means3D, scales, rots, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H):
    """project() in matrix algebra only, with no flat index into either matrix: the yardstick of the camera convention.

    HAC/scene/cameras.py:54-57 stores world_view_transform = getWorld2View2(R, T).transpose(0, 1) and full_proj_transform =
    world_view_transform @ getProjectionMatrix(...).transpose(0, 1).  getWorld2View2 returns the column-vector matrix Rt, p_view = Rt [p 1]^T
    (utils/graphics_utils.py:38-49), and getProjectionMatrix the column-vector P; so with the stored matrices a point is a ROW vector:
    [p 1] @ view = (Rt [p 1]^T)^T and [p 1] @ proj = (P Rt [p 1]^T)^T (geom_transform_points, graphics_utils.py:22-29, multiplies the
    same way).  The rotation that takes a world direction (a column) to view space is Rt[:3, :3] = view[:3, :3]^T = W, and the screen-space
    covariance of EWA splatting is J W Sigma W^T J^T + 0.3 I with J = [[fx / z, 0, -fx x / z^2], [0, fy / z, -fy y / z^2]] at the
    view-space position (x, y, z); a coordinate clamped at +-1.3 tan(fov) z enters J detached, as in project().  The conic is its inverse."""
    return _project_matrices(means3D, scales, rots, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H)


def mutant_projection(name):
    """project_matrix_form with one of MUTANTS: the errors of reading the matrices that an identity rotation with equal focal lengths hides."""
    assert name in MUTANTS

    def f(*a):
        return _project_matrices(*a, mutant=name)
    return f


def tile_rects(ix, iy, radii, W, H):
    """The tile rectangle [rx0, rx1) x [ry0, ry1) of every Gaussian, as k_preprocess takes it from the pixel centre and the radius."""
    gx, gy = (W + BX - 1) // BX, (H + BY - 1) // BY
    r = torch.as_tensor(radii).reshape(-1).to(torch.float64)
    ixd, iyd = ix.detach(), iy.detach()
    rx0 = torch.trunc((ixd - r) / BX).clamp(0, gx)
    ry0 = torch.trunc((iyd - r) / BY).clamp(0, gy)
    rx1 = torch.trunc((ixd + r + BX - 1) / BX).clamp(0, gx)
    ry1 = torch.trunc((iyd + r + BY - 1) / BY).clamp(0, gy)
    return rx0, ry0, rx1, ry1


def render(means3D, opacities, colors, scales, rotations, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H, bg, radii, keep=None,
           project=project):
    """Image (3, H, W) float64 and the per-tile decisions {tile: keep (pixels, entries)}; radii: the device's (or the oracle's);
    project: the projection to render (and differentiate) through, project or project_matrix_form."""
    ix, iy, A, B, C, tz = project(means3D, scales, rotations, cov3D, scale_modifier, view, proj, tanfx, tanfy, W, H)
    op = opacities.double().reshape(-1)
    col = colors.double()
    bgd = torch.as_tensor(bg).double().reshape(3)
    gx, gy = (W + BX - 1) // BX, (H + BY - 1) // BY
    vis = torch.as_tensor(radii).reshape(-1) > 0
    rx0, ry0, rx1, ry1 = tile_rects(ix, iy, radii, W, H)
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



CAMERAS = ("identity", "yaw90", "general", "general_anisotropic", "translated_scaled")


def cameras():
    """tests/golden/cameras.npz, made by the reference's own getWorld2View2 / getProjectionMatrix (tests/golden/make_cameras.py):
    {name: {R, T, FoVx, FoVy, znear, zfar, world_view_transform, full_proj_transform, camera_center, tanfovx, tanfovy}}."""
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cameras.npz"))
    names = [str(n) for n in z["names"]]
    assert tuple(names) == CAMERAS
    return {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in names}


def scene_for_camera(cam, n, seed, W, H, cluster=0):
    """training_scene() seen through a camera of cameras(): laid out in view space for the camera's own tan(fov) (so the clamp band, the
    0.99-opacity share and the one-tile cluster sit where they do for its focal lengths), then carried to the world through the inverse of
    its view matrix.  The layout is training_scene's (view space = means + (0, 0, 6)) plus what only shows with unequal focal lengths:
    a batch past the frustum's top and bottom (clamped in y) and three splats wide enough for a square of more than 64 tiles at
    200 x 120.  Quaternions stay as drawn: random in the world."""
    tx, ty = float(cam["tanfovx"]), float(cam["tanfovy"])
    sc = training_scene(n, seed, W, H, cluster=cluster, tanfov=(tx, ty))
    rng = np.random.RandomState(seed + 2)
    m, s, o = sc["means"], sc["scales"], sc["opac"]
    k = max(4, n // 40)
    a = n // 20 + k                                                         # after training_scene's batch past the sides
    z = rng.uniform(1.0, 3.0, k).astype(np.float32)
    side = np.where(rng.rand(k) < 0.5, -1.0, 1.0).astype(np.float32)
    m[a: a + k, 0] = rng.uniform(-0.5, 0.5, k) * (z + 6.0) * tx
    m[a: a + k, 1] = side * 1.6 * ty * (z + 6.0)                            # |y / z| = 1.6 tan(fov_y) > 1.3 tan(fov_y)
    m[a: a + k, 2] = z
    s[a: a + k] = np.float32(0.25 * (z + 6.0) * ty)[:, None] * np.ones((1, 3), np.float32)
    b = a + k
    zb = rng.uniform(-1.0, 1.0, 3).astype(np.float32)
    m[b: b + 3, 0] = rng.uniform(-0.2, 0.2, 3) * (zb + 6.0) * tx
    m[b: b + 3, 1] = rng.uniform(-0.2, 0.2, 3) * (zb + 6.0) * ty
    m[b: b + 3, 2] = zb
    s[b: b + 3] = np.float32(0.45 * (zb + 6.0) * tx)[:, None] * np.ones((1, 3), np.float32)     # sigma = 0.45 W / 2 pixels in x
    o[b: b + 3, 0] = np.float32(0.3)
    view = cam["world_view_transform"].astype(np.float32)
    pv = np.concatenate([m.astype(np.float64) + np.array([0.0, 0.0, 6.0]), np.ones((n, 1))], 1)
    sc["means"] = (pv @ np.linalg.inv(view.astype(np.float64)))[:, :3].astype(np.float32)
    sc["view"], sc["proj"] = view, cam["full_proj_transform"].astype(np.float32)
    sc["campos"] = cam["camera_center"].astype(np.float32)
    return sc


CAMERA_SEED = 17        # the forward scenes under the fixture cameras; chosen on the CPU for blend_margin (tests/test_raster_ref_cpu.py)


def blend_margin(ix, iy, A, B, C, opacities, radii, W, H):
    """min |255 alpha - 1| over every (pixel, visible Gaussian) with power <= 0: how far the scene stays from the 1 / 255 blend threshold.
    Two fp32 forwards in the same operation order differ in alpha by their expf alone, 1.5 ulp = 1.8e-7 relative between them; a scene
    with a pair nearer the threshold than that may blend it on one side only, a step of up to 1 / 255 in a pixel that no tolerance on
    the image covers."""
    vis = torch.as_tensor(radii).reshape(-1) > 0
    ix, iy, A, B, C, op = ix[vis], iy[vis], A[vis], B[vis], C[vis], opacities.double().reshape(-1)[vis]
    dx = ix[None, :] - torch.arange(W, dtype=torch.float64)[:, None]
    best = float("inf")
    for y in range(H):
        dy = (iy - y)[None, :]
        power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
        m = (255.0 * op * torch.exp(power) - 1.0).abs()[power <= 0]
        best = min(best, float(m.min()))
    return best
