"""CPU checks of the float64 rasteriser restatement (tests/raster_ref.py) that the GPU backward is measured against: its image is the
oracle's, and its autograd gradients are the true ones (gradcheck with the discrete decisions frozen)."""
import numpy as np
import pytest
import torch

from tests import raster_ref as rr


@pytest.mark.parametrize("n,W,H", [(50, 33, 17), (400, 64, 48), (1500, 96, 64)])
def test_reference_image_matches_oracle(orc, n, W, H):
    sc = rr.scene(n, n, W, H)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    ref, radii, _ = orc.raster_forward(bg, W, H, sc["means"], sc["colors"], sc["opac"], sc["scales"], 1.0, sc["rots"], sc["view"], sc["proj"], sc["tx"], sc["ty"])
    t = rr.tensors(sc, "cpu")
    img, _ = rr.render(t["means"], t["opac"], t["colors"], t["scales"], t["rots"], None, 1.0, t["view"], t["proj"], sc["tx"], sc["ty"], W, H, bg, radii)
    assert (radii > 0).sum() > n // 3
    assert np.abs(img.numpy() - ref).max() < 1e-5


def test_reference_image_matches_oracle_training_scene(orc):
    W, H = 80, 56
    sc = rr.training_scene(600, 5, W, H, cluster=300)
    bg = np.array([0.3, 0.1, 0.0], np.float32)
    ref, radii, _ = orc.raster_forward(bg, W, H, sc["means"], sc["colors"], sc["opac"], sc["scales"], 1.0, sc["rots"], sc["view"], sc["proj"], sc["tx"], sc["ty"])
    t = rr.tensors(sc, "cpu")
    img, dec = rr.render(t["means"], t["opac"], t["colors"], t["scales"], t["rots"], None, 1.0, t["view"], t["proj"], sc["tx"], sc["ty"], W, H, bg, radii)
    assert np.abs(img.numpy() - ref).max() < 1e-5
    assert max(d.shape[1] for d in dec.values()) > 256          # a list longer than two LDS batches of k_render_backward


@pytest.mark.parametrize("use_cov", [False, True])
def test_reference_gradcheck_frozen_decisions(use_cov):
    W, H, n = 16, 16, 6
    rng = np.random.RandomState(3)
    sc = rr.scene(n, 11, W, H)
    sc["means"][:] = np.c_[rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), rng.uniform(-1, 1, n)].astype(np.float32)
    sc["scales"][:] = np.exp(rng.randn(n, 3) * 0.3 - 1.5).astype(np.float32)
    sc["opac"][:] = rng.uniform(0.2, 0.8, (n, 1)).astype(np.float32)
    t = {k: v.double() for k, v in rr.tensors(sc, "cpu").items()}
    bg = torch.tensor([0.2, 0.1, 0.3], dtype=torch.float64)
    radii = torch.full((n,), 40, dtype=torch.int32)         # every Gaussian in the one tile
    R = torch.tensor(np.random.RandomState(0).randn(3, H, W))
    cov = None
    if use_cov:
        with torch.no_grad():
            s = 1.3 * t["scales"]
            q = t["rots"]
            r, x, y, z = q.unbind(1)
            Rm = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                              torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                              torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
            S = Rm @ torch.diag_embed(s * s) @ Rm.transpose(1, 2)
            cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    args = dict(view=t["view"], proj=t["proj"], tanfx=sc["tx"], tanfy=sc["ty"], W=W, H=H, bg=bg, radii=radii)
    _, keep = rr.render(t["means"], t["opac"], t["colors"], t["scales"], t["rots"], cov, 1.3, **args)
    assert sum(int(k.sum()) for k in keep.values()) > 0

    if use_cov:
        def f(m, o, c, cv):
            return (rr.render(m, o, c, None, None, cv, 1.3, keep=keep, **args)[0] * R).sum()
        inputs = (t["means"], t["opac"], t["colors"], cov)
    else:
        def f(m, o, c, s, q):
            return (rr.render(m, o, c, s, q, None, 1.3, keep=keep, **args)[0] * R).sum()
        inputs = (t["means"], t["opac"], t["colors"], t["scales"], t["rots"])
    inputs = tuple(x.clone().requires_grad_(True) for x in inputs)
    assert torch.autograd.gradcheck(f, inputs, eps=1e-6, atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ cameras made by the reference's Python
CAMS = rr.cameras()
ROTATED = [c for c in rr.CAMERAS if c != "identity"]
# (n, W, H, cluster, seed): the scenes of the GPU tests under the fixture cameras -- test_gpu_rasterizer.py's two forward shapes and
# test_gpu_raster_backward.py's two gradient cases
CASES = [(3000, 200, 120, 0, rr.CAMERA_SEED), (50, 33, 17, 0, rr.CAMERA_SEED), (1200, 83, 45, 300, 3), (1200, 83, 45, 300, 4)]


def _project_args(sc, W, H, t=None):
    t = t or rr.tensors(sc, "cpu")
    return (t["means"], t["scales"], t["rots"], None, 1.0, t["view"], t["proj"], sc["tx"], sc["ty"], W, H)


def test_identity_fixture_is_the_scene_camera():
    """The reference's functions give the matrices every earlier test wrote out by hand (float32: a rounding apart at most)."""
    sc = rr.scene(10, 0, 200, 120)
    cam = CAMS["identity"]
    assert np.array_equal(cam["world_view_transform"], sc["view"])
    assert np.allclose(cam["full_proj_transform"], sc["proj"], rtol=3e-7, atol=1e-9)
    assert abs(cam["tanfovx"] - sc["tx"]) < 1e-15 and abs(cam["tanfovy"] - sc["ty"]) < 1e-15
    assert np.array_equal(cam["camera_center"], np.array([0.0, 0.0, -6.0], np.float32))


@pytest.mark.parametrize("name", ROTATED)
def test_fixture_cameras_are_what_they_claim(name):
    cam = CAMS[name]
    Wm = cam["world_view_transform"][:3, :3].astype(np.float64)
    assert np.abs(Wm @ Wm.T - np.eye(3)).max() < 1e-6
    assert np.abs(Wm - Wm.T).max() > 0.3 and np.abs(Wm - np.eye(3)).max() > 0.3    # a transposed read moves it, and so does none at all
    if name == "yaw90":
        assert np.array_equal(np.abs(Wm), np.array([[0.0, 0, 1], [0, 1, 0], [1, 0, 0]])) and Wm[0, 2] == -Wm[2, 0]
    if name == "general_anisotropic":
        assert cam["tanfovx"] < cam["tanfovy"]
        for W, H in ((200, 120), (33, 17), (83, 45)):
            fx, fy = W / (2 * cam["tanfovx"]), H / (2 * cam["tanfovy"])
            assert abs(fx / fy - 1) >= 0.2
    # camera_center is the point the view matrix sends to the origin
    c = np.append(cam["camera_center"].astype(np.float64), 1.0) @ cam["world_view_transform"].astype(np.float64)
    assert np.abs(c[:3]).max() < 1e-5


@pytest.mark.parametrize("name", rr.CAMERAS)
@pytest.mark.parametrize("n,W,H,cluster,seed", CASES)
def test_projections_agree(name, n, W, H, cluster, seed):
    """project (flat indices, as the kernel and the oracle read the matrices) against project_matrix_form (none): 1e-9 relative."""
    sc = rr.scene_for_camera(CAMS[name], n, seed, W, H, cluster=cluster)
    a, b = rr.project(*_project_args(sc, W, H)), rr.project_matrix_form(*_project_args(sc, W, H))
    front = a[5] > 0.2
    assert 0 < int(front.sum()) < n
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = x[front], y[front]
        assert float((x - y).abs().max()) <= 1e-9 * float(y.abs().max()), (k, float((x - y).abs().max()))


@pytest.fixture(scope="module")
def camera_frames(orc):
    """Per (camera, shape): the scene, the oracle's image / radii / list length, computed once."""
    cache = {}

    def get(name, n, W, H, cluster, seed):
        key = (name, n, W, H, cluster, seed)
        if key not in cache:
            sc = rr.scene_for_camera(CAMS[name], n, seed, W, H, cluster=cluster)
            bg = np.array([0.1, 0.2, 0.3], np.float32)
            cache[key] = (sc, bg) + orc.raster_forward(bg, W, H, sc["means"], sc["colors"], sc["opac"], sc["scales"], 1.0, sc["rots"], sc["view"],
                                                       sc["proj"], sc["tx"], sc["ty"])
        return cache[key]
    return get


@pytest.mark.parametrize("name", rr.CAMERAS)
@pytest.mark.parametrize("n,W,H,cluster,seed", CASES)
def test_reference_image_matches_oracle_cameras(camera_frames, name, n, W, H, cluster, seed):
    """The float64 image through the index-free projection is the oracle's, and the scene is no quiet one: what the GPU tests under this
    camera rely on is there -- visible and hidden Gaussians, both clamps, a list longer than two LDS batches, a square of more than 64 tiles.

    At 200 x 120 the image is not compared: among the 6e7 (pixel, Gaussian) pairs of 3000 Gaussians some come within the oracle's own
    fp32 rounding of the 1 / 255 threshold whatever the seed, and the float64 image then differs from the oracle's by that Gaussian
    in that pixel (1e-3, measured under `general_anisotropic`, seed 3000: two pixels, |255 alpha - 1| = 3e-6 in each).  The GPU test at
    that shape compares two fp32 forwards of one operation order, which differ by expf alone: asserted here instead is that the scene
    keeps 1e-6 from the threshold, five times what two expf can differ by (raster_ref.blend_margin)."""
    sc, bg, ref, radii, _ = camera_frames(name, n, W, H, cluster, seed)
    t = rr.tensors(sc, "cpu")
    vis = torch.as_tensor(radii > 0)
    assert n // 3 < int(vis.sum()) < n
    ix, iy, A, B, C, tz = rr.project_matrix_form(*_project_args(sc, W, H, t))
    assert int((tz <= 0.2).sum()) > 0                                               # some behind the camera
    if (W, H) == (200, 120):
        rx0, ry0, rx1, ry1 = rr.tile_rects(ix, iy, radii, W, H)
        assert int((vis & ((rx1 - rx0) * (ry1 - ry0) > 64)).sum()) > 0              # k_duplicate_sorted's REC_BIG record
        assert rr.blend_margin(ix, iy, A, B, C, t["opac"], radii, W, H) >= 1e-6
    else:
        img, dec = rr.render(t["means"], t["opac"], t["colors"], t["scales"], t["rots"], None, 1.0, t["view"], t["proj"], sc["tx"], sc["ty"], W, H,
                             bg, radii, project=rr.project_matrix_form)
        assert np.abs(img.numpy() - ref).max() < 1e-5
        if cluster:
            assert max(d.shape[1] for d in dec.values()) > 256
    if n == 50:
        return
    pv = (torch.cat([t["means"].double(), torch.ones(n, 1, dtype=torch.float64)], 1) @ t["view"].double())[:, :3]
    assert int((vis & ((pv[:, 0] / pv[:, 2]).abs() > 1.3 * sc["tx"])).sum()) > 0    # clamped in x and on the image
    assert int((vis & ((pv[:, 1] / pv[:, 2]).abs() > 1.3 * sc["ty"])).sum()) > 0    # clamped in y and on the image


def _gradcheck_scene(cam):
    W, H, n = 16, 16, 6
    rng = np.random.RandomState(3)
    sc = rr.scene(n, 11, W, H)
    sc["tx"], sc["ty"] = float(cam["tanfovx"]), float(cam["tanfovy"])
    view = cam["world_view_transform"].astype(np.float64)
    pv = np.c_[rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), rng.uniform(-1, 1, n) + 6.0, np.ones(n)]
    sc["means"][:] = (pv @ np.linalg.inv(view))[:, :3].astype(np.float32)
    sc["scales"][:] = np.exp(rng.randn(n, 3) * 0.3 - 1.5).astype(np.float32)
    sc["opac"][:] = rng.uniform(0.2, 0.8, (n, 1)).astype(np.float32)
    sc["view"], sc["proj"] = cam["world_view_transform"], cam["full_proj_transform"]
    return sc, W, H, n


@pytest.mark.parametrize("use_cov", [False, True])
@pytest.mark.parametrize("form", ["project", "project_matrix_form"])
def test_reference_gradcheck_frozen_decisions_anisotropic(use_cov, form):
    """test_reference_gradcheck_frozen_decisions under the rotated camera with unequal focal lengths, through either projection."""
    sc, W, H, n = _gradcheck_scene(CAMS["general_anisotropic"])
    t = {k: v.double() for k, v in rr.tensors(sc, "cpu").items()}
    bg = torch.tensor([0.2, 0.1, 0.3], dtype=torch.float64)
    radii = torch.full((n,), 40, dtype=torch.int32)
    R = torch.tensor(np.random.RandomState(0).randn(3, H, W))
    cov = None
    if use_cov:
        with torch.no_grad():
            S = rr._sigma(t["scales"], t["rots"], None, 1.3)
            cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    args = dict(view=t["view"], proj=t["proj"], tanfx=sc["tx"], tanfy=sc["ty"], W=W, H=H, bg=bg, radii=radii, project=getattr(rr, form))
    _, keep = rr.render(t["means"], t["opac"], t["colors"], t["scales"], t["rots"], cov, 1.3, **args)
    assert sum(int(k.sum()) for k in keep.values()) > 100                   # (pixel, Gaussian) pairs that blend

    if use_cov:
        def f(m, o, c, cv):
            return (rr.render(m, o, c, None, None, cv, 1.3, keep=keep, **args)[0] * R).sum()
        inputs = (t["means"], t["opac"], t["colors"], cov)
    else:
        def f(m, o, c, s, q):
            return (rr.render(m, o, c, s, q, None, 1.3, keep=keep, **args)[0] * R).sum()
        inputs = (t["means"], t["opac"], t["colors"], t["scales"], t["rots"])
    inputs = tuple(x.clone().requires_grad_(True) for x in inputs)
    assert torch.autograd.gradcheck(f, inputs, eps=1e-6, atol=1e-6, rtol=1e-5)


def _focal(name, W, H):
    return W / (2 * CAMS[name]["tanfovx"]), H / (2 * CAMS[name]["tanfovy"])


# focal_y := focal_x is a mutation only where the two differ (by a fifth or more: every rotated camera but yaw90 at 83 x 45)
MUTANT_CASES = [(c, m) for c in ROTATED for m in rr.MUTANTS
                if m != "focal_y_is_focal_x" or abs(_focal(c, CASES[2][1], CASES[2][2])[0] / _focal(c, CASES[2][1], CASES[2][2])[1] - 1) >= 0.2]


@pytest.mark.parametrize("name,mutant", MUTANT_CASES)
def test_mutants_fail_the_gpu_comparisons(camera_frames, name, mutant):
    """Each wrong reading of the matrices, put into the index-free projection, misses what the GPU tests assert of the device against the
    right one: the image within 1e-4 and every gradient within 1e-4 norm-relative (tests/test_gpu_raster_backward.py), and the oracle's
    image within 2e-5 (tests/test_gpu_rasterizer.py).  So a kernel with that error cannot pass them."""
    n, W, H, cluster, seed = CASES[2]
    sc, bg, ref, radii, _ = camera_frames(name, n, W, H, cluster, seed)
    R = torch.tensor(np.random.RandomState(3).randn(3, H, W))
    out = {}
    for tag, proj in (("good", rr.project_matrix_form), ("bad", rr.mutant_projection(mutant))):
        t = {k: v.double().requires_grad_(k in ("means", "scales", "rots", "opac", "colors")) for k, v in rr.tensors(sc, "cpu").items()}
        img, _ = rr.render(t["means"], t["opac"], t["colors"], t["scales"], t["rots"], None, 1.0, t["view"], t["proj"], sc["tx"], sc["ty"], W, H, bg,
                           radii, project=proj)
        (torch.nan_to_num(img) * R).sum().backward()
        out[tag] = (img.detach().numpy(), {k: t[k].grad for k in ("means", "scales", "rots", "opac", "colors")})
    assert np.abs(out["good"][0] - ref).max() < 1e-5
    assert not np.abs(np.nan_to_num(out["bad"][0]) - ref).max() < 1e-4
    for k, g in out["good"][1].items():
        b = torch.nan_to_num(out["bad"][1][k])
        assert not float((b - g).norm() / g.norm()) <= 1e-4, k
