"""GPU parity of the rasteriser forward / visible_filter against the oracle.
Tolerances: radii exact (identical fp32 op order, correctly rounded sqrt / div on both sides); pixels
differ only through expf (ocml vs glibc) -> max abs 2e-5, and PSNR against a common target within
0.01 dB (the north star's tolerance)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _scene(n, seed, W, H):
    rng = np.random.RandomState(seed)
    means = (rng.rand(n, 3).astype(np.float32) - 0.5) * np.array([6, 4, 6], np.float32)
    means[: n // 20, 2] -= 9.0   # some behind the camera
    scales = np.exp(rng.randn(n, 3).astype(np.float32) * 0.5 - 2.5)
    q = rng.randn(n, 4).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    opac = (1 / (1 + np.exp(-rng.randn(n, 1).astype(np.float32) * 2)))
    colors = rng.rand(n, 3).astype(np.float32)
    # camera at z = -6 looking down +z: world -> view is a translation; matrices stored transposed (cameras.py:48-57)
    Rt = np.eye(4, dtype=np.float32); Rt[2, 3] = 6.0
    fovx = 1.0; fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
    znear, zfar = 0.01, 100.0
    tx, ty = math.tan(fovx / 2), math.tan(fovy / 2)
    Pm = np.zeros((4, 4), np.float32)
    Pm[0, 0] = 1 / tx; Pm[1, 1] = 1 / ty; Pm[3, 2] = 1.0; Pm[2, 2] = zfar / (zfar - znear); Pm[2, 3] = -(zfar * znear) / (zfar - znear)
    view = Rt.T.copy()
    full = (view @ Pm.T).astype(np.float32)
    return dict(means=means, scales=scales, rots=q, opac=opac, colors=colors, view=view, proj=full, tx=tx, ty=ty)


def _settings(torch, sc, W, H, bg):
    from gauspcc_amd.rasterizer import GaussianRasterizationSettings

    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=sc["tx"], tanfovy=sc["ty"], bg=torch.tensor(bg).cuda(), scale_modifier=1.0,
                                         viewmatrix=torch.tensor(sc["view"]).cuda(), projmatrix=torch.tensor(sc["proj"]).cuda(), sh_degree=1,
                                         campos=torch.tensor(sc.get("campos", [0.0, 0.0, -6.0])).cuda(), prefiltered=False, debug=False)


def _check_forward(orc, sc, n, W, H):
    import torch

    from gauspcc_amd.rasterizer import GaussianRasterizer, psnr

    bg = np.array([0.1, 0.2, 0.3], np.float32)
    rast = GaussianRasterizer(_settings(torch, sc, W, H, bg))
    t = {k: torch.tensor(v).cuda() for k, v in sc.items() if isinstance(v, np.ndarray)}
    img, radii = rast(means3D=t["means"], means2D=torch.zeros_like(t["means"]), shs=None, colors_precomp=t["colors"], opacities=t["opac"],
                      scales=t["scales"], rotations=t["rots"], cov3D_precomp=None)
    ref, rradii, L = orc.raster_forward(bg, W, H, sc["means"], sc["colors"], sc["opac"], sc["scales"], 1.0, sc["rots"], sc["view"], sc["proj"], sc["tx"], sc["ty"])
    assert img.shape == (3, H, W) and radii.dtype == torch.int32
    assert np.array_equal(radii.cpu().numpy(), rradii)
    assert rast.num_rendered == L and (rradii > 0).sum() > n // 3
    d = np.abs(img.cpu().numpy() - ref)
    print(f"forward {n} {W}x{H}: {int((rradii > 0).sum())} visible, {L} pairs, max |image - oracle| {d.max():.3e}")
    assert d.max() < 2e-5, d.max()
    target = torch.tensor(np.clip(ref + np.random.RandomState(1).randn(*ref.shape).astype(np.float32) * 0.05, 0, 1)).cuda()
    p_dev = psnr(img.clamp(0, 1), target).mean().item()
    p_ref = psnr(torch.tensor(ref).cuda().clamp(0, 1), target).mean().item()
    assert abs(p_dev - p_ref) < 0.01


@pytest.mark.parametrize("n,W,H", [(3000, 200, 120), (50, 33, 17), (20000, 320, 240)])
def test_forward_matches_oracle(orc, n, W, H):
    _check_forward(orc, _scene(n, n, W, H), n, W, H)


CAMERA_NAMES = ("identity", "yaw90", "general", "general_anisotropic", "translated_scaled")      # tests/golden/cameras.npz (raster_ref.CAMERAS)


@pytest.mark.parametrize("n,W,H", [(3000, 200, 120), (50, 33, 17)])
@pytest.mark.parametrize("camera", CAMERA_NAMES)
def test_forward_matches_oracle_cameras(orc, camera, n, W, H):
    """test_forward_matches_oracle under the cameras the reference's own getWorld2View2 / getProjectionMatrix made
    (tests/golden/make_cameras.py): rotations, unequal focal lengths, tan(FoVx / 2) < tan(FoVy / 2), the scene normalisation's translate
    and scale.  33 x 17: partial tiles both ways; 200 x 120: 13 x 8 tiles, with squares of more than 64 (tests/test_raster_ref_cpu.py
    asserts what each scene holds)."""
    from tests import raster_ref as rr

    _check_forward(orc, rr.scene_for_camera(rr.cameras()[camera], n, rr.CAMERA_SEED, W, H), n, W, H)


def _check_visible_filter(orc, sc, n, W, H):
    import torch

    from gauspcc_amd.rasterizer import GaussianRasterizer

    rast = GaussianRasterizer(_settings(torch, sc, W, H, np.zeros(3, np.float32)))
    t = {k: torch.tensor(v).cuda() for k, v in sc.items() if isinstance(v, np.ndarray)}
    scales6 = torch.cat([t["scales"], t["scales"]], 1)     # the reference passes scales[:, :3] of a wider tensor (non-contiguous view)
    radii = rast.visible_filter(means3D=t["means"], scales=scales6[:, :3], rotations=t["rots"], cov3D_precomp=None)
    _, rradii, _ = orc.raster_forward(np.zeros(3, np.float32), W, H, sc["means"], None, None, sc["scales"], 1.0, sc["rots"], sc["view"], sc["proj"], sc["tx"], sc["ty"])
    assert np.array_equal(radii.cpu().numpy(), rradii)
    assert 0 < (rradii > 0).sum() < n


def test_visible_filter_matches_forward_radii(orc):
    _check_visible_filter(orc, _scene(10000, 7, 256, 144), 10000, 256, 144)


@pytest.mark.parametrize("camera", CAMERA_NAMES)
def test_visible_filter_matches_forward_radii_cameras(orc, camera):
    from tests import raster_ref as rr

    n, W, H = 3000, 200, 120
    _check_visible_filter(orc, rr.scene_for_camera(rr.cameras()[camera], n, rr.CAMERA_SEED, W, H), n, W, H)


def test_chain_under_rotated_camera(orc):
    """visible_filter -> generate_neural_gaussians -> GaussianRasterizer, as tests/test_gpu_rd_loop.py chains them for its axis-aligned
    camera, under `general_anisotropic` of tests/golden/cameras.npz: the view matrix, the projection and the camera centre (the reference's
    world_view_transform.inverse()[3, :3], HAC/scene/cameras.py:57) name one camera all along the chain."""
    import types

    import torch

    from gauspcc_amd.neural_gaussians import generate_neural_gaussians
    from gauspcc_amd.rasterizer import GaussianRasterizer, psnr
    from gauspcc_amd.synth import SyntheticGaussianModel
    from tests import raster_ref as rr

    W, H = 200, 120
    cam = rr.cameras()["general_anisotropic"]
    sc = dict(view=cam["world_view_transform"], proj=cam["full_proj_transform"], tx=float(cam["tanfovx"]), ty=float(cam["tanfovy"]),
              campos=cam["camera_center"])
    bg = np.array([0.05, 0.1, 0.15], np.float32)
    rast = GaussianRasterizer(_settings(torch, sc, W, H, bg))
    pc = SyntheticGaussianModel(20_000, seed=3)
    anchors = pc.get_anchor
    n = anchors.shape[0]
    # the centre and the view matrix agree: a rigid transform keeps every anchor's distance to the camera
    pv = torch.cat([anchors.cpu().double(), torch.ones(n, 1, dtype=torch.float64)], 1) @ torch.tensor(sc["view"]).double()
    dist = (anchors.cpu().double() - torch.tensor(sc["campos"]).double()).norm(dim=1)
    assert float((pv[:, :3].norm(dim=1) - dist).abs().max()) < 1e-5 and float(pv[:, 2].min()) > 0.2
    rot_id = torch.zeros(n, 4, device="cuda"); rot_id[:, 0] = 1.0
    with torch.no_grad():
        radii_pure = rast.visible_filter(means3D=anchors, scales=pc.get_scaling[:, :3], rotations=rot_id, cov3D_precomp=None)
        _, rpure, _ = orc.raster_forward(bg, W, H, anchors.cpu().numpy(), None, None, pc.get_scaling[:, :3].cpu().numpy(), 1.0, rot_id.cpu().numpy(),
                                         sc["view"], sc["proj"], sc["tx"], sc["ty"])
        assert np.array_equal(radii_pure.cpu().numpy(), rpure)
        visible = radii_pure > 0
        assert int(visible.sum()) > n // 2
        xyz, color, opacity, scaling, rot, _ = generate_neural_gaussians(types.SimpleNamespace(camera_center=torch.tensor(sc["campos"]).cuda()), pc, visible)
        img, radii = rast(means3D=xyz, means2D=torch.zeros_like(xyz), shs=None, colors_precomp=color, opacities=opacity, scales=scaling,
                          rotations=rot, cov3D_precomp=None)
    ref, rradii, L = orc.raster_forward(bg, W, H, xyz.cpu().numpy(), color.cpu().numpy(), opacity.cpu().numpy(), scaling.cpu().numpy(), 1.0,
                                        rot.cpu().numpy(), sc["view"], sc["proj"], sc["tx"], sc["ty"])
    assert xyz.shape[0] > n and int((rradii > 0).sum()) > xyz.shape[0] // 2
    assert np.array_equal(radii.cpu().numpy(), rradii)
    assert rast.num_rendered == L
    d = np.abs(img.cpu().numpy() - ref)
    target = torch.tensor(np.clip(ref + np.random.RandomState(1).randn(*ref.shape).astype(np.float32) * 0.05, 0, 1)).cuda()
    p_dev = psnr(img.clamp(0, 1), target).mean().item()
    p_ref = psnr(torch.tensor(ref).cuda().clamp(0, 1), target).mean().item()
    print(f"chain: {int(visible.sum())} of {n} anchors, {xyz.shape[0]} Gaussians, {L} pairs, max |image - oracle| {d.max():.3e}, PSNR {p_dev:.4f} / {p_ref:.4f}")
    assert abs(p_dev - p_ref) < 0.01


def test_empty_and_background():
    import torch

    from gauspcc_amd.rasterizer import GaussianRasterizer

    W, H = 40, 24
    sc = _scene(8, 3, W, H)
    sc["means"][:, 2] = -50.0   # everything behind the camera
    bg = np.array([0.25, 0.5, 0.75], np.float32)
    rast = GaussianRasterizer(_settings(torch, sc, W, H, bg))
    t = {k: torch.tensor(v).cuda() for k, v in sc.items() if isinstance(v, np.ndarray)}
    img, radii = rast(means3D=t["means"], means2D=None, shs=None, colors_precomp=t["colors"], opacities=t["opac"], scales=t["scales"], rotations=t["rots"])
    assert int(radii.sum()) == 0
    assert torch.allclose(img, torch.tensor(bg).cuda().view(3, 1, 1).expand(3, H, W))


@pytest.mark.parametrize("boost", [0.0, 1.2])
def test_two_level_sort_equals_combined_key_sort(boost):
    """The (tile | depth) order through a depth sort of the Gaussians + a tile sort of the duplicates (csrc/rasterizer.hip, round 5) against
    the reference's single sort of the combined key (GAUSPCC_RASTER_SORT2=0, developer knob): the same image bit for bit, on a scene where a
    third of the Gaussians share their depth with others (equal keys: the stable order by Gaussian index decides).  boost 1.2: splats of ~50 pixels
    radius, their bounding squares on either side of 64 tiles -- both forms of k_duplicate_sorted's record (tile mask / REC_BIG walk)."""
    import hashlib
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    snippet = r"""
import sys, hashlib
import numpy as np
sys.path.insert(0, %r)
import torch
from tests.test_gpu_rasterizer import _scene, _settings
from gauspcc_amd.rasterizer import GaussianRasterizer
W, H, n = 400, 300, 60000
sc = _scene(n, 11, W, H)
sc["means"][::3, 2] = np.float32(0.5)          # shared depth
sc["means"][1::7, 2] = np.float32(-1.25)
sc["scales"] *= np.float32(np.exp(%r))
rast = GaussianRasterizer(_settings(torch, sc, W, H, np.array([0.1, 0.2, 0.3], np.float32)))
t = {k: torch.tensor(v).cuda() for k, v in sc.items() if isinstance(v, np.ndarray)}
img, radii = rast(means3D=t["means"], means2D=None, shs=None, colors_precomp=t["colors"], opacities=t["opac"], scales=t["scales"], rotations=t["rots"])
print("digest", hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest(), int((radii > 64).sum()), rast.num_rendered)
""" % (root, boost)
    out = []
    for v, cull in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        e = dict(os.environ)
        e["GAUSPCC_DEV"] = "1"
        e["GAUSPCC_RASTER_SORT2"] = v
        e["GAUSPCC_RASTER_CULL"] = cull      # exact tile culling (csrc/rasterizer.hip: tile_touches): shorter lists, the same image, the reference's num_rendered
        r = subprocess.run([sys.executable, "-c", snippet], env=e, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out.append([ln for ln in r.stdout.splitlines() if ln.startswith("digest")][0])
    assert out[0] == out[1] == out[2] == out[3] and int(out[0].split()[-1]) > 100000
    assert boost == 0.0 or int(out[0].split()[-2]) > 1000       # squares wider than 8 tiles are there


def test_needle_splats_survive_exact_culling():
    """ADVICE (round 5): long thin splats far from their centre -- sigma of a few hundred pixels along one axis, a fraction of a pixel across --
    make the three terms of q = 0.5 A dx^2 + B dx dy + 0.5 C dy^2 ~1e6 each while q sits near the 1 / 255 threshold (~5): the fp32 edge minimum
    of the tile test and k_render's per-pixel power then differ by far more than the old absolute margin, and a tile could be culled although
    one of its pixels passes the blend test.  With the margin scaled by the magnitude of the terms the image is the same with and without
    culling (GAUSPCC_RASTER_CULL, developer knob), bit for bit.  Contract: HAC/gaussian_renderer/__init__.py:199-225."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    snippet = r"""
import sys, hashlib
import numpy as np
sys.path.insert(0, %r)
import torch
from tests.test_gpu_rasterizer import _scene, _settings
from gauspcc_amd.rasterizer import GaussianRasterizer
W, H, n = 1600, 1060, 4000
sc = _scene(n, 23, W, H)
rng = np.random.RandomState(5)
sc["scales"][:, 0] = np.exp(rng.rand(n).astype(np.float32) * 1.5 + 0.2)      # 1.2 .. 5.5 world units: hundreds to thousands of pixels
sc["scales"][:, 1:] = np.exp(rng.rand(n, 2).astype(np.float32) * 1.0 - 7.0)   # ~1e-3 world units: well under a pixel
sc["opac"][:] = np.float32(0.9)
sc["means"][:, 2] = np.abs(sc["means"][:, 2])                                  # all in front of the camera
rast = GaussianRasterizer(_settings(torch, sc, W, H, np.array([0.0, 0.0, 0.0], np.float32)))
t = {k: torch.tensor(v).cuda() for k, v in sc.items() if isinstance(v, np.ndarray)}
img, radii = rast(means3D=t["means"], means2D=None, shs=None, colors_precomp=t["colors"], opacities=t["opac"], scales=t["scales"], rotations=t["rots"])
assert bool(torch.isfinite(img).all()) and float(img.max()) > 0.05
print("digest", hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest(), int((radii > 200).sum()), rast.num_rendered)
""" % root
    out = []
    for cull in ("1", "0"):
        e = dict(os.environ)
        e["GAUSPCC_DEV"] = "1"
        e["GAUSPCC_RASTER_CULL"] = cull
        r = subprocess.run([sys.executable, "-c", snippet], env=e, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out.append([ln for ln in r.stdout.splitlines() if ln.startswith("digest")][0].split())
    assert out[0][1] == out[1][1], "the image changed with exact tile culling"
    assert int(out[0][2]) > 500                    # the scene really is needles: radii of hundreds of pixels
