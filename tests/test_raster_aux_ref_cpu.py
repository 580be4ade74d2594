"""CPU checks of the float64 restatement of the rasteriser's depth and opacity maps (tests/raster_aux_ref.py), the yardstick of
tests/test_gpu_raster_aux.py: its image is raster_ref.render's, its maps are the sums they claim to be, their autograd gradients are the
true ones (gradcheck with the decisions frozen), and wall_scene keeps clear of the stop threshold.  And extras= is validated without a device."""
import numpy as np
import pytest
import torch

from tests import raster_aux_ref as ra
from tests import raster_ref as rr

SCENES = [(300, 48, 32, 1, 1.0, 0), (1200, 83, 45, 3, 1.25, 300)]


@pytest.mark.parametrize("n,W,H,seed,sm,cluster", SCENES)
def test_maps_are_the_sums_they_claim(orc, n, W, H, seed, sm, cluster):
    sc = rr.training_scene(n, seed, W, H, cluster=cluster)
    bg = np.array([0.2, 0.4, 0.1], np.float32)
    ref, radii, _ = orc.raster_forward(bg, W, H, sc["means"], sc["colors"], sc["opac"], sc["scales"], sm, sc["rots"], sc["view"], sc["proj"], sc["tx"], sc["ty"])
    t = rr.tensors(sc, "cpu")
    args = (t["scales"], t["rots"], None, sm, t["view"], t["proj"], sc["tx"], sc["ty"], W, H)
    img0, dec0 = rr.render(t["means"], t["opac"], t["colors"], *args, bg, radii)
    img, inv, alp, dec = ra.render_aux(t["means"], t["opac"], t["colors"], *args, bg, radii)
    assert torch.equal(img, img0)                                   # the same operations: bit for bit
    assert dec.keys() == dec0.keys() and all(torch.equal(dec[k], dec0[k]) for k in dec)
    d_orc = np.abs(img.numpy() - ref).max()
    print(f"aux reference {n} {W}x{H}: max |image - oracle| {d_orc:.3e}")
    assert d_orc < 1e-5
    assert inv.shape == (1, H, W) and alp.shape == (1, H, W)
    zero = np.zeros(3, np.float32)
    wsum = ra.render_aux(t["means"], t["opac"], torch.ones_like(t["colors"]), *args, zero, radii)[0]      # colour 1, no background: sum_i w_i
    assert float((alp - wsum[:1]).abs().max()) <= 1e-12
    csum = ra.render_aux(t["means"], t["opac"], t["colors"], *args, zero, radii)[0]                       # sum_i w_i c_i
    assert float((img - (1 - alp) * torch.tensor(bg).double()[:, None, None] - csum).abs().max()) <= 1e-12
    tz = rr.project(t["means"], *args)[5]
    vis = torch.as_tensor(radii > 0)
    assert 0 < int(vis.sum()) < n
    assert bool((inv <= alp * (1 / tz[vis]).max()).all())
    assert float(inv.max()) > 0 and float(alp.max()) > 0.9 and float(alp.min()) < 0.5


def _one_tile_scene():
    """The scene of test_raster_ref_cpu.test_reference_gradcheck_frozen_decisions: six Gaussians in one 16 x 16 tile."""
    W, H, n = 16, 16, 6
    rng = np.random.RandomState(3)
    sc = rr.scene(n, 11, W, H)
    sc["means"][:] = np.c_[rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), rng.uniform(-1, 1, n)].astype(np.float32)
    sc["scales"][:] = np.exp(rng.randn(n, 3) * 0.3 - 1.5).astype(np.float32)
    sc["opac"][:] = rng.uniform(0.2, 0.8, (n, 1)).astype(np.float32)
    return sc, W, H, n


@pytest.mark.parametrize("use_cov", [False, True])
@pytest.mark.parametrize("form", ["project", "project_matrix_form"])
def test_maps_gradcheck_frozen_decisions(use_cov, form):
    sc, W, H, n = _one_tile_scene()
    t = {k: v.double() for k, v in rr.tensors(sc, "cpu").items()}
    bg = torch.tensor([0.2, 0.1, 0.3], dtype=torch.float64)
    radii = torch.full((n,), 40, dtype=torch.int32)         # every Gaussian in the one tile
    Rd, Ra = (torch.tensor(np.random.RandomState(s).randn(1, H, W)) for s in (1, 2))
    cov = None
    if use_cov:
        with torch.no_grad():
            S = rr._sigma(t["scales"], t["rots"], None, 1.3)
            cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    args = dict(view=t["view"], proj=t["proj"], tanfx=sc["tx"], tanfy=sc["ty"], W=W, H=H, bg=bg, radii=radii, project=getattr(rr, form))
    keep = ra.render_aux(t["means"], t["opac"], t["colors"], t["scales"], t["rots"], cov, 1.3, **args)[3]
    assert sum(int(k.sum()) for k in keep.values()) > 100                   # (pixel, Gaussian) pairs that blend

    def loss(out):
        return (out[1] * Rd).sum() + (out[2] * Ra).sum()

    if use_cov:
        def f(m, o, cv):
            return loss(ra.render_aux(m, o, t["colors"], None, None, cv, 1.3, keep=keep, **args))
        inputs = (t["means"], t["opac"], cov)
    else:
        def f(m, o, s, q):
            return loss(ra.render_aux(m, o, t["colors"], s, q, None, 1.3, keep=keep, **args))
        inputs = (t["means"], t["opac"], t["scales"], t["rots"])
    inputs = tuple(x.clone().requires_grad_(True) for x in inputs)
    assert torch.autograd.gradcheck(f, inputs, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_wall_scene_meets_its_conditions(orc):
    """Conditions the scene must meet (not tolerances): more than 90 % of the pixels stop early; no (pixel, blended entry) up to the stop
    comes within 1e-4 relative of the 1e-4 threshold -- ten times what an fp32 product of 40 factors can be off by (40 x 6e-8 = 2.4e-6
    for the product, and as much again for the alphas) --, so the device and float64 stop at the same entry; and the 1 / 255 test keeps
    raster_ref.blend_margin's 1e-6."""
    W = H = 32
    sc = ra.wall_scene(ra.WALL_SEED)
    n = len(sc["means"])
    bg = np.zeros(3, np.float32)
    _, radii, _ = orc.raster_forward(bg, W, H, sc["means"], sc["colors"], sc["opac"], sc["scales"], 1.0, sc["rots"], sc["view"], sc["proj"], sc["tx"], sc["ty"])
    assert (radii > 0).all() and 35 <= n <= 45
    t = rr.tensors(sc, "cpu")
    pargs = (t["scales"], t["rots"], None, 1.0, t["view"], t["proj"], sc["tx"], sc["ty"], W, H)
    ix, iy, A, B, C, tz = rr.project(t["means"], *pargs)
    assert bool((tz[1:] >= tz[:-1]).all()) and 3.0 - 1e-6 <= float(tz.min()) and float(tz.max()) <= 9.0 + 1e-6
    assert bool(((ix - W / 2).abs() <= 8.5).all() and ((iy - H / 2).abs() <= 8.5).all())
    share, margin = ra.stop_stats(t["means"], t["opac"], *pargs, radii)
    print(f"wall_scene seed {ra.WALL_SEED}: {100 * share:.1f} % of the pixels stop early, min |T_after / 1e-4 - 1| {margin:.3e}")
    assert share > 0.9
    assert margin >= 1e-4
    assert rr.blend_margin(ix, iy, A, B, C, t["opac"], radii, W, H) >= 1e-6
    alp = ra.render_aux(t["means"], t["opac"], t["colors"], *pargs, bg, radii)[2]
    assert float(alp.min()) > 0.99                                            # a wall: the pixels that do not stop are nearly opaque too


@pytest.mark.parametrize("extras", [("depth",), ("invdepth", "invdepth"), "invdepth", ["alpha"], ("alpha", None)])
def test_extras_are_validated_without_a_device(extras):
    """A bad name, a repeat and a non-tuple raise ValueError before any tensor is touched or any device call made."""
    from gauspcc_amd.rasterizer import GaussianRasterizer

    rast = GaussianRasterizer(raster_settings=None)
    with pytest.raises(ValueError):
        rast(None, None, None, colors_precomp=None, extras=extras)
