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
