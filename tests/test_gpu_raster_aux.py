"""GPU checks of the rasteriser's depth and opacity maps (GaussianRasterizer(..., extras=): gsr_forward_aux, gsr_forward_train_aux +
gsr_backward_aux) against the float64 restatement of tests/raster_aux_ref.py, and of what they must leave alone: the image, the radii and
the colour path's gradients, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import raster_aux_ref as ra
from tests import raster_ref as rr
from tests.test_gpu_raster_backward import _inputs, _settings

pytestmark = pytest.mark.gpu

BOTH = ("invdepth", "alpha")
BG = np.array([0.2, 0.4, 0.1], np.float32)
# name: (n, W, H, seed, use_cov, scale_modifier, cluster, camera)
CASES = {
    "small": (300, 48, 32, 1, False, 1.0, 0, None),
    "partial_tiles_sm": (1200, 83, 45, 3, False, 1.25, 300, None),
    "long_lists": (2000, 96, 64, 2, False, 1.0, 300, None),      # lists longer than two LDS batches
    "cov3D_precomp": (1200, 83, 45, 4, True, 1.0, 300, None),
    "wall": (40, 32, 32, ra.WALL_SEED, False, 1.0, 0, None),     # every pixel's list runs into the stop rule
    "general_camera": (1200, 83, 45, 3, False, 1.25, 300, "general"),
}
FORWARD_CASES = [c for c in CASES if c != "general_camera"]
LOSSES = ("all", "invdepth", "alpha")


def _scene(case):
    n, W, H, seed, use_cov, sm, cluster, camera = CASES[case]
    if case == "wall":
        return ra.wall_scene(seed, n, W, H)
    if camera:
        return rr.scene_for_camera(rr.cameras()[camera], n, seed, W, H, cluster=cluster)
    return rr.training_scene(n, seed, W, H, cluster=cluster)


def _weights(seed, H, W):
    rng = np.random.RandomState(seed)
    return {k: torch.tensor(rng.randn(c, H, W).astype(np.float32)).cuda() for k, c in (("image", 3), ("invdepth", 1), ("alpha", 1))}


def _loss(name, img, inv, alp, Wt):
    if name == "invdepth":
        return (inv * Wt["invdepth"]).sum()
    if name == "alpha":
        return (alp * Wt["alpha"]).sum()
    return (img * Wt["image"]).sum() + (inv * Wt["invdepth"]).sum() + (alp * Wt["alpha"]).sum()


def _device_grads(rast, sc, use_cov, sm, loss, Wt, extras=BOTH):
    inp = _inputs(sc, use_cov, sm)
    out = rast(shs=None, extras=extras, **inp)
    maps = dict(zip(extras, out[2:]))
    _loss(loss, out[0], maps.get("invdepth"), maps.get("alpha"), Wt).backward()
    return out, {k: v.grad for k, v in inp.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _case(case):
    """Per case, computed once and never changed: the scene, the device's maps and radii from the inference path, and the float64
    reference binned with those radii -- its image and maps, and its gradients under the three losses."""
    from gauspcc_amd.rasterizer import GaussianRasterizer

    n, W, H, seed, use_cov, sm, cluster, camera = CASES[case]
    sc = _scene(case)
    rast = GaussianRasterizer(_settings(sc, W, H, BG, sm))
    inp = _inputs(sc, use_cov, sm)
    with torch.no_grad():
        img, radii, inv, alp = rast(shs=None, extras=BOTH, **inp)
    r = radii.cpu()
    ref_in = {k: (None if v is None else v.detach().cpu().double().requires_grad_(True)) for k, v in inp.items()}
    project = rr.project_matrix_form if camera else rr.project
    rimg, rinv, ralp, dec = ra.render_aux(ref_in["means3D"], ref_in["opacities"], ref_in["colors_precomp"], ref_in["scales"], ref_in["rotations"],
                                          ref_in["cov3D_precomp"], sm, torch.tensor(sc["view"]), torch.tensor(sc["proj"]), sc["tx"], sc["ty"], W, H, BG, r,
                                          project=project)
    Wt = _weights(seed, H, W)
    Wc = {k: v.cpu().double() for k, v in Wt.items()}
    keys = [k for k, v in ref_in.items() if v is not None and k != "means2D"]
    ref_grads = {}
    for loss in LOSSES:
        g = torch.autograd.grad(_loss(loss, rimg, rinv, ralp, Wc), [ref_in[k] for k in keys], retain_graph=True, allow_unused=True)
        ref_grads[loss] = {k: (torch.zeros_like(ref_in[k]) if gk is None else gk) for k, gk in zip(keys, g)}
    tz = project(ref_in["means3D"], ref_in["scales"], ref_in["rotations"], ref_in["cov3D_precomp"], sm, torch.tensor(sc["view"]), torch.tensor(sc["proj"]),
                 sc["tx"], sc["ty"], W, H)[5].detach()
    return dict(sc=sc, rast=rast, radii=r, dev=(img.cpu(), inv.cpu(), alp.cpu()), ref=(rimg.detach(), rinv.detach(), ralp.detach()), dec=dec,
                ref_grads=ref_grads, Wt=Wt, max_invz=float((1 / tz[r > 0]).max()))


@pytest.mark.parametrize("case", FORWARD_CASES)
def test_forward_maps_match_float64_reference(case):
    n, W, H, seed, use_cov, sm, cluster, camera = CASES[case]
    c = _case(case)
    if case == "wall":
        assert int((c["radii"] > 0).sum()) == n
    else:
        assert 0 < int((c["radii"] > 0).sum()) < n
    if cluster:
        assert max(d.shape[1] for d in c["dec"].values()) > 256
    dimg, dinv, dalp = (float((d.double() - r).abs().max()) for d, r in zip(c["dev"], c["ref"]))
    print(f"aux forward {case}: max |image - float64| {dimg:.3e}, |alpha - float64| {dalp:.3e}, |invdepth - float64| {dinv:.3e} "
          f"= {dinv / c['max_invz']:.3e} x max(1 / tz) = {c['max_invz']:.4f}")
    assert dimg < 1e-4
    assert dalp < 1e-4
    assert dinv < 1e-4 * c["max_invz"]
    assert float(c["ref"][1].max()) > 0 and float(c["ref"][2].max()) > 0.5


def _frame(kind):
    """colors_precomp: a training scene with partial tiles and a cluster; shs: 64 Gaussians with degree-3 coefficients."""
    from gauspcc_amd.rasterizer import GaussianRasterizer

    if kind == "shs":
        n, W, H = 64, 48, 32
        sc = rr.scene(n, 7, W, H)
        rast = GaussianRasterizer(_settings(sc, W, H, BG)._replace(sh_degree=3))
        inp = _inputs(sc, False, 1.0)
        inp.pop("colors_precomp")
        shs = torch.tensor(np.random.RandomState(8).randn(n, 16, 3).astype(np.float32) * 0.3).cuda().requires_grad_(True)
        return rast, dict(inp, shs=shs, colors_precomp=None), (H, W)
    n, W, H = 1200, 83, 45
    sc = rr.training_scene(n, 3, W, H, cluster=300)
    return GaussianRasterizer(_settings(sc, W, H, BG)), dict(_inputs(sc, False, 1.0), shs=None), (H, W)


@pytest.mark.parametrize("kind", ["colors_precomp", "shs"])
def test_colour_path_untouched(kind):
    rast, inp, (H, W) = _frame(kind)
    img_t, radii_t = rast(**inp)
    nr = rast.num_rendered
    with torch.no_grad():
        img_i, radii_i = rast(**inp)
    assert img_t.grad_fn is not None and img_i.grad_fn is None and torch.equal(img_t.detach(), img_i)
    seen = {}
    for extras in (("invdepth",), ("alpha",), BOTH, BOTH[::-1]):
        for path in ("inference", "training"):
            rast.num_rendered = None
            if path == "inference":
                with torch.no_grad():
                    out = rast(extras=extras, **inp)
            else:
                out = rast(extras=extras, **inp)
            assert isinstance(out, tuple) and len(out) == 2 + len(extras)
            assert (out[0].grad_fn is not None) == (path == "training") and out[1].grad_fn is None
            assert torch.equal(out[0].detach(), img_i), (extras, path)
            assert torch.equal(out[1], radii_i) and rast.num_rendered == nr, (extras, path)
            for name, m in zip(extras, out[2:]):
                assert m.shape == (1, H, W) and m.dtype == torch.float32 and m.is_cuda, (extras, path, name)
                assert (m.grad_fn is not None) == (path == "training")
                first = seen.setdefault(name, m.detach())       # the same map whatever the path, the company and the order asked
                assert torch.equal(m.detach(), first), (extras, path, name)
    assert float(seen["invdepth"].max()) > 0 and 0.5 < float(seen["alpha"].max()) <= 1.0 and float(seen["alpha"].min()) >= 0.0
    assert rast(extras=(), **inp)[0].shape == (3, H, W) and len(rast(extras=None, **inp)) == 2


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", list(CASES))
def test_gradients_match_float64_reference(case, loss):
    n, W, H, seed, use_cov, sm, cluster, camera = CASES[case]
    c = _case(case)
    out, g = _device_grads(c["rast"], c["sc"], use_cov, sm, loss, c["Wt"])
    r = c["radii"]
    assert torch.equal(out[1].cpu(), r)
    for k, v in g.items():
        assert v is not None and torch.isfinite(v).all(), k
        assert (v[r <= 0] == 0).all(), k
        if k == "means2D":
            assert (v[:, 2] == 0).all()
            continue
        if k == "colors_precomp" and loss != "all":
            assert torch.count_nonzero(v) == 0                  # no colour gradient from the maps
            continue
        gr = c["ref_grads"][loss][k]
        rel = float((v.cpu().double() - gr).norm() / gr.norm())
        print(f"aux backward {case} loss={loss} {k}: {rel:.3e}")
        assert rel <= 1e-4, (k, rel)


@pytest.mark.parametrize("case", ["partial_tiles_sm", "cov3D_precomp"])
def test_extras_without_gradient_change_nothing(case):
    """Extras requested, the loss on the image alone: every input gradient is the one of the call without extras, bit for bit."""
    n, W, H, seed, use_cov, sm, cluster, camera = CASES[case]
    c = _case(case)
    base = _inputs(c["sc"], use_cov, sm)
    img, _ = c["rast"](shs=None, **base)
    (img * c["Wt"]["image"]).sum().backward()
    for extras in (("invdepth",), ("alpha",), BOTH):
        inp = _inputs(c["sc"], use_cov, sm)
        out = c["rast"](shs=None, extras=extras, **inp)
        (out[0] * c["Wt"]["image"]).sum().backward()
        for k, v in inp.items():
            if v is not None:
                assert torch.equal(v.grad, base[k].grad), (extras, k)


def test_backward_bitwise_deterministic():
    n, W, H, seed, use_cov, sm, cluster, camera = CASES["long_lists"]
    c = _case("long_lists")
    runs = [_device_grads(c["rast"], c["sc"], use_cov, sm, "all", c["Wt"])[1] for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("P", [0, 200])
def test_degenerate_frames(P):
    """No Gaussian at all, and 200 Gaussians behind the camera: zero maps, a background image, and a backward that returns zeros."""
    from gauspcc_amd.rasterizer import GaussianRasterizer

    W, H = 48, 32
    sc = rr.training_scene(200, 5, W, H)
    sc["means"][:, 2] = -7.0 - np.abs(sc["means"][:, 2])        # view depth z + 6 <= -1
    rast = GaussianRasterizer(_settings(sc, W, H, BG))
    inp = {k: (None if v is None else v.detach()[:P].clone().requires_grad_(True)) for k, v in _inputs(sc, False, 1.0).items()}
    Wt = _weights(3, H, W)
    bg_img = torch.tensor(BG).cuda()[:, None, None].expand(3, H, W)
    with torch.no_grad():
        img_i, radii_i, inv_i, alp_i = rast(shs=None, extras=BOTH, **inp)
    img, radii, inv, alp = rast(shs=None, extras=BOTH, **inp)
    for i, m, a in ((img_i, inv_i, alp_i), (img.detach(), inv.detach(), alp.detach())):
        assert torch.equal(i, bg_img)
        assert m.shape == (1, H, W) and a.shape == (1, H, W) and torch.count_nonzero(m) == 0 and torch.count_nonzero(a) == 0
    assert radii.shape == (P,) and not radii.any() and not radii_i.any()
    _loss("all", img, inv, alp, Wt).backward()
    for k, v in inp.items():
        if v is not None:
            assert v.grad is not None and v.grad.shape == v.shape and torch.count_nonzero(v.grad) == 0, k


def test_state_survives_other_calls():
    """Between a forward with extras and its backward, other rasteriser calls without extras run (an inference frame of another size of
    problem and a training frame with its own backward): the first frame's gradients are those of the undisturbed run, bit for bit."""
    n, W, H, seed, use_cov, sm, cluster, camera = CASES["partial_tiles_sm"]
    c = _case("partial_tiles_sm")
    _, want = _device_grads(c["rast"], c["sc"], use_cov, sm, "all", c["Wt"])
    inp = _inputs(c["sc"], use_cov, sm)
    img, _, inv, alp = c["rast"](shs=None, extras=BOTH, **inp)
    other = _case("long_lists")
    n2, W2, H2, _, cov2, sm2, _, _ = CASES["long_lists"]
    with torch.no_grad():
        other["rast"](shs=None, **_inputs(other["sc"], cov2, sm2))
    inp2 = _inputs(other["sc"], cov2, sm2)
    (other["rast"](shs=None, **inp2)[0] * other["Wt"]["image"]).sum().backward()
    c["rast"].visible_filter(means3D=inp["means3D"], scales=inp["scales"], rotations=inp["rotations"])
    _loss("all", img, inv, alp, c["Wt"]).backward()
    for k, v in inp.items():
        if v is not None:
            assert torch.equal(v.grad, want[k]), k
