"""GPU checks of the rasteriser's backward (GaussianRasterizer under autograd: gsr_forward_train + gsr_backward) against the float64
restatement of tests/raster_ref.py, and its bookkeeping at the scale of the 1 M-anchor RD frame."""
import math
import types

import numpy as np
import pytest
import torch

from tests import raster_ref as rr

pytestmark = pytest.mark.gpu

NAMES = ("means3D", "means2D", "opacities", "colors_precomp", "scales", "rotations", "cov3D_precomp")


def _settings(sc, W, H, bg, scale_modifier=1.0):
    from gauspcc_amd.rasterizer import GaussianRasterizationSettings

    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=sc["tx"], tanfovy=sc["ty"], bg=torch.tensor(bg).cuda(),
                                         scale_modifier=scale_modifier, viewmatrix=torch.tensor(sc["view"]).cuda(),
                                         projmatrix=torch.tensor(sc["proj"]).cuda(), sh_degree=1,
                                         campos=torch.tensor(sc.get("campos", [0.0, 0.0, -6.0])).cuda(),
                                         prefiltered=False, debug=False)


def _cov(scales, rots, sm):
    s = sm * scales.double()
    r, x, y, z = rots.double().unbind(1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                     torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                     torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    S = R @ torch.diag_embed(s * s) @ R.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()


def _inputs(sc, use_cov, sm):
    t = rr.tensors(sc, "cuda")
    d = dict(means3D=t["means"], means2D=torch.zeros_like(t["means"]), opacities=t["opac"], colors_precomp=t["colors"])
    if use_cov:
        d.update(scales=None, rotations=None, cov3D_precomp=_cov(t["scales"].cpu(), t["rots"].cpu(), sm).cuda())
    else:
        d.update(scales=t["scales"], rotations=t["rots"], cov3D_precomp=None)
    return {k: (None if v is None else v.clone().requires_grad_(True)) for k, v in d.items()}


def _device_grads(rast, inp, R):
    img, radii = rast(shs=None, **inp)
    (img * R).sum().backward()
    return img, radii, {k: v.grad for k, v in inp.items() if v is not None}


@pytest.mark.parametrize("n,W,H,seed,use_cov,sm,cluster", [
    (300, 48, 32, 1, False, 1.0, 0),
    (2000, 96, 64, 2, False, 1.0, 300),
    (1200, 83, 45, 3, False, 1.25, 300),      # non-square, partial tiles, scale_modifier != 1
    (1200, 83, 45, 4, True, 1.0, 300),        # cov3D_precomp
])
def test_gradients_match_float64_reference(n, W, H, seed, use_cov, sm, cluster):
    _check_gradients(rr.training_scene(n, seed, W, H, cluster=cluster), n, W, H, seed, use_cov, sm, cluster, rr.project)


ROTATED = [c for c in rr.CAMERAS if c != "identity"]


@pytest.mark.parametrize("n,W,H,seed,use_cov,sm,cluster", [
    (1200, 83, 45, 3, False, 1.25, 300),
    (1200, 83, 45, 4, True, 1.0, 300),
])
@pytest.mark.parametrize("camera", ROTATED)
def test_gradients_match_float64_reference_cameras(camera, n, W, H, seed, use_cov, sm, cluster):
    """The same bounds under the rotated cameras of tests/golden/cameras.npz, against the reference rendered through the index-free
    projection (raster_ref.project_matrix_form): k_preprocess_backward's reading of the view matrix and of the two focal lengths."""
    _check_gradients(rr.scene_for_camera(rr.cameras()[camera], n, seed, W, H, cluster=cluster), n, W, H, seed, use_cov, sm, cluster,
                     rr.project_matrix_form)


def _check_gradients(sc, n, W, H, seed, use_cov, sm, cluster, project):
    from gauspcc_amd.rasterizer import GaussianRasterizer

    bg = np.array([0.2, 0.4, 0.1], np.float32)
    rast = GaussianRasterizer(_settings(sc, W, H, bg, sm))
    inp = _inputs(sc, use_cov, sm)
    R = torch.tensor(np.random.RandomState(seed).randn(3, H, W).astype(np.float32)).cuda()
    img, radii, g = _device_grads(rast, inp, R)
    assert img.grad_fn is not None and radii.grad_fn is None
    r = radii.cpu()
    assert 0 < int((r > 0).sum()) < n
    # the reference, binned with the device's radii
    ref_in = {k: (None if v is None else v.detach().cpu().double().requires_grad_(True)) for k, v in inp.items()}
    ref_img, dec = rr.render(ref_in["means3D"], ref_in["opacities"], ref_in["colors_precomp"], ref_in["scales"], ref_in["rotations"],
                             ref_in["cov3D_precomp"], sm, torch.tensor(sc["view"]), torch.tensor(sc["proj"]), sc["tx"], sc["ty"], W, H, bg, r,
                             project=project)
    dimg = np.abs(ref_img.detach().numpy() - img.detach().cpu().numpy()).max()
    print(f"backward {n} {W}x{H} cov3D_precomp={use_cov}: max |image - float64| {dimg:.3e}")
    assert dimg < 1e-4
    if cluster:
        assert max(d.shape[1] for d in dec.values()) > 256
    (ref_img * R.cpu().double()).sum().backward()
    for k, v in g.items():
        assert v.shape == inp[k].shape and v.dtype == inp[k].dtype, k
        assert torch.isfinite(v).all(), k
        assert (v[r <= 0] == 0).all(), k
        if k == "means2D":
            assert (v[:, 2] == 0).all()
            continue
        gr = ref_in[k].grad
        gd = v.cpu().double()
        rel = float((gd - gr).norm() / gr.norm())
        print(f"  {k}: {rel:.3e}")
        assert rel <= 1e-4, (k, rel)         # measured <= 3.2e-6 (profiles/r07_raster_backward.txt), <= 5.0e-6 under the cameras (r09_raster_cameras.txt)


def _check_means2D(sc, n, W, H, project):
    from gauspcc_amd.rasterizer import GaussianRasterizer

    bg = np.zeros(3, np.float32)
    rast = GaussianRasterizer(_settings(sc, W, H, bg))
    inp = _inputs(sc, False, 1.0)
    R = torch.tensor(np.random.RandomState(1).randn(3, H, W).astype(np.float32)).cuda()
    _, radii, g = _device_grads(rast, inp, R)
    # the reference with the centre (ix, iy) replaced by a leaf of the same value
    t = {k: inp[k].detach().cpu().double() for k in ("means3D", "opacities", "colors_precomp", "scales", "rotations")}
    ix, iy, *rest = project(t["means3D"], t["scales"], t["rotations"], None, 1.0, torch.tensor(sc["view"]), torch.tensor(sc["proj"]), sc["tx"], sc["ty"], W, H)
    cx, cy = ix.clone().requires_grad_(True), iy.clone().requires_grad_(True)
    img, _ = rr.render(t["means3D"], t["opacities"], t["colors_precomp"], t["scales"], t["rotations"], None, 1.0, torch.tensor(sc["view"]),
                       torch.tensor(sc["proj"]), sc["tx"], sc["ty"], W, H, bg, radii.cpu(), project=lambda *a: (cx, cy, *rest))
    (img * R.cpu().double()).sum().backward()
    ref = torch.stack([cx.grad * (W / 2), cy.grad * (H / 2)], 1)
    dev = g["means2D"].cpu().double()[:, :2]
    rel = float((dev - ref).norm() / ref.norm())
    print(f"means2D {n} {W}x{H}: {rel:.3e}")
    assert rel <= 1e-3


def test_means2D_matches_reference_pixel_gradient():
    """means2D.grad[:, :2] is dL/d(NDC) = dL/d(pixel centre) * (W/2, H/2) of the reference with its centre as a free input."""
    n, W, H, seed = 800, 64, 48, 9
    _check_means2D(rr.training_scene(n, seed, W, H), n, W, H, rr.project)


def test_means2D_matches_reference_pixel_gradient_anisotropic():
    """The same under `general_anisotropic` (tests/golden/cameras.npz): W / 2 != H / 2 and focal_x != focal_y (70.4 against 41.4 pixels),
    so neither pair can stand in for the other."""
    n, W, H, seed = 800, 68, 48, 9
    _check_means2D(rr.scene_for_camera(rr.cameras()["general_anisotropic"], n, seed, W, H), n, W, H, rr.project_matrix_form)


def test_inference_unchanged():
    from gauspcc_amd.rasterizer import GaussianRasterizer

    n, W, H = 3000, 200, 120
    sc = rr.training_scene(n, 21, W, H, cluster=200)
    rast = GaussianRasterizer(_settings(sc, W, H, np.array([0.1, 0.2, 0.3], np.float32)))
    inp = _inputs(sc, False, 1.0)
    img_t, radii_t = rast(shs=None, **inp)
    nr_t = rast.num_rendered
    with torch.no_grad():
        img_i, radii_i = rast(shs=None, **inp)
    assert img_t.grad_fn is not None and img_i.grad_fn is None
    assert torch.equal(img_t.detach(), img_i) and torch.equal(radii_t, radii_i) and rast.num_rendered == nr_t
    plain = {k: (None if v is None else v.detach()) for k, v in inp.items()}
    img_p, _ = rast(shs=None, **plain)                      # nothing requires grad: the inference path
    assert img_p.grad_fn is None and torch.equal(img_p, img_i)


@pytest.mark.parametrize("P", [0, 200])
def test_degenerate_training_frames(P):
    """No Gaussian at all (empty inputs that require grad), and 200 Gaussians behind the camera (no (Gaussian, tile) pair: the pair-sized
    state is never asked for): the training frame is the inference frame, all background, and the backward returns zeros."""
    from gauspcc_amd.rasterizer import GaussianRasterizer

    W, H = 48, 32
    sc = rr.training_scene(200, 5, W, H)
    sc["means"][:, 2] = -7.0 - np.abs(sc["means"][:, 2])        # view depth z + 6 <= -1
    bg = np.array([0.2, 0.4, 0.1], np.float32)
    rast = GaussianRasterizer(_settings(sc, W, H, bg))
    inp = {k: (None if v is None else v.detach()[:P].clone().requires_grad_(True)) for k, v in _inputs(sc, False, 1.0).items()}
    img_t, radii_t = rast(shs=None, **inp)
    nr_t = rast.num_rendered
    with torch.no_grad():
        img_i, radii_i = rast(shs=None, **inp)
    assert img_t.grad_fn is not None and img_i.grad_fn is None
    assert torch.equal(img_t.detach(), img_i) and torch.equal(radii_t, radii_i) and rast.num_rendered == nr_t
    assert torch.equal(img_i, torch.tensor(bg).cuda()[:, None, None].expand(3, H, W))
    assert radii_t.shape == (P,) and not radii_t.any()
    R = torch.tensor(np.random.RandomState(3).randn(3, H, W).astype(np.float32)).cuda()
    (img_t * R).sum().backward()
    for k, v in inp.items():
        if v is not None:
            assert v.grad is not None and v.grad.shape == v.shape and torch.count_nonzero(v.grad) == 0, k


def test_backward_bitwise_deterministic_small():
    from gauspcc_amd.rasterizer import GaussianRasterizer

    n, W, H = 2000, 96, 64
    sc = rr.training_scene(n, 2, W, H, cluster=300)
    rast = GaussianRasterizer(_settings(sc, W, H, np.array([0.2, 0.4, 0.1], np.float32)))
    R = torch.tensor(np.random.RandomState(2).randn(3, H, W).astype(np.float32)).cuda()
    runs = []
    for _ in range(2):
        inp = _inputs(sc, False, 1.0)
        runs.append(_device_grads(rast, inp, R)[2])
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_state_survives_other_calls():
    """Two training forwards (two cameras) with an inference forward and a visible_filter between them, one backward of the summed loss:
    the gradients equal the sum of the two separate backwards, bit for bit."""
    from gauspcc_amd.rasterizer import GaussianRasterizer

    n, W, H = 1500, 96, 64
    sc = rr.training_scene(n, 31, W, H, cluster=100)
    sc2 = dict(sc)
    # the camera turned (0.2 rad about (0.3, 1, 0.2)) and moved; p_view2 = Rot p_view + shift; row-vector matrices: Rot^T on the right, translation in row 3
    k = np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    turn = np.eye(4); turn[:3, :3] = (np.eye(3) + math.sin(0.2) * K + (1 - math.cos(0.2)) * (K @ K)).T
    view2 = sc["view"].astype(np.float64) @ turn; view2[3, 0] += 0.4; view2[3, 1] -= 0.3
    view2 = view2.astype(np.float32)
    assert np.abs(view2[:3, :3] - view2[:3, :3].T).max() > 0.1
    sc2["view"] = view2
    Pm = np.linalg.solve(sc["view"].astype(np.float64), sc["proj"].astype(np.float64))
    sc2["proj"] = (view2.astype(np.float64) @ Pm).astype(np.float32)
    r1 = GaussianRasterizer(_settings(sc, W, H, np.zeros(3, np.float32)))
    r2 = GaussianRasterizer(_settings(sc2, W, H, np.zeros(3, np.float32)))
    R1 = torch.tensor(np.random.RandomState(1).randn(3, H, W).astype(np.float32)).cuda()
    R2 = torch.tensor(np.random.RandomState(2).randn(3, H, W).astype(np.float32)).cuda()
    sep = []
    for r, R in ((r1, R1), (r2, R2)):
        inp = _inputs(sc, False, 1.0)
        sep.append(_device_grads(r, inp, R)[2])
    inp = _inputs(sc, False, 1.0)
    img1, _ = r1(shs=None, **inp)
    with torch.no_grad():
        r2(shs=None, **{k: (None if v is None else v.detach() * 1.01) for k, v in inp.items()})
    r1.visible_filter(means3D=inp["means3D"], scales=inp["scales"], rotations=inp["rotations"])
    img2, _ = r2(shs=None, **inp)
    ((img1 * R1).sum() + (img2 * R2).sum()).backward()
    for k, v in inp.items():
        if v is not None:
            assert torch.equal(v.grad, sep[0][k] + sep[1][k]), k


def test_hac_call_shape():
    """HAC/gaussian_renderer/__init__.py:187-225: screenspace_points = zeros_like(xyz, requires_grad=True) + 0; retain_grad(); after backward its
    .grad is (P, 3), non-zero only where radii > 0 (what training_statis reads)."""
    from gauspcc_amd.rasterizer import GaussianRasterizer

    n, W, H = 1500, 96, 64
    sc = rr.training_scene(n, 41, W, H)
    t = rr.tensors(sc, "cuda")
    xyz = t["means"].clone().requires_grad_(True)
    opacity, color = t["opac"].clone().requires_grad_(True), t["colors"].clone().requires_grad_(True)
    scaling, rot = t["scales"].clone().requires_grad_(True), t["rots"].clone().requires_grad_(True)
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device="cuda") + 0
    screenspace_points.retain_grad()
    rast = GaussianRasterizer(_settings(sc, W, H, np.zeros(3, np.float32)))
    rendered_image, radii = rast(means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=color, opacities=opacity, scales=scaling,
                                 rotations=rot, cov3D_precomp=None)
    (rendered_image - 0.5).abs().mean().backward()
    g = screenspace_points.grad
    assert g is not None and g.shape == (n, 3)
    vis = radii > 0
    assert (g[~vis] == 0).all() and (g[:, 2] == 0).all()
    assert (g[vis, :2].norm(dim=-1) > 0).float().mean() > 0.5
    for p in (xyz, opacity, color, scaling, rot):
        assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad[~vis] == 0).all()


def test_it_trains():
    from gauspcc_amd.rasterizer import GaussianRasterizer

    n, W, H = 500, 64, 48
    sc = rr.scene(n, 51, W, H)
    rast = GaussianRasterizer(_settings(sc, W, H, np.zeros(3, np.float32)))
    t = rr.tensors(sc, "cuda")
    logit = lambda p: torch.log(p / (1 - p))
    with torch.no_grad():
        target, _ = rast(means3D=t["means"], means2D=None, shs=None, colors_precomp=t["colors"], opacities=t["opac"], scales=t["scales"],
                         rotations=t["rots"], cov3D_precomp=None)
    g = torch.Generator(device="cuda").manual_seed(0)
    params = dict(m=(t["means"] + 0.05 * torch.randn(t["means"].shape, device="cuda", generator=g)),
                  ls=(torch.log(t["scales"]) + 0.2 * torch.randn(t["scales"].shape, device="cuda", generator=g)),
                  q=(t["rots"] + 0.1 * torch.randn(t["rots"].shape, device="cuda", generator=g)),
                  lo=(logit(t["opac"].clamp(0.01, 0.99)) + 0.5 * torch.randn(t["opac"].shape, device="cuda", generator=g)),
                  c=(t["colors"] + 0.2 * torch.randn(t["colors"].shape, device="cuda", generator=g)))
    params = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam([{"params": [params["m"]], "lr": 2e-3}, {"params": [params["ls"], params["q"], params["lo"], params["c"]], "lr": 1e-2}])
    losses = []
    for _ in range(300):
        opt.zero_grad()
        img, _ = rast(means3D=params["m"], means2D=None, shs=None, colors_precomp=params["c"], opacities=torch.sigmoid(params["lo"]),
                      scales=torch.exp(params["ls"]), rotations=torch.nn.functional.normalize(params["q"]), cov3D_precomp=None)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] / 10, (losses[0], losses[-1])


@pytest.fixture(scope="module")
def rd_frame():
    """The 1 M-anchor synthetic RD frame of tools/rd_frame_probe.py (1600 x 1060)."""
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians
    from gauspcc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from gauspcc_amd.synth import SyntheticGaussianModel

    W, H = 1600, 1060
    dev = torch.device("cuda", 0)
    enc = SyntheticGaussianModel(1_000_000, seed=0, device="cuda:0")
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
    settings = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(fovx / 2), tanfovy=math.tan(fovy / 2),
                                             bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=full, sh_degree=1,
                                             campos=eye, prefiltered=False, debug=False)
    with torch.no_grad():
        xyz, color, opacity, scaling, rot, _ = generate_neural_gaussians(types.SimpleNamespace(camera_center=eye), enc, None)
    return GaussianRasterizer(settings), dict(means3D=xyz, opacities=opacity, colors_precomp=color, scales=scaling, rotations=rot), (H, W)


def _frame_grads(rast, attrs, R):
    inp = {k: v.detach().clone().requires_grad_(True) for k, v in attrs.items()}
    img, radii = rast(means2D=None, shs=None, cov3D_precomp=None, **inp)
    (img * R).sum().backward()
    torch.cuda.synchronize()
    return radii, {k: v.grad for k, v in inp.items()}


def test_rd_frame_deterministic_and_exact_colour_bookkeeping(rd_frame):
    rast, attrs, (H, W) = rd_frame
    R = torch.randn((3, H, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    radii, g1 = _frame_grads(rast, attrs, R)
    assert rast.num_rendered > 5_000_000
    _, g2 = _frame_grads(rast, attrs, R)
    vis = radii > 0
    assert 0 < int(vis.sum()) < radii.numel()
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert torch.isfinite(g1[k]).all(), k
        assert (g1[k][~vis] == 0).all(), k
    # the image is linear in the colours and no decision depends on them: <grad_c L, v> = (L(c + v) - L(c - v)) / 2 from the forward alone
    v = torch.randn(attrs["colors_precomp"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    lin = []
    with torch.no_grad():
        for sgn in (1.0, -1.0):
            a = dict(attrs); a["colors_precomp"] = attrs["colors_precomp"] + sgn * v
            img, _ = rast(means2D=None, shs=None, cov3D_precomp=None, **a)
            lin.append((img.double() * R.double()).sum().item())
    fd = (lin[0] - lin[1]) / 2
    an = (g1["colors_precomp"].double() * v.double()).sum().item()
    assert abs(an - fd) <= 1e-4 * abs(fd), (an, fd)
