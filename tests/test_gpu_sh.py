"""GPU checks of the spherical-harmonic colour pass (gsr_sh_forward / gsr_sh_backward behind gauspcc_amd.sh_utils and the rasteriser's
shs= argument): values and gradients bit for bit against the numpy float32 restatement of tests/sh_ref.py, gradients against its float64
version within the project's bound e_dev <= 4 e_t32 + 1e-6 scale (e_t32 the float32 torch program's error on the same inputs, scale the
largest reference magnitude), and the rasteriser with shs= against the same frame with the colours precomputed."""
import numpy as np
import pytest
import torch

from tests import raster_ref as rr
from tests import sh_ref as sr

pytestmark = pytest.mark.gpu

CAM = np.array([0.25, -0.5, 3.0], np.float32)


def _cuda(a, grad=False):
    return torch.tensor(a, device="cuda").requires_grad_(grad)


def _same_bits(t, want, what):
    got = t.detach().cpu().numpy()
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, float(np.abs(got - want).max()))


def _inputs(P, M, seed, half_negative=False):
    rng = np.random.default_rng(seed)
    sh = rng.standard_normal((P, M, 3)).astype(np.float32)
    if half_negative:
        sh[:, 0] -= np.float32(0.5 / sr.C0)                  # value + 0.5 symmetric about 0
    means = rng.uniform(-2, 2, (P, 3)).astype(np.float32)
    dirs = rng.standard_normal((P, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    dcol = rng.standard_normal((P, 3)).astype(np.float32)
    return sh, means, dirs, dcol


def _check_bits(shs, sh_np, means, dirs, dcol, deg, what):
    """shs: a CUDA leaf (P, M, 3) (any strides) holding sh_np.  sh_colors and eval_sh, forward and backward, against the restatement."""
    from gauspcc_amd import sh_utils

    m = _cuda(means, True)
    col = sh_utils.sh_colors(shs, m, _cuda(CAM), deg)
    want, clamped = sr.forward32(sh_np, deg, means=means, campos=CAM)
    _same_bits(col, want, (what, "colours"))
    col.backward(_cuda(dcol))
    gsh, gm = sr.backward32(sh_np, deg, dcol, means=means, campos=CAM, clamped=clamped)
    _same_bits(shs.grad, gsh, (what, "dL_dsh"))
    _same_bits(m.grad, gm, (what, "dL_dmeans3D"))
    shs.grad = None
    # eval_sh reads (P, 3, M): the same memory through the transposed view
    d = _cuda(dirs, True)
    val = sh_utils.eval_sh(deg, shs.transpose(1, 2), d)
    _same_bits(val, sr.forward32(sh_np, deg, dirs=dirs)[0], (what, "eval_sh"))
    val.backward(_cuda(dcol))
    gsh, gd = sr.backward32(sh_np, deg, dcol, dirs=dirs)
    _same_bits(shs.grad, gsh, (what, "eval_sh dL_dsh"))
    _same_bits(d.grad, gd, (what, "dL_ddirs"))
    shs.grad = None


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000])
def test_values_and_gradients_bit_for_bit(P, deg):
    """Both layouts at the wave edges and over many workgroups: (P, M, 3) contiguous (the rasteriser's; eval_sh sees it as a strided
    (P, 3, M)) and (P, 3, M) contiguous (eval_sh's; sh_colors sees it as a strided (P, M, 3))."""
    M = sr.count(deg)
    sh, means, dirs, dcol = _inputs(P, M, 100 * deg + P)
    _check_bits(_cuda(sh, True), sh, means, dirs, dcol, deg, ("(P, M, 3)", P, deg))
    base = _cuda(np.ascontiguousarray(sh.transpose(0, 2, 1)), True)         # (P, 3, M) contiguous
    shs = base.transpose(1, 2)
    assert M == 1 or P == 1 or not shs.is_contiguous()
    from gauspcc_amd import sh_utils

    col = sh_utils.sh_colors(shs, _cuda(means), _cuda(CAM), deg)
    want, clamped = sr.forward32(sh, deg, means=means, campos=CAM)
    _same_bits(col, want, ("(P, 3, M)", P, deg))
    col.backward(_cuda(dcol))
    _same_bits(base.grad.transpose(1, 2).contiguous(), sr.backward32(sh, deg, dcol, means=means, campos=CAM, clamped=clamped)[0], ("(P, 3, M) grad", P, deg))
    base.grad = None
    d = _cuda(dirs, True)
    val = sh_utils.eval_sh(deg, base, d)
    _same_bits(val, sr.forward32(sh, deg, dirs=dirs)[0], ("(P, 3, M) eval_sh", P, deg))
    val.backward(_cuda(dcol))
    gsh, gd = sr.backward32(sh, deg, dcol, dirs=dirs)
    _same_bits(base.grad.transpose(1, 2).contiguous(), gsh, ("(P, 3, M) eval_sh grad", P, deg))
    _same_bits(d.grad, gd, ("(P, 3, M) dL_ddirs", P, deg))


@pytest.mark.parametrize("deg", [0, 1, 2])
@pytest.mark.parametrize("P", [65, 1000])
def test_more_coefficients_stored_than_active(P, deg):
    """M = 16 with degree 0..2: the inactive coefficients are not read into the sum and their gradient entries are written as zeros."""
    sh, means, dirs, dcol = _inputs(P, 16, 7 + deg)
    sh[:, sr.count(deg):] = np.float32(1e30)                 # would show in any sum that touched it
    shs = _cuda(sh, True)
    _check_bits(shs, sh, means, dirs, dcol, deg, ("M = 16", P, deg))
    from gauspcc_amd import sh_utils

    sh_utils.sh_colors(shs, _cuda(means), _cuda(CAM), deg).sum().backward()
    assert not shs.grad[:, sr.count(deg):].any() and shs.grad[:, : sr.count(deg)].any()


def test_non_contiguous_views_and_direct_path():
    P = 333
    sh, means, dirs, dcol = _inputs(P, 25, 11)
    # a slice of wider rows: row stride 75, 16 coefficients; every other row; both are staged with 4-byte loads
    big = _cuda(sh)
    _check_bits(big[:, :16].detach().requires_grad_(True), sh[:, :16], means, dirs, dcol, 3, "slice of wider rows")
    v = big[::2].detach()
    assert not v.is_contiguous()
    v.requires_grad_(True)
    _check_bits(v, sh[::2], means[::2], dirs[::2], dcol[::2], 4, "every other row")
    # an offset of 4 bytes from an aligned block: dense rows that are not 16-byte aligned
    flat = torch.zeros(P * 48 + 1, device="cuda")
    off = flat[1:].view(P, 16, 3)
    off.copy_(_cuda(sh[:, :16]))
    _check_bits(off.detach().requires_grad_(True), sh[:, :16], means, dirs, dcol, 3, "unaligned")
    # the direct path: a broadcast coefficient (stride 0) and rows too wide for LDS staging (M = 40: the gradient's 120-float rows)
    one = _cuda(sh[:, :1])
    _check_bits(one.expand(P, 4, 3).detach().requires_grad_(True), np.broadcast_to(sh[:, :1], (P, 4, 3)).copy(), means, dirs, dcol, 1, "broadcast coefficient")
    wide = np.random.default_rng(5).standard_normal((P, 40, 3)).astype(np.float32)
    _check_bits(_cuda(wide, True), wide, means, dirs, dcol, 4, "M = 40")
    wide_t = _cuda(np.ascontiguousarray(wide.transpose(0, 2, 1)))           # (P, 3, 40): the active span is 105 floats
    _check_bits(wide_t.transpose(1, 2).detach().requires_grad_(True), wide, means, dirs, dcol, 4, "(P, 3, 40)")


def _raw_forward(shs, means, campos, deg):
    from gauspcc_amd import _lib, runtime

    P, dev = means.shape[0], means.device
    colors = torch.empty((P, 3), device=dev)
    clamped = torch.empty((P, 3), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().gsr_sh_forward(runtime.context(dev), P, deg, shs.data_ptr(), shs.stride(1), shs.stride(2), shs.stride(0), means.data_ptr(),
                                         campos.data_ptr(), None, colors.data_ptr(), clamped.data_ptr(), runtime.stream_ptr(dev)))
    return colors, clamped


def test_clamp():
    from gauspcc_amd import sh_utils

    P, deg = 1000, 3
    sh, means, _, dcol = _inputs(P, 16, 21, half_negative=True)
    want, clamped = sr.forward32(sh, deg, means=means, campos=CAM)
    assert 0.4 < clamped.mean() < 0.6                        # roughly half the channels go negative
    col, cl = _raw_forward(_cuda(sh), _cuda(means), _cuda(CAM), deg)
    assert np.array_equal(cl.cpu().numpy().astype(bool), clamped)
    _same_bits(col, want, "colours")
    shs = _cuda(sh, True)
    sh_utils.sh_colors(shs, _cuda(means), _cuda(CAM), deg).backward(_cuda(dcol))
    g = shs.grad.cpu().numpy()
    off = np.broadcast_to(clamped[:, None, :], g.shape)
    assert (g[off] == 0.0).all() and not np.signbit(g[off]).any()
    assert (g[~off] != 0.0).all()                            # a nonzero basis value times a nonzero upstream gradient


def test_exact_zero_is_not_clamped():
    """value + 0.5 == 0 exactly: clamped records value < 0, so the gradient passes."""
    from gauspcc_amd import sh_utils

    c0 = np.float32(sr.C0)
    s = np.float32(-0.5) / c0
    cands = [s]
    for _ in range(4):
        cands = [np.nextafter(cands[0], np.float32(-10)), *cands, np.nextafter(cands[-1], np.float32(10))]
    exact = [x for x in cands if c0 * x + np.float32(0.5) == 0]
    assert exact, "no float32 coefficient gives exactly -0.5"
    below = np.nextafter(exact[0], np.float32(-10))
    while c0 * below + np.float32(0.5) == 0:
        below = np.nextafter(below, np.float32(-10))
    sh = np.zeros((2, 1, 3), np.float32)
    sh[0, 0, :], sh[1, 0, :] = exact[0], below
    means = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], np.float32)
    col, cl = _raw_forward(_cuda(sh), _cuda(means), _cuda(CAM), 0)
    assert cl.cpu().numpy().tolist() == [[0, 0, 0], [1, 1, 1]] and (col == 0).all()
    shs = _cuda(sh, True)
    sh_utils.sh_colors(shs, _cuda(means), _cuda(CAM), 0).sum().backward()
    g = shs.grad.cpu().numpy()
    assert (g[0, 0] == c0).all() and (g[1, 0] == 0).all()


def test_camera_centre_and_nan():
    from gauspcc_amd import sh_utils

    P, deg = 130, 3
    sh, means, _, dcol = _inputs(P, 16, 31)
    sh[:, 0] = np.abs(sh[:, 0]) + 2                          # bright: nothing clamps
    means[64] = CAM
    shs, m = _cuda(sh, True), _cuda(means, True)
    col = sh_utils.sh_colors(shs, m, _cuda(CAM), deg)
    col.backward(_cuda(dcol))
    assert torch.isfinite(col).all() and torch.isfinite(m.grad).all() and torch.isfinite(shs.grad).all()
    _same_bits(col[64], np.float32(sr.C0) * sh[64, 0] + np.float32(0.5), "the DC term")
    assert (m.grad[64] == 0).all() and (m.grad[63] != 0).any() and (m.grad[65] != 0).any()
    assert (shs.grad[64, 1:] == 0).all() and (shs.grad[64, 0] != 0).all()      # d = 0: every basis value above the DC term is 0
    _same_bits(col, sr.forward32(sh, deg, means=means, campos=CAM)[0], "colours")
    # NaN stays in its own Gaussian
    sh[7, 3, 1] = np.nan
    means[9, 0] = np.nan
    shs, m = _cuda(sh, True), _cuda(means, True)
    col = sh_utils.sh_colors(shs, m, _cuda(CAM), deg)
    col.backward(_cuda(dcol))
    bad = torch.zeros(P, dtype=torch.bool, device="cuda")
    bad[7] = bad[9] = True
    assert torch.isnan(col[7, 1]) and torch.isnan(col[9]).all() and torch.isnan(m.grad[9]).all()
    assert torch.isfinite(col[~bad]).all() and torch.isfinite(m.grad[~bad]).all() and torch.isfinite(shs.grad[~bad]).all()


def _holds(dev, t32, ref, what, mask=None):
    """e_dev <= 4 e_t32 + 1e-6 scale over the entries of `mask` (all without one)."""
    dev, t32, ref = dev.detach().double().cpu(), t32.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(ref.abs().max())
    if mask is not None:
        dev, t32, ref = dev[mask], t32[mask], ref[mask]
    e_dev, e_t32 = float((dev - ref).abs().max()), float((t32 - ref).abs().max())
    print(what, "e_dev", e_dev, "e_t32", e_t32, "scale", scale)
    assert e_dev <= 4 * e_t32 + 1e-6 * scale, (what, e_dev, e_t32, scale)


@pytest.mark.parametrize("deg", [1, 3])
def test_gradients_against_float64(deg):
    from gauspcc_amd import sh_utils

    P, M = 1000, 16
    sh, means, dirs, dcol = _inputs(P, M, 40 + deg, half_negative=True)
    w = _cuda(dcol)

    def grads(fn, dtype, a, b):
        a, b = _cuda(a).to(dtype).requires_grad_(True), _cuda(b).to(dtype).requires_grad_(True)
        out = fn(a, b)
        (out * w.to(out.dtype)).sum().backward()
        return out, a.grad, b.grad

    cam = _cuda(CAM)
    # the clamping form.  A channel within 1e-5 of the clamp may fall on either side of it in float32: its Gaussian is left out
    c64, s64, m64 = grads(lambda s, m: sr.colors64(s, m, cam, deg), torch.float64, sh, means)
    c32, s32, m32 = grads(lambda s, m: sr.torch32_colors(s, m, cam, deg), torch.float32, sh, means)
    cd, sd, md = grads(lambda s, m: sh_utils.sh_colors(s, m, cam, deg), torch.float32, sh, means)
    pre = sr._torch_values(_cuda(sh).double(), deg, sr._torch_direction(_cuda(means).double(), cam.double())) + 0.5
    rows = (pre.abs() > 1e-5).all(dim=1).cpu()
    assert rows.float().mean() > 0.99
    _holds(cd, c32, c64, ("colours", deg), rows)
    _holds(sd, s32, s64, ("dL_dsh", deg), rows)
    _holds(md, m32, m64, ("dL_dmeans3D", deg), rows)
    assert not sd[:, sr.count(deg):].any()
    # eval_sh: (P, 3, M) and unit directions
    sh_t = np.ascontiguousarray(sh.transpose(0, 2, 1))
    v64, a64, d64 = grads(lambda s, d: sr.eval64(deg, s, d), torch.float64, sh_t, dirs)
    v32, a32, d32 = grads(lambda s, d: sr.torch32_eval(deg, s, d), torch.float32, sh_t, dirs)
    vd, ad, dd = grads(lambda s, d: sh_utils.eval_sh(deg, s, d), torch.float32, sh_t, dirs)
    _holds(vd, v32, v64, ("eval_sh", deg))
    _holds(ad, a32, a64, ("eval_sh dL_dsh", deg))
    _holds(dd, d32, d64, ("dL_ddirs", deg))
    assert not ad[:, :, sr.count(deg):].any()
    # the library's torch path (what a CPU or float64 caller gets) is the same function
    assert float((sh_utils.eval_sh(deg, _cuda(sh_t).double(), _cuda(dirs).double()) - v64.detach()).abs().max()) <= 1e-12 * float(v64.detach().abs().max())


# ---------------------------------------------------------------------------------------------------------------- through the rasteriser
W, H, N = 83, 45, 300


def _frame(camera, deg, M, seed=6):
    from gauspcc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

    sc = rr.scene_for_camera(rr.cameras()[camera], N, seed, W, H)
    t = rr.tensors(sc, "cuda")
    rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=sc["tx"], tanfovy=sc["ty"], bg=torch.tensor([0.1, 0.2, 0.3]).cuda(),
                                       scale_modifier=1.0, viewmatrix=t["view"], projmatrix=t["proj"], sh_degree=deg, campos=t["campos"],
                                       prefiltered=False, debug=False)
    rng = np.random.default_rng(seed)
    shs = (rng.standard_normal((N, M, 3)) * 0.8).astype(np.float32)
    shs[:, 0] += 0.5
    geom = dict(means2D=None, opacities=t["opac"], scales=t["scales"], rotations=t["rots"], cov3D_precomp=None)
    return GaussianRasterizer(rs), rs, t["means"], _cuda(shs), geom


@pytest.mark.parametrize("camera,deg,M", [("general", 3, 16), ("general_anisotropic", 1, 16), ("yaw90", 2, 9)])
def test_rasteriser_shs_equals_precomputed_colours(camera, deg, M):
    from gauspcc_amd import sh_utils

    rast, rs, means, shs, geom = _frame(camera, deg, M)
    with torch.no_grad():
        img, radii = rast(means3D=means, shs=shs, colors_precomp=None, **geom)
        col = sh_utils.sh_colors(shs, means, rs.campos, deg)
        ref, rradii = rast(means3D=means, shs=None, colors_precomp=col, **geom)
    assert (radii > 0).sum() > N // 2 and (col == 0).any() and (col > 0).float().mean() > 0.5
    assert torch.equal(img, ref) and torch.equal(radii, rradii)
    # training mode: the same bits again, and means3D.grad is the sum of the rasteriser's part and the colour pass's
    R = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).cuda()

    def train():
        m, s = means.clone().requires_grad_(True), shs.clone().requires_grad_(True)
        out, rad = rast(means3D=m, shs=s, colors_precomp=None, **geom)
        (out * R).sum().backward()
        return out.detach(), rad, m.grad, s.grad

    img_t, radii_t, gm, gs = train()
    assert torch.equal(img_t, img) and torch.equal(radii_t, radii)
    m1, m2, s2 = means.clone().requires_grad_(True), means.clone().requires_grad_(True), shs.clone().requires_grad_(True)
    c = sh_utils.sh_colors(s2, m2, rs.campos, deg)
    c_in = c.detach().requires_grad_(True)
    out, _ = rast(means3D=m1, shs=None, colors_precomp=c_in, **geom)
    assert torch.equal(out.detach(), img)
    (out * R).sum().backward()
    c.backward(c_in.grad)
    assert m1.grad.abs().sum() > 0 and m2.grad.abs().sum() > 0
    assert torch.equal(gm, m1.grad + m2.grad) and torch.equal(gs, s2.grad)
    # two runs, identical bits
    again = train()
    assert all(torch.equal(a, b) for a, b in zip(again, (img_t, radii_t, gm, gs)))


def test_rasteriser_no_grad_and_plain_tensors_take_the_inference_path():
    rast, rs, means, shs, geom = _frame("general", 3, 16)
    img, radii = rast(means3D=means, shs=shs, colors_precomp=None, **geom)           # nothing requires grad
    assert not img.requires_grad
    s = shs.clone().requires_grad_(True)
    with torch.no_grad():
        img2, _ = rast(means3D=means, shs=s, colors_precomp=None, **geom)
    assert not img2.requires_grad and torch.equal(img, img2)
    img3, _ = rast(means3D=means, shs=s, colors_precomp=None, **geom)
    assert img3.requires_grad and torch.equal(img3.detach(), img)


def test_it_fits_coefficients():
    """30 Adam steps on shs towards a picture rendered from other coefficients: the loss ends below a third of its start."""
    rast, rs, means, target_shs, geom = _frame("general", 2, 9)
    with torch.no_grad():
        target, _ = rast(means3D=means, shs=target_shs, colors_precomp=None, **geom)
    g = torch.Generator(device="cuda").manual_seed(0)
    shs = (target_shs + 0.3 * torch.randn(target_shs.shape, device="cuda", generator=g)).requires_grad_(True)
    opt = torch.optim.Adam([shs], lr=4e-2)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        img, _ = rast(means3D=means, shs=shs, colors_precomp=None, **geom)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("losses", losses[0], losses[-1])
    assert losses[-1] < losses[0] / 3, (losses[0], losses[-1])


def test_errors():
    from gauspcc_amd import sh_utils

    rast, rs, means, shs, geom = _frame("general", 3, 16)
    col = torch.zeros(N, 3, device="cuda")
    with pytest.raises(Exception, match="excatly one"):
        rast(means3D=means, shs=shs, colors_precomp=col, **geom)
    with pytest.raises(Exception, match="excatly one"):
        rast(means3D=means, shs=None, colors_precomp=None, **geom)
    with pytest.raises(ValueError, match="16"):                              # M too small for the degree
        rast(means3D=means, shs=shs[:, :15], colors_precomp=None, **geom)
    with pytest.raises(ValueError):                                          # wrong last dimension
        rast(means3D=means, shs=shs.transpose(1, 2), colors_precomp=None, **geom)
    with pytest.raises(ValueError):
        rast(means3D=means, shs=shs[:-1], colors_precomp=None, **geom)
    from gauspcc_amd.rasterizer import GaussianRasterizer

    with pytest.raises(ValueError, match="0..4"):                            # degree 5
        GaussianRasterizer(rs._replace(sh_degree=5))(means3D=means, shs=torch.zeros(N, 36, 3, device="cuda"), colors_precomp=None, **geom)
    with pytest.raises(ValueError, match="0..4"):
        sh_utils.eval_sh(5, torch.zeros(4, 3, 36, device="cuda"), torch.zeros(4, 3, device="cuda"))
    with pytest.raises(RuntimeError):                                        # CPU tensors: no CPU path
        rast(means3D=means.cpu(), shs=shs.cpu(), colors_precomp=None, **{k: (None if v is None else v.cpu()) for k, v in geom.items()})
    # degree 4 renders (the original stops at 3)
    img, _ = GaussianRasterizer(rs._replace(sh_degree=4))(means3D=means, shs=torch.randn(N, 25, 3, device="cuda"), colors_precomp=None, **geom)
    assert torch.isfinite(img).all()
