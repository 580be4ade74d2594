"""gsr_wavelet_l1_forward / gsr_wavelet_l1_backward (gauspcc_amd.loss_utils.wavelet_loss) and gsr_haar_forward / gsr_haar_inverse
(gauspcc_amd.wavelets) on the device: values and both gradients against the float64 restatement (tests/wavelet_ref.py) with the
project's bound e_dev <= 4 e_t32 + 1e-6 scale, e_t32 the float32 conv2d program's own error on the same inputs and scale the largest
|expected|; what the reference's own wavelet_loss recorded (tests/golden/wavelet.npz); the modules' shapes, band order, sign, adjoint and
inverse; bitwise repeatability; edge cases and errors.

Gradients are sums of sign(difference coefficient) terms, so they are compared where no coefficient is within 1e-5 of zero in float64:
the small shapes use wavelet_ref.pick_seed (no such coefficient at all), the larger ones leave out the 4 x 4 blocks that hold one."""
import os

import numpy as np
import pytest
import torch

from gauspcc_amd import loss_utils, wavelets
from gauspcc_amd.loss_utils import photometric_loss, tcgs_photometric_loss, wavelet_loss
from tests import wavelet_ref as wr

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(3, 1, 1), (3, 2, 3), (3, 5, 6), (3, 13, 18), (3, 24, 32), (3, 37, 41), (1, 9, 7)]
STEPS = [0, 12000, 25001]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavelet.npz")
_id = lambda s: "x".join(map(str, s))   # noqa: E731


def _err(a, ref):
    return float((a.detach().double().cpu() - ref.detach().double().cpu()).abs().max())


def _holds(dev, t32, ref, what, mask=None):
    """e_dev <= 4 e_t32 + 1e-6 scale over the entries of `mask` (all without one)."""
    dev, t32, ref = (t.detach().double().cpu() for t in (dev, t32, ref))
    if mask is not None:
        dev, t32, ref = dev[mask], t32[mask], ref[mask]
    e_dev, e_t32, scale = float((dev - ref).abs().max()), float((t32 - ref).abs().max()), float(ref.abs().max())
    assert e_dev <= 4 * e_t32 + 1e-6 * scale, (what, e_dev, e_t32, scale)


def _device_run(x, y, step):
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    v = wavelet_loss(a, b, step)
    assert v.shape == () and v.dtype == torch.float32
    v.backward()
    return v.detach(), a.grad, b.grad


def _compare(x, y, step, mask=None):
    """x, y on the device: the drop-in's value and gradients against float64 (CPU), calibrated by the float32 program on the device."""
    r = wr.grads(lambda a, b: wr.wavelet_loss64(a, b, step)[0], x.cpu(), y.cpu(), torch.float64)
    t = wr.grads(lambda a, b: wr.wavelet_loss(a, b, step), x, y, torch.float32)
    d = _device_run(x, y, step)
    _holds(d[0], t[0], r[0], "value")
    _holds(d[1], t[1], r[1], "grad1", mask)
    _holds(d[2], t[2], r[2], "grad2", mask)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_against_float64(shape, step):
    x, y = wr.make_images(shape, wr.pick_seed(shape), device=DEV)
    _compare(x, y, step)


@pytest.mark.parametrize("step", [12000, 25001])
def test_larger_shape_many_workgroups(step):
    shape = (3, 260, 410)                                  # 20 085 blocks: 79 workgroups, rows not a multiple of 4 wide
    x, y = wr.make_images(shape, 0)
    unsafe = wr.unsafe_pixels(x, y)
    share = float(unsafe.float().mean())
    assert share <= 0.01, share
    _compare(x.to(DEV), y.to(DEV), step, mask=~unsafe)


def test_larger_shape_vector_path():
    shape = (3, 258, 412)                                  # rows are whole float4s, the last block row is cut
    x, y = wr.make_images(shape, 0)
    unsafe = wr.unsafe_pixels(x, y)
    assert float(unsafe.float().mean()) <= 0.01
    _compare(x.to(DEV), y.to(DEV), 12000, mask=~unsafe)


def test_full_size_value_and_bands():
    x, y = wr.make_images((3, 1060, 1600), 0)
    v64, b64 = wr.wavelet_loss64(x, y, 12000)
    x, y = x.to(DEV), y.to(DEV)
    with torch.no_grad():
        v32 = wr.wavelet_loss(x, y, 12000)
        t = wr.DWTForward(J=2, wave="haar", mode="zero")
        b32 = torch.stack(wr.band_l1(*t(x.unsqueeze(0)), *t(y.unsqueeze(0))))
    weights = loss_utils.wavelet_weights(12000)
    assert weights == wr.band_weights(12000)
    loss, bands = loss_utils._wavelet_forward(x, y, weights)
    _holds(loss[0], v32, v64, "value")
    for k in range(7):
        _holds(bands[k], b32[k], b64[k], f"band {k}")
    assert torch.equal(wavelet_loss(x, y, 12000), loss[0])


def test_reference_fixture():
    g = np.load(GOLDEN)
    for shape in [(3, 24, 32), (3, 13, 18), (3, 37, 41)]:
        name = _id(shape)
        x, y = torch.tensor(g[f"{name}_img1"]).to(DEV), torch.tensor(g[f"{name}_img2"]).to(DEV)
        for step in (0, 12000, 25000, 25001, 30000):
            k = f"{name}_s{step}"
            v, d1, d2 = _device_run(x, y, step)
            ref = float(g[f"{k}_value"])
            e_t32 = abs(float(g[f"{k}_value32"]) - ref)
            assert abs(float(v) - ref) <= 4 * e_t32 + 1e-6 * abs(ref), (k, float(v), ref, e_t32)
            for d, gname, e_t32 in ((d1, "grad1", g[f"{k}_grad32_err"][0]), (d2, "grad2", g[f"{k}_grad32_err"][1])):
                want = g[f"{k}_{gname}"]
                e_dev = np.abs(d.double().cpu().numpy() - want).max()
                assert e_dev <= 4 * e_t32 + 1e-6 * np.abs(want).max(), (k, gname, e_dev, e_t32)


# ------------------------------------------------------------------ the modules
@pytest.mark.parametrize("shape", [(2, 3, 13, 18), (1, 3, 37, 41)], ids=_id)
def test_dwt_forward_shapes_band_order_and_sign(shape):
    x = wr.make_images(shape, 2, device=DEV)[0]
    for J in (1, 2, 3):
        xfm = wavelets.DWTForward(J=J, wave="haar", mode="zero").to(DEV)
        assert not list(xfm.parameters()) and not list(xfm.buffers())
        yl, yh = xfm(x)
        rl, rh = wr.dwt_quads(x.double().cpu(), J)
        tl, th = wr.dwt_conv(x, J)
        assert isinstance(yh, list) and len(yh) == J
        assert yl.shape == rl.shape and yl.dtype == torch.float32
        _holds(yl, tl, rl, ("Yl", J))
        for j in range(J):
            assert yh[j].shape == rh[j].shape and yh[j].dim() == 5 and yh[j].shape[2] == 3
            for k in range(3):
                _holds(yh[j][:, :, k], th[j][:, :, k], rh[j][:, :, k], ("Yh", J, j, k))
    # the bands are far apart, so the bound above tells them and their signs apart
    assert float((rh[0][:, :, 0] - rh[0][:, :, 1]).abs().max()) > 1e-2 and float(rh[0].abs().max()) > 1e-2


def test_dwt_adjoint_inverse_none_and_crop():
    shape = (1, 3, 37, 41)                                 # 37 x 41 -> 19 x 21 -> 10 x 11 -> 5 x 6: odd at two levels
    x = wr.make_images(shape, 3, device=DEV)[0]
    xfm, ifm = wavelets.DWTForward(J=3, wave="db1"), wavelets.DWTInverse(wave="haar", mode="zero")
    a = x.clone().requires_grad_(True)
    yl, yh = xfm(a)
    gen = torch.Generator().manual_seed(4)
    ul = torch.randn(yl.shape, generator=gen).to(DEV)
    uh = [torch.randn(h.shape, generator=gen).to(DEV) for h in yh]
    lhs = (yl * ul).sum() + sum((h * u).sum() for h, u in zip(yh, uh))
    lhs.backward()
    rhs = (x.double() * a.grad.double()).sum()
    assert abs(float(lhs.detach().double()) - float(rhs)) <= 1e-5 * max(abs(float(rhs)), 1.0)
    # the transpose is the inverse, cropped: DWT^T u = DWTInverse(u)[..., :H, :W]
    back = ifm((ul, uh))
    assert back.shape == (1, 3, 38, 42)
    assert float((back[..., :37, :41] - a.grad).abs().max()) <= 1e-5 * float(a.grad.abs().max())
    # the inverse's own backward is the forward
    cl, ch = ul.clone().requires_grad_(True), [u.clone().requires_grad_(True) for u in uh]
    w = torch.randn(back.shape, generator=gen).to(DEV)
    (ifm((cl, ch)) * w).sum().backward()
    fl, fh = wavelets.DWTForward(J=3)(w)                   # 38 x 42 -> 19 x 21 -> 10 x 11 -> 5 x 6
    assert float((cl.grad - fl).abs().max()) <= 1e-5 * float(fl.abs().max())
    for c, f in zip(ch, fh):
        assert c.grad.shape == f.shape and float((c.grad - f).abs().max()) <= 1e-5 * float(f.abs().max())
    # round trip, against the conv2d program too (it crops the low band the same way)
    with torch.no_grad():
        yl, yh = xfm(x)
        rec = ifm((yl, yh))
        assert rec.shape == (1, 3, 38, 42) and float((rec[..., :37, :41] - x).abs().max()) <= 1e-6
        assert float((rec - wr.idwt_conv(yl, yh)).abs().max()) <= 1e-6
        # None stands for zeros
        some = ifm((yl, [yh[0], yh[1], None]))
        want = wr.idwt_conv(yl, [yh[0], yh[1], torch.zeros_like(yh[2])])
        assert some.shape == want.shape == (1, 3, 38, 42) and float((some - want).abs().max()) <= 1e-6
        # as in the package, a None level has the low band's size: nothing says that 20 x 22 was 19 x 21
        some = ifm((yl, [None, yh[1], None]))
        want = wr.idwt_conv(yl, [torch.zeros(1, 3, 3, 20, 22, device=DEV), yh[1], torch.zeros_like(yh[2])])
        assert some.shape == want.shape == (1, 3, 40, 44) and float((some - want).abs().max()) <= 1e-6
        for shape2 in ((2, 3, 13, 18), (1, 1, 1, 1), (1, 2, 8, 12)):
            z = wr.make_images(shape2, 5, device=DEV)[1]
            for J in (1, 2):
                r = ifm(wavelets.DWTForward(J=J, wave="haar")(z))
                assert float((r[..., : shape2[-2], : shape2[-1]] - z).abs().max()) <= 1e-6, (shape2, J)


def test_import_drop_in():
    """The reference's formula with gauspcc_amd.wavelets.DWTForward in place of the package's equals the fused loss."""
    xfm = wavelets.DWTForward(J=2, mode="zero", wave="haar").to("cuda")
    for shape in [(3, 13, 18), (3, 24, 32), (3, 37, 41)]:
        x, y = wr.make_images(shape, wr.pick_seed(shape), device=DEV)
        for step in STEPS:
            r = wr.grads(lambda a, b: wr.wavelet_loss64(a, b, step)[0], x.cpu(), y.cpu(), torch.float64)
            t = wr.grads(lambda a, b: wr.wavelet_loss(a, b, step), x, y, torch.float32)
            m = wr.grads(lambda a, b: wr.wavelet_loss(a, b, step, xfm=xfm), x, y, torch.float32)
            d = _device_run(x, y, step)
            for i, what in enumerate(("value", "grad1", "grad2")):
                _holds(m[i], t[i], r[i], ("modules", what))
                e, e_t32, scale = _err(m[i], d[i]), _err(t[i], r[i]), float(r[i].abs().max())
                assert e <= 4 * e_t32 + 1e-6 * scale, (shape, step, what, e, e_t32)


# ------------------------------------------------------------------ behaviour
def test_bitwise_repeatable_and_across_streams():
    x, y = wr.make_images((3, 260, 410), 1, device=DEV)
    ref = _device_run(x, y, 12000)
    for u, v in zip(ref, _device_run(x, y, 12000)):
        assert torch.equal(u, v)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    torch.cuda.synchronize()
    for i in range(4):
        with torch.cuda.stream(s1 if i % 2 == 0 else s2):
            outs.append(_device_run(x, y, 12000))
    torch.cuda.synchronize()
    for o in outs:
        for u, v in zip(ref, o):
            assert torch.equal(u, v)
    assert torch.equal(ref[2], -ref[1])


def test_identical_images_give_zero_and_zero_gradient():
    x = wr.make_images((3, 37, 41), 0, device=DEV)[0]
    for step in STEPS:
        v, d1, d2 = _device_run(x, x.clone(), step)
        assert float(v) == 0.0
        assert torch.equal(d1, torch.zeros_like(x)) and torch.equal(d2, torch.zeros_like(x))


def test_gradients_are_exact_negatives_and_one_sided():
    x, y = wr.make_images((3, 37, 41), 0, device=DEV)
    v, d1, d2 = _device_run(x, y, 25001)
    assert torch.equal(d2, -d1) and bool(d1.any())
    a = x.clone().requires_grad_(True)
    wavelet_loss(a, y, 25001).backward()
    assert torch.equal(a.grad, d1)
    b = y.clone().requires_grad_(True)
    wavelet_loss(x, b, 25001).backward()
    assert torch.equal(b.grad, d2)
    a = x.clone().requires_grad_(True)
    (3.0 * wavelet_loss(a, y, 25001)).backward()
    assert float((a.grad - 3.0 * d1).abs().max()) <= 1e-6 * float(d1.abs().max())


def test_non_contiguous_and_no_grad():
    x, y = wr.make_images((3, 24, 32), 1, device=DEV)
    wide = torch.cat([x, torch.ones_like(x)], dim=2)       # (3, 24, 64): its left half is x, not contiguous
    view = wide[..., :32]
    assert not view.is_contiguous()
    assert torch.equal(wavelet_loss(view, y), wavelet_loss(x, y))
    a = wide.clone().requires_grad_(True)
    wavelet_loss(a[..., :32], y, 12000).backward()
    assert torch.equal(a.grad[..., :32], _device_run(x, y, 12000)[1]) and not a.grad[..., 32:].any()
    with torch.no_grad():
        v = wavelet_loss(x.clone().requires_grad_(True), y)
    assert not v.requires_grad and torch.equal(v, wavelet_loss(x, y))
    yl, yh = wavelets.DWTForward(J=2)(view.unsqueeze(0))
    rl, rh = wavelets.DWTForward(J=2)(x.unsqueeze(0))
    assert torch.equal(yl, rl) and all(torch.equal(u, v) for u, v in zip(yh, rh))


def test_tcgs_photometric_loss_equals_its_parts():
    x, y = wr.make_images((3, 123, 211), 2, device=DEV)
    for lam, wav, step in ((0.2, 0.02, 0), (0.35, 0.1, 25001)):
        a = x.clone().requires_grad_(True)
        loss, l1, sv, wv = tcgs_photometric_loss(a, y, lam, wav, step)
        assert loss.requires_grad and not (l1.requires_grad or sv.requires_grad or wv.requires_grad)
        base, l1b, svb = photometric_loss(x, y, lam)
        assert torch.equal(l1, l1b) and torch.equal(sv, svb) and torch.equal(wv, wavelet_loss(x, y, step))
        assert torch.equal(loss.detach(), base + wav * wv)
        loss.backward()
        b = x.clone().requires_grad_(True)
        (photometric_loss(b, y, lam)[0] + wav * wavelet_loss(b, y, step)).backward()
        assert torch.equal(a.grad, b.grad)
    assert torch.equal(tcgs_photometric_loss(x, y)[0], photometric_loss(x, y)[0] + 0.02 * wavelet_loss(x, y))


def test_errors():
    x, y = wr.make_images((3, 16, 16), 0, device=DEV)
    with pytest.raises(TypeError):
        wavelet_loss(x.double(), y.double())
    with pytest.raises(TypeError):
        wavelet_loss(x.half(), y)
    with pytest.raises(RuntimeError):
        wavelet_loss(x.cpu(), y.cpu())
    with pytest.raises(ValueError):
        wavelet_loss(x, y[:, :8])
    with pytest.raises(ValueError):
        wavelet_loss(x.unsqueeze(0), y.unsqueeze(0))
    for kw in ({"wave": "db2"}, {"mode": "symmetric"}, {"wave": "bior2.2", "mode": "periodization"}):
        with pytest.raises(NotImplementedError, match="served: (haar|zero)"):
            wavelets.DWTForward(J=2, **kw)
        with pytest.raises(NotImplementedError, match="served: (haar|zero)"):
            wavelets.DWTInverse(**kw)
    xfm = wavelets.DWTForward(J=1)
    with pytest.raises(TypeError):
        xfm(x.unsqueeze(0).double())
    with pytest.raises(RuntimeError):
        xfm(x.unsqueeze(0).cpu())
    with pytest.raises(ValueError):
        xfm(x)
    with pytest.raises(ValueError):
        wavelets.DWTInverse()((x.unsqueeze(0), [torch.zeros(1, 3, 3, 9, 9, device=DEV)]))
