"""gauspcc_amd.triplane on the device against the float64 restatement of its contract (tests/triplane_ref.py).

Accuracy criterion (no tolerance fixed in advance): for each of output, plane gradient and coordinate gradient,
e_dev = max |device - float64| must not exceed 4 x e_t32 = max |float32 torch formula on the same GPU - float64| over the same elements.
The factor covers two equally valid float32 rounding orders (fused vs separate multiply-add) compared by a maximum over ~10^6 elements.
The coordinate gradient is discontinuous where a pixel coordinate crosses an integer: for that comparison only, samples whose float64
pixel coordinate lies within 1e-3 of an integer are left out (under 3 % of them: tests/test_triplane_ref_cpu.py)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triplane_ref as ref  # noqa: E402

CASES = ref.CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


def _planes(C, H, W, seed):
    return torch.randn(3, C, H, W, generator=torch.Generator().manual_seed(seed + 100), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs, the float64 reference (computed once, on the CPU) and the float32 torch formula's results on the GPU."""
    N, K, C, H, W, seed, cluster = case
    planes, co = _planes(C, H, W, seed), ref.make_coordinates(N, K, seed, cluster)
    go = torch.randn(N, K * 3 * C, generator=torch.Generator().manual_seed(seed + 200), dtype=torch.float32)
    mx, mn = ref.bounds()
    a64 = (planes.double(), co.double(), mx.double(), mn.double(), ref.RADII)
    out64 = ref.sample(*a64)
    gp64, gc64 = ref.closed_form_grads(*a64, go.double())
    p, c = planes.to(DEV).requires_grad_(True), co.to(DEV).requires_grad_(True)
    out32 = ref.torch_formula(p, c, mx.to(DEV), mn.to(DEV), ref.RADII)
    gp32, gc32 = torch.autograd.grad(out32, (p, c), go.to(DEV))
    keep = ~ref.near_texel_boundary(co, H, W)
    return dict(planes=planes, co=co, go=go, mx=mx, mn=mn, out64=out64, gp64=gp64, gc64=gc64, out32=out32.detach().cpu(), gp32=gp32.cpu(), gc32=gc32.cpu(),
                keep=keep)


def _device_run(d, repeat=None, co=None):
    from gauspcc_amd.triplane import triplane_sample

    p = d["planes"].to(DEV).requires_grad_(True)
    c = (d["co"] if co is None else co).to(DEV).requires_grad_(True)
    out = triplane_sample(p, c, d["mx"].to(DEV), d["mn"].to(DEV), ref.RADII, repeat=repeat)
    gp, gc = torch.autograd.grad(out, (p, c), d["go"].to(DEV))
    return out.detach(), gp, gc


def _err(a, b, keep=None):
    e = (a.double().cpu() - b).abs()
    return float((e if keep is None else e[keep]).max())


def _criterion(tag, dev, t32, want, keep=None):
    e_dev, e_t32 = _err(dev, want, keep), _err(t32, want, keep)
    print(f"{tag}: e_dev {e_dev:.3e}  e_t32 {e_t32:.3e}  ratio {e_dev / e_t32 if e_t32 else float('inf') if e_dev else 0.0:.2f}")
    return e_dev <= FACTOR * e_t32, (tag, e_dev, e_t32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-K%d-C%d-%dx%d" % c[:5])
def test_matches_float64_restatement(case):
    d = _case(case)
    out, gp, gc = _device_run(d)
    assert out.shape == d["out64"].shape and gp.shape == d["gp64"].shape and gc.shape == d["gc64"].shape
    checks = [_criterion("output", out, d["out32"], d["out64"]), _criterion("d planes", gp, d["gp32"], d["gp64"]),
              _criterion("d coordinates", gc, d["gc32"], d["gc64"], d["keep"])]
    assert all(ok for ok, _ in checks), [info for ok, info in checks if not ok]


def test_empty_input_returns_empty_without_a_launch():
    from gauspcc_amd import _lib, runtime
    from gauspcc_amd.triplane import triplane_sample

    mx, mn = ref.bounds(device=DEV)
    p = _planes(8, 16, 16, 0).to(DEV).requires_grad_(True)
    runtime.context(DEV)
    before = _lib.lib().gpcc_debug_launches(0)
    out = triplane_sample(p, torch.empty(0, 4, 3, device=DEV), mx, mn, ref.RADII)
    assert out.shape == (0, 4 * 3 * 8)
    out.sum().backward()
    assert _lib.lib().gpcc_debug_launches(0) == before
    assert p.grad.shape == p.shape and not p.grad.any()
    assert triplane_sample(p.detach(), torch.empty(0, 3, device=DEV), mx, mn, ref.RADII, repeat=4).shape == (0, 96)


def test_backward_is_bitwise_reproducible_also_across_streams():
    d = _case(CASES[1])          # 16 x 16, half the points in a tight cluster: runs longer than a sum chunk, across chunk borders
    _, gp0, gc0 = _device_run(d)
    _, gp1, gc1 = _device_run(d)
    assert torch.equal(gp0, gp1) and torch.equal(gc0, gc1)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    res = []
    torch.cuda.synchronize()
    for s in (s1, s2):           # enqueued back to back: the two backwards overlap on the device
        with torch.cuda.stream(s):
            res.append(_device_run(d))
    torch.cuda.synchronize()
    for _, gp, gc in res:
        assert torch.equal(gp, gp0) and torch.equal(gc, gc0)


def test_repeat_form_equals_the_materialised_call():
    N, K, C, H, W, seed, _ = CASES[3]
    d = dict(_case(CASES[3]))
    anchors = d["co"][:, 0, :].contiguous()
    mat = anchors.unsqueeze(1).repeat(1, K, 1)
    out_m, gp_m, gc_m = _device_run(d, co=mat)
    out_r, gp_r, gc_r = _device_run(d, repeat=K, co=anchors)
    assert torch.equal(out_r, out_m)
    assert gc_r.shape == (N, 3)
    _, gp_r2, gc_r2 = _device_run(d, repeat=K, co=anchors)
    assert torch.equal(gp_r, gp_r2) and torch.equal(gc_r, gc_r2)
    # the float64 reference and the float32 torch formula of the materialised samples
    mx, mn = d["mx"], d["mn"]
    gp64, gc64 = ref.closed_form_grads(d["planes"].double(), mat.double(), mx.double(), mn.double(), ref.RADII, d["go"].double())
    p, c = d["planes"].to(DEV).requires_grad_(True), mat.to(DEV).requires_grad_(True)
    gp32, gc32 = torch.autograd.grad(ref.torch_formula(p, c, mx.to(DEV), mn.to(DEV), ref.RADII), (p, c), d["go"].to(DEV))
    keep = ~ref.near_texel_boundary(anchors, H, W)
    checks = [_criterion("repeat d planes", gp_r, gp32.cpu(), gp64), _criterion("repeat d coordinates", gc_r, gc32.sum(1).cpu(), gc64.sum(1), keep),
              _criterion("materialised d planes", gp_m, gp32.cpu(), gp64)]
    assert all(ok for ok, _ in checks), [info for ok, info in checks if not ok]


def test_non_finite_rows_give_zeros_and_leave_the_rest_untouched():
    from gauspcc_amd import _lib, runtime

    d = dict(_case(CASES[1]))
    C = CASES[1][2]
    out0, gp0, gc0 = _device_run(d)
    co = d["co"].clone()
    bad = (5, 1777)
    co[bad[0]] = float("nan")
    co[bad[1]] = float("inf")
    co[40, 2, 1] = float("-inf")               # one sample of a row: the planes that read y
    go = d["go"].clone()
    d["go"] = go
    out, gp, gc = _device_run(d, co=co)
    for r in bad:
        assert not out[r].any() and not gc[r].any()
    o40 = out[40].view(4, 3, C)
    assert not o40[2, 0].any() and not o40[2, 2].any() and torch.equal(o40[2, 1], out0[40].view(4, 3, C)[2, 1])
    rest = torch.ones(co.shape[0], dtype=torch.bool)
    rest[[5, 1777, 40]] = False
    assert torch.equal(out[rest], out0[rest]) and torch.equal(gc[rest], gc0[rest])
    assert torch.isfinite(gp).all() and torch.isfinite(gc).all()
    # the plane gradient is the one of the finite samples alone: the reference with the bad samples moved to the origin and their
    # upstream gradient zeroed (the sorted order differs from a clean run's, so this is the accuracy criterion, not torch.equal)
    g2 = go.clone().view(-1, 4, 3, C)
    g2[5] = 0
    g2[1777] = 0
    g2[40, 2, 0] = 0
    g2[40, 2, 2] = 0
    g2 = g2.view(go.shape)
    clean = torch.where(torch.isfinite(co), co, torch.zeros_like(co))
    gp64, _ = ref.closed_form_grads(d["planes"].double(), clean.double(), d["mx"].double(), d["mn"].double(), ref.RADII, g2.double())
    p, c = d["planes"].to(DEV).requires_grad_(True), clean.to(DEV)
    gp32, = torch.autograd.grad(ref.torch_formula(p, c, d["mx"].to(DEV), d["mn"].to(DEV), ref.RADII), p, g2.to(DEV))
    ok, info = _criterion("non-finite d planes", gp, gp32.cpu(), gp64)
    assert ok, info
    torch.cuda.synchronize()
    assert _lib.lib().gpcc_device_error_check(runtime.context(DEV)) == 0


def test_sample_from_planes_has_the_reference_signature_and_shape():
    from gauspcc_amd.triplane import generate_planes, sample_from_planes, triplane_sample

    d = _case(CASES[4])
    N, K, C = CASES[4][:3]
    args = (d["planes"].to(DEV), d["co"].to(DEV), d["mx"].to(DEV), d["mn"].to(DEV))
    out = sample_from_planes(generate_planes(DEV), *args, box_warp=1, radii=ref.RADII)
    assert out.shape == (N, K, 3, C)
    assert torch.equal(out.reshape(N, -1), triplane_sample(*args, ref.RADII))
    # non-contiguous inputs are made contiguous
    pt = d["planes"].to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not pt.is_contiguous()
    assert torch.equal(triplane_sample(pt, *args[1:], ref.RADII), out.reshape(N, -1))


def test_module_modes_shapes_and_state_dict_from_the_restatement():
    from gauspcc_amd.triplane import Triplane

    torch.manual_seed(3)
    C, R, K, N = 6, 32, 4, 500
    theirs = ref.RefTriplane(C, R, 2 * ref.RADII).to(DEV)
    ours = Triplane(C, R, 2 * ref.RADII).to(DEV)
    ours.load_state_dict(theirs.state_dict())
    theirs.load_state_dict(ours.state_dict())
    co = ref.make_coordinates(N, K, 21).to(DEV)
    mx, mn = ref.bounds(device=DEV)
    out = ours(co, mx, mn)
    assert out.shape == (N, K * 3 * C)
    want = theirs(co, mx, mn)
    e = (out - want).abs().max().item()
    assert e <= 1e-6, e                                       # planes in +-1e-2: a float32 rounding of the weights is ~1e-9
    o, a, b = ours(co, mx, mn, is_training=1, step=12000)
    assert a is None and b is None and torch.equal(o, out)
    assert ours.get_encode().numel() == 0
    o, comp, rec = ours(co, mx, mn, is_training=1, step=15001)
    assert torch.equal(o, out) and comp.shape == (3, 8, R // 8, R // 8) and rec.shape == (3, C, R, R)
    assert ours.compressed_plane is comp and ours.get_encode() is comp
    assert ours(co[:, 0].contiguous(), mx, mn, repeat=K).shape == (N, K * 3 * C)


def test_short_optimisation_follows_torch_formula():
    from gauspcc_amd.triplane import triplane_sample

    g = torch.Generator().manual_seed(31)
    N, K, C, R, lr, steps = 2000, 2, 8, 32, 1e-2, 20
    mx, mn = ref.bounds(device=DEV)
    co0 = ((torch.rand(N, K, 3, generator=g) * 2 - 1) * 0.6).to(DEV)
    p0 = (torch.randn(3, C, R, R, generator=g) * 0.5).to(DEV)
    target = torch.randn(N, K * 3 * C, generator=g).to(DEV) * 0.5
    runs = []
    for formula in ("hip", "torch"):
        p, c = p0.clone().requires_grad_(True), co0.clone().requires_grad_(True)
        opt = torch.optim.Adam([p, c], lr=lr)
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            out = triplane_sample(p, c, mx, mn, ref.RADII) if formula == "hip" else ref.torch_formula(p, c, mx, mn, ref.RADII)
            loss = ((out - target) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        runs.append((p.detach(), c.detach(), losses))
    (ph, ch, lh), (pt, ct, lt) = runs
    print(f"losses hip {lh[0]:.6f} -> {lh[-1]:.6f}, torch -> {lt[-1]:.6f}; |d planes| mean {float((ph - pt).abs().mean()):.3e} max {float((ph - pt).abs().max()):.3e}; "
          f"|d coordinates| mean {float((ch - ct).abs().mean()):.3e} max {float((ch - ct).abs().max()):.3e}")
    assert lh[-1] < lh[0]
    assert abs(lh[-1] - lt[-1]) <= 1e-2 * lt[-1], (lh[-1], lt[-1])
    # As in test_gpu_ssim: Adam divides by sqrt(v), so a last-bit difference of a near-zero gradient, or a coordinate that crosses a
    # texel boundary one step earlier in one program, becomes a step of up to lr.  The runs agree to 5 % of one step on average; no
    # parameter can be further apart than the two programs can move it in opposite directions (2 lr per step).
    for a, b in ((ph, pt), (ch, ct)):
        dlt = (a - b).abs()
        assert float(dlt.mean()) <= 0.05 * lr and float(dlt.max()) <= 2 * lr * steps, (float(dlt.mean()), float(dlt.max()))


def test_tcgs_model_slice_runs_forward_and_backward():
    from gauspcc_amd.entropy_models import Entropy_gaussian
    from gauspcc_amd.synth import SyntheticGaussianModelTC

    m = SyntheticGaussianModelTC(3000, seed=2, resolution=64, tri_feat_dim=16, device=DEV)
    F, K = m.feat_dim, m.n_offsets
    assert m.knnanchor.shape == (3000, m.knn, 3)
    anchor = m.get_anchor
    ctx = m.triplane(m.knnanchor, m.x_bound_max, m.x_bound_min)
    assert ctx.shape == (3000, m.knn * 3 * m.tri_feat_dim)
    mean, scale, *_ = torch.split(m.get_tri_mlp(torch.cat([ctx, anchor], dim=1)), [F, F, 6, 6, 3 * K, 3 * K, 1, 1, 1], dim=-1)
    feat = m._anchor_feat.clone().requires_grad_(True)
    bits = Entropy_gaussian(Q=1)(feat, mean, torch.nn.functional.softplus(scale) + 1e-3, 1.0)
    bits.sum().backward()
    params = [m.triplane.planes, feat] + list(m.mlp_triplane.parameters())
    for p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert m.triplane.planes.grad.abs().sum() > 0
    torch.cuda.synchronize()
