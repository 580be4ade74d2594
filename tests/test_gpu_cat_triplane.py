"""gauspcc_amd.cat_triplane on the device against the float64 restatement of its contract (tests/cat_triplane_ref.py) and the reference's
recorded outputs (tests/golden/cat_triplane.npz).

Accuracy criterion (no tolerance fixed in advance), the one of tests/test_gpu_triplane.py: for each of output, plane gradients and
coordinate gradient, e_dev = max |device - float64| must not exceed 4 x e_t32 = max |float32 torch formula on the same GPU - float64| over
the same elements.  The coordinate gradient is discontinuous where a pixel coordinate crosses an integer: for that comparison only, the
points of cat_triplane_ref.near_texel_boundary are left out (at most 5 % of a case: tests/test_cat_triplane_ref_cpu.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arm_ref  # noqa: E402
import cat_triplane_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
ERR_ARG = -2     # GPCC_ERR_ARG
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cat_triplane.npz")
RUNS = [(c[0], level) for c in R.CASES for level in c[5]]


def _dev(xf):
    return {k: v.to(DEV) for k, v in xf.items()}


def _kw(xf, contract):
    return dict(contract=tuple(xf[k] for k in ("pca_mean", "rotation", "variance", "aabb", "con_aabb"))) if contract else dict(aabb=xf["aabb"])


@functools.lru_cache(maxsize=None)
def _inputs(name, contract):
    pts, grids, xf, shapes = R.make_case(name, contract)
    C, L = grids[0][0].shape[1], len(grids)
    go = torch.randn(pts.shape[0], L * 3 * C, generator=torch.Generator().manual_seed(77 + R.SEEDS[name]), dtype=torch.float32)
    return dict(pts=pts, grids=grids, xf=xf, shapes=shapes, go=go)


@functools.lru_cache(maxsize=None)
def _case(name, level, contract, quantise):
    """The float64 reference (computed once, on the CPU) and the float32 torch formula's results on the GPU."""
    d = dict(_inputs(name, contract))
    a64 = (d["pts"].double(), R.as64(d["grids"]), level, quantise, R.xf64(d["xf"]), contract)
    d["out64"] = R.sample(*a64)
    d["gp64"], d["gc64"] = R.closed_form_grads(*a64, d["go"].double())
    p = d["pts"].to(DEV).requires_grad_(not contract)
    gs = [[t.to(DEV).requires_grad_(True) for t in lv] for lv in d["grids"]]
    out32 = R.torch_formula(p, gs, level, quantise, _dev(d["xf"]), contract)
    leaves = [t for lv in gs for t in lv] + ([] if contract else [p])
    g32 = torch.autograd.grad(out32, leaves, d["go"].to(DEV), allow_unused=True)
    d["out32"] = out32.detach().cpu()
    d["gp32"] = [torch.zeros_like(t).cpu() if g is None else g.cpu() for g, t in zip(g32[:len(leaves) - (0 if contract else 1)], leaves)]
    d["gc32"] = None if contract else g32[-1].cpu()
    d["keep"] = ~R.near_texel_boundary(d["pts"], d["shapes"], d["xf"], contract)
    return d


def _device_run(d, level, contract, quantise, pts=None, go=None, grids=None):
    from gauspcc_amd.cat_triplane import ms_triplane_sample

    p = (d["pts"] if pts is None else pts).to(DEV).requires_grad_(not contract)
    gs = [[t.to(DEV).requires_grad_(True) for t in lv] for lv in (d["grids"] if grids is None else grids)]
    out = ms_triplane_sample(p, gs, level=level, quantise=quantise, **_kw(_dev(d["xf"]), contract))
    leaves = [t for lv in gs for t in lv] + ([] if contract else [p])
    g = torch.autograd.grad(out, leaves, (d["go"] if go is None else go).to(DEV))
    return out.detach(), list(g[:3 * len(gs)]), (None if contract else g[-1])


def _err(a, b, keep=None):
    e = (a.detach().double().cpu() - b).abs()
    return float((e if keep is None else e[keep]).max())


def _criterion(tag, dev, t32, want, keep=None):
    e_dev, e_t32 = _err(dev, want, keep), _err(t32, want, keep)
    print(f"{tag}: e_dev {e_dev:.3e}  e_t32 {e_t32:.3e}  ratio {e_dev / e_t32 if e_t32 else float('inf') if e_dev else 0.0:.2f}")
    return e_dev <= FACTOR * e_t32, (tag, e_dev, e_t32)


@pytest.mark.parametrize("quantise", [True, False], ids=["quantised", "raw"])
@pytest.mark.parametrize("contract", [True, False], ids=["contract", "plain"])
@pytest.mark.parametrize("name,level", RUNS, ids=[f"{n}-level{v}" for n, v in RUNS])
def test_matches_float64_restatement(name, level, contract, quantise):
    d = _case(name, level, contract, quantise)
    out, gp, gc = _device_run(d, level, contract, quantise)
    assert out.shape == d["out64"].shape and out.dtype == torch.float32
    checks = [_criterion("output", out, d["out32"], d["out64"])]
    for i, (g, g32, g64) in enumerate(zip(gp, d["gp32"], d["gp64"])):
        assert g.shape == d["grids"][i // 3][i % 3].shape
        checks.append(_criterion(f"d plane {i // 3}{i % 3}", g, g32, g64.reshape(g.shape)))
        if i // 3 and level <= i // 3:
            assert not g.any()                       # a level that `level` leaves out has no gradient
    if not contract:
        assert gc.shape == d["pts"].shape
        checks.append(_criterion("d pts", gc, d["gc32"], d["gc64"], d["keep"]))
    assert all(ok for ok, _ in checks), [info for ok, info in checks if not ok]


@pytest.mark.parametrize("contract", [True, False], ids=["contract", "plain"])
@pytest.mark.parametrize("name", ["odd", "cluster"])
def test_fused_quantiser_equals_planes_rounded_by_torch(name, contract):
    d = _inputs(name, contract)
    rounded = [[torch.round(t * 16) / 16 for t in lv] for lv in d["grids"]]
    out_q, gp_q, _ = _device_run(d, 2, contract, True)
    out_r, gp_r, _ = _device_run(d, 2, contract, False, grids=rounded)
    assert torch.equal(out_q, out_r)
    assert all(torch.equal(a, b) for a, b in zip(gp_q, gp_r))
    assert not torch.equal(out_q, _device_run(d, 2, contract, False)[0])


def test_backward_is_bitwise_reproducible_also_across_streams():
    d = _inputs("cluster", False)    # half the points inside one texel: runs longer than a sum chunk, across chunk borders
    _, gp0, gc0 = _device_run(d, 2, False, True)
    _, gp1, gc1 = _device_run(d, 2, False, True)
    assert all(torch.equal(a, b) for a, b in zip(gp0, gp1)) and torch.equal(gc0, gc1)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    res = []
    torch.cuda.synchronize()
    for s in (s1, s2):               # enqueued back to back: the two backwards overlap on the device
        with torch.cuda.stream(s):
            res.append(_device_run(d, 2, False, True))
    torch.cuda.synchronize()
    for _, gp, gc in res:
        assert all(torch.equal(a, b) for a, b in zip(gp, gp0)) and torch.equal(gc, gc0)


def test_empty_input_returns_empty_without_a_launch():
    from gauspcc_amd import _lib, runtime
    from gauspcc_amd.cat_triplane import ms_triplane_sample

    d = _inputs("odd", False)
    gs = [[t.to(DEV).requires_grad_(True) for t in lv] for lv in d["grids"]]
    runtime.context(DEV)
    before = _lib.lib().gpcc_debug_launches(0)
    out = ms_triplane_sample(torch.empty(0, 3, device=DEV), gs, aabb=d["xf"]["aabb"].to(DEV))
    assert out.shape == (0, 2 * 3 * 3)
    out.sum().backward()
    assert _lib.lib().gpcc_debug_launches(0) == before
    for lv in gs:
        for t in lv:
            assert t.grad.shape == t.shape and not t.grad.any()
    xf = _dev(_inputs("odd", True)["xf"])
    assert ms_triplane_sample(torch.empty(0, 3, device=DEV), [[t.detach() for t in lv] for lv in gs], **_kw(xf, True)).shape == (0, 18)
    # the C entry point itself zeroes the plane gradients of an empty call
    from gauspcc_amd.cat_triplane import NORMALIZE, _Plan
    from gauspcc_amd.runtime import ptrs
    plan = _Plan([tuple(t.shape[1:]) for lv in gs for t in lv], 2, False, NORMALIZE)
    gps = [torch.full_like(t, 7.0) for lv in gs for t in lv]
    rc = _lib.lib().gsge_msplane_backward(runtime.context(DEV), None, None, 0, *plan.args([t for lv in gs for t in lv], (None, None, None, None, None)),
                                          ptrs(gps), None, runtime.Workspace(DEV).fn(), None, runtime.stream_ptr(DEV))
    assert rc == 0 and _lib.lib().gpcc_debug_launches(0) == before
    torch.cuda.synchronize()
    assert all(not g.any() for g in gps)


def test_limits_are_refused_before_any_launch():
    from gauspcc_amd import _lib, runtime
    from gauspcc_amd.cat_triplane import CONTRACT, NORMALIZE, _Plan
    from gauspcc_amd.runtime import ptrs

    d = _inputs("odd", False)
    gs = [t.to(DEV) for lv in d["grids"] for t in lv]
    pts, aabb = d["pts"].to(DEV), d["xf"]["aabb"].to(DEV).reshape(-1)
    out = torch.empty(pts.shape[0], 18, device=DEV)
    ctx, L = runtime.context(DEV), _lib.lib()
    before = L.gpcc_debug_launches(0)
    shapes = [tuple(t.shape[1:]) for t in gs]

    def fwd(plan, n=pts.shape[0], xf=(None, None, None, aabb, None)):
        return L.gsge_msplane_forward(ctx, pts.data_ptr(), n, *plan.args(gs, xf), out.data_ptr(), runtime.Workspace(DEV).fn(), None, runtime.stream_ptr(DEV))

    bad_c, bad_h = _Plan(shapes, 2, False, NORMALIZE), _Plan([(3, 1, 5)] + shapes[1:], 2, False, NORMALIZE)
    bad_c.C = 257
    assert fwd(bad_c) == ERR_ARG and fwd(bad_h) == ERR_ARG
    assert fwd(_Plan(shapes, 2, False, NORMALIZE), n=(1 << 32) // 24 + 1) == ERR_ARG
    assert fwd(_Plan(shapes, 2, False, CONTRACT)) == ERR_ARG                       # contract without its tensors
    nine = _Plan(shapes, 2, False, NORMALIZE)
    nine.L = 9
    assert fwd(nine) == ERR_ARG
    # a coordinate gradient together with contract
    xf = _dev(_inputs("odd", True)["xf"])
    plan = _Plan(shapes, 2, False, CONTRACT)
    gps, gpts = [torch.empty_like(t) for t in gs], torch.empty_like(pts)
    rc = L.gsge_msplane_backward(ctx, out.data_ptr(), pts.data_ptr(), pts.shape[0],
                                 *plan.args(gs, tuple(xf[k].reshape(-1) for k in ("pca_mean", "rotation", "variance", "aabb", "con_aabb"))),
                                 ptrs(gps), gpts.data_ptr(), runtime.Workspace(DEV).fn(), None, runtime.stream_ptr(DEV))
    assert rc == ERR_ARG
    assert L.gpcc_debug_launches(0) == before


def test_point_at_the_pca_origin_gives_a_zero_row_and_no_gradient():
    from gauspcc_amd import _lib, runtime

    d = _inputs("odd", True)
    out0, gp0, _ = _device_run(d, 2, True, True)
    pts = torch.cat([d["pts"][:20], d["xf"]["pca_mean"][None], d["pts"][20:]])          # p = pts - pca_mean = 0: 1 / mag = inf
    go = torch.cat([d["go"][:20], torch.full((1, d["go"].shape[1]), 3.0), d["go"][20:]])
    out, gp, _ = _device_run(d, 2, True, True, pts=pts, go=go)
    assert not out[20].any()
    rest = torch.ones(pts.shape[0], dtype=torch.bool)
    rest[20] = False
    assert torch.equal(out[rest], out0)
    # the same (row, slot) order among the contributing entries: the plane gradients keep their bits
    assert all(torch.equal(a, b) for a, b in zip(gp, gp0))
    # a NaN coordinate on the normalize_aabb path: a zero row, zero coordinate gradient
    e = _inputs("odd", False)
    bad = e["pts"].clone()
    bad[5, 1] = float("nan")
    bad[9, 0] = float("inf")
    o0, g0, c0 = _device_run(e, 2, False, False)
    o1, g1, c1 = _device_run(e, 2, False, False, pts=bad)
    keep = torch.ones(bad.shape[0], dtype=torch.bool)
    keep[[5, 9]] = False
    assert not o1[5].any() and not o1[9].any() and not c1[5].any() and not c1[9].any()
    assert torch.equal(o1[keep], o0[keep]) and torch.equal(c1[keep], c0[keep])
    assert all(torch.isfinite(g).all() for g in g1)
    torch.cuda.synchronize()
    assert _lib.lib().gpcc_device_error_check(runtime.context(DEV)) == 0


def test_degenerate_aabb_gives_zero_rows_and_zero_gradients():
    d = dict(_inputs("odd", False))
    d["xf"] = {"aabb": torch.tensor([[2.0, 2.0, 2.0], [2.0, -2.0, -2.0]])}      # no extent along x: 2 / 0 in the scale, g is not finite
    out, gp, gc = _device_run(d, 2, False, False)
    assert not out.any() and not gc.any() and torch.isfinite(gc).all()
    assert all(not g.any() for g in gp)


def test_other_transforms_and_interpolate_ms_features():
    from gauspcc_amd.cat_triplane import interpolate_ms_features, ms_triplane_sample

    d = _inputs("three", False)
    gs = [[t.to(DEV) for t in lv] for lv in d["grids"]]
    xf = _dev(d["xf"])
    pts = d["pts"].to(DEV)
    want = ms_triplane_sample(pts, gs, level=1, **_kw(xf, False))
    g = R.to_unit_box(pts, xf["aabb"])
    assert torch.equal(interpolate_ms_features(g, gs, 2, True, None, level=1), want)
    assert torch.equal(interpolate_ms_features(g.view(3, 100, 3), gs, 2, True, None), want)
    assert torch.equal(interpolate_ms_features(g, gs, 2, True, 2, level=3), ms_triplane_sample(pts, gs[:2], level=3, **_kw(xf, False)))
    # non-contiguous and [C, H, W] planes
    odd = [[t[0].permute(0, 2, 1).contiguous().permute(0, 2, 1) for t in lv] for lv in gs]
    assert not odd[0][0].is_contiguous()
    assert torch.equal(ms_triplane_sample(pts, odd, level=1, **_kw(xf, False)), want)
    # con_normalize_aabb alone, on points that are contracted already
    c = _inputs("three", True)
    cx = _dev(c["xf"])
    y = torch.rand(300, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    got = ms_triplane_sample(y, gs, contract=dict(aabb=cx["aabb"], con_aabb=cx["con_aabb"]))
    assert torch.equal(got, interpolate_ms_features(R.contracted_to_box(y, cx["aabb"], cx["con_aabb"]), gs, 2, True, None, level=2))


# ------------------------------------------------------------------ the module against the reference's recorded outputs
@functools.lru_cache(maxsize=None)
def _z():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _field(path, comp_iter=10):
    from gauspcc_amd.cat_triplane import TriPlaneField

    z = _z()
    config = {"grid_dimensions": 2, "input_coordinate_dim": 3, "output_coordinate_dim": 3, "resolution": [5, 7, 3]}
    field = TriPlaneField(1.0, config, [1, 2], path == "con", comp_iter, device=DEV)
    sd = {k: v.clone() for k, v in field.state_dict().items()}
    for l in range(2):
        for p in range(3):
            sd[f"grids.{l}.{p}"] = torch.as_tensor(z[f"plane_{l}_{p}"])
    for j, k in enumerate(k for k in sd if k.startswith("arm")):
        sd[k] = torch.as_tensor(z[f"arm_{j}"])
    names = {"aabb": "aabb", "rotation": "rotation_matrix", "pca_mean": "pca_mean", "variance": "variance", "con_aabb": "con_aabb"}
    for k, name in names.items():
        if f"{path}_{k}" in z:
            sd[name] = torch.as_tensor(z[f"{path}_{k}"])
    field.load_state_dict(sd)
    return field


def _bits64():
    z = _z()
    return sum(float(arm_ref.forward64([np.round(z[f"plane_{l}_{p}"] * 16) for l in range(2)], [z[f"arm_{10 * p + j}"] for j in range(10)])["rate"].sum())
               for p in range(3))


@pytest.mark.parametrize("path", ["con", "pln"])
def test_field_reproduces_the_reference(path):
    """The yardstick here is the reference's own float32 error against the float64 restatement: e_dev <= 4 x e_ref."""
    z = _z()
    field, contract = _field(path), path == "con"
    pts = torch.as_tensor(z[f"{path}_pts"]).to(DEV)
    grids = [[torch.as_tensor(z[f"plane_{l}_{p}"]) for p in range(3)] for l in range(2)]
    xf = {k: torch.as_tensor(z[f"{path}_{k}"]) for k in (("pca_mean", "rotation", "variance", "aabb", "con_aabb") if contract else ("aabb",))}
    w = torch.as_tensor(z["w"])
    checks = []
    for tag, itr in (("q", -1), ("r", 3)):
        field.zero_grad()
        feat, bits = field(pts, itr=itr)
        (feat * w.to(DEV)).sum().backward()
        a64 = (pts.cpu().double(), R.as64(grids), 2, tag == "q", R.xf64(xf), contract)
        out64 = R.sample(*a64)
        gp64, _ = R.closed_form_grads(*a64, w.double())
        checks.append(_criterion(f"{tag} features", feat.detach(), torch.as_tensor(z[f"{path}_{tag}_feat"]), out64))
        for i in range(6):
            l, p = divmod(i, 3)
            checks.append(_criterion(f"{tag} d plane {l}{p}", field.grids[l][p].grad, torch.as_tensor(z[f"{path}_{tag}_gp{l}{p}"]), gp64[i].reshape(grids[l][p].shape)))
        if tag == "q":
            want = _bits64()
            e_dev, e_ref = abs(float(bits.detach()) - want), abs(float(z[f"{path}_q_bits"]) - want)
            print(f"total_bits: device {float(bits.detach()):.6f}  reference {float(z[f'{path}_q_bits']):.6f}  float64 {want:.6f}")
            assert e_dev <= FACTOR * e_ref, (e_dev, e_ref)
            assert field.total_bits is bits
        else:
            assert isinstance(bits, int) and bits == 0
    assert all(ok for ok, _ in checks), [info for ok, info in checks if not ok]
    # get_density takes the points behind forward's PCA step and contraction
    x = pts
    if contract:
        x = field.contract_to_unisphere(torch.matmul(x - field.pca_mean, field.rotation_matrix) / field.variance,
                                        torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], device=DEV))
    feat, _ = field.get_density(x, itr=-1)
    ok, info = _criterion("get_density", feat, torch.as_tensor(z[f"{path}_q_feat"]), R.sample(pts.cpu().double(), R.as64(grids), 2, True, R.xf64(xf), contract))
    assert ok, info


def test_training_noise_is_drawn_in_the_reference_order():
    from gauspcc_amd.arm import arm_rate

    field = _field("con", comp_iter=10)
    pts = torch.as_tensor(_z()["con_pts"]).to(DEV)
    torch.manual_seed(123)
    _, bits = field(pts, itr=11)
    torch.manual_seed(123)
    sent = ([], [], [])
    for level in field.grids:                       # level by level, plane by plane, one rand_like per latent
        for ii, latent in enumerate(level):
            y = latent.detach() * 16
            sent[ii].append(y + (torch.rand_like(y) - 0.5))
    want = arm_rate(sent[0], field.arm) + arm_rate(sent[1], field.arm2) + arm_rate(sent[2], field.arm3)
    assert torch.equal(bits.detach(), want.detach())
    assert bits.requires_grad
    bits.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for lv in field.grids for p in lv)
    assert field.arm.mlp[0].w.grad is not None
    # at evaluation time the rounding passes the gradient unchanged, as the reference's quantiser does
    field.zero_grad()
    _, rounded_bits = field(pts, itr=-1)
    rounded_bits.backward()
    assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for lv in field.grids for p in lv)
    # another order of the draws gives another rate
    torch.manual_seed(123)
    swapped = ([], [], [])
    for ii in range(3):
        for level in field.grids:
            y = level[ii].detach() * 16
            swapped[ii].append(y + (torch.rand_like(y) - 0.5))
    other = arm_rate(swapped[0], field.arm) + arm_rate(swapped[1], field.arm2) + arm_rate(swapped[2], field.arm3)
    assert not torch.equal(other.detach(), want.detach())


def test_bitstream_round_trip_accepts_the_field(tmp_path):
    from gauspcc_amd.arm_codec import decode_triplane, encode_triplane

    field = _field("con")
    info, nbytes = encode_triplane(field, str(tmp_path))
    assert len(info) == 3 and nbytes > 0
    back = decode_triplane(field, str(tmp_path), info)
    assert len(back) == 2
    for level, dec in zip(field.grids, back):
        for p in range(3):
            assert torch.equal(dec[p], torch.round(level[p].detach() * 16) / 16)
    field.save_latent(str(tmp_path), 7)
    saved = torch.load(os.path.join(str(tmp_path), "grids_hat_7.pth"))
    assert torch.equal(saved[1][2], torch.round(field.grids[1][2] * 16))
