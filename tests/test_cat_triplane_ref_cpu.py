"""tests/cat_triplane_ref.py against the reference's recorded outputs (tests/golden/cat_triplane.npz), the conditions the test inputs have
to meet, and what gauspcc_amd.cat_triplane does without a GPU (state dict, construction on the CPU, argument errors).

Accuracy criterion, the project's usual one: the reference's float32 result may be as far from the float64 restatement as 4 x the float32
torch formula of cat_triplane_ref (the same sequence written by us, run on the same CPU) is on the same elements."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arm_ref  # noqa: E402
import cat_triplane_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cat_triplane.npz")
FACTOR = 4.0
XF_KEYS = {"con": ("pca_mean", "rotation", "variance", "aabb", "con_aabb"), "pln": ("aabb",)}
CONFIG = {"grid_dimensions": 2, "input_coordinate_dim": 3, "output_coordinate_dim": 3, "resolution": [5, 7, 3]}


@functools.lru_cache(maxsize=None)
def _z():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _golden(path):
    z = _z()
    grids = [[torch.as_tensor(z[f"plane_{l}_{p}"]) for p in range(3)] for l in range(2)]
    xf = {k: torch.as_tensor(z[f"{path}_{k}"]) for k in XF_KEYS[path]}
    return torch.as_tensor(z[f"{path}_pts"]), grids, xf, torch.as_tensor(z["w"])


def _err(a, b):
    return float((torch.as_tensor(a).double() - b).abs().max())


def _criterion(tag, got, t32, want):
    e_got, e_t32 = _err(got, want), _err(t32, want)
    print(f"{tag}: e_ref {e_got:.3e}  e_t32 {e_t32:.3e}  ratio {e_got / e_t32 if e_t32 else float('inf') if e_got else 0.0:.2f}")
    return e_got <= FACTOR * e_t32, (tag, e_got, e_t32)


@pytest.mark.parametrize("path", ["con", "pln"])
@pytest.mark.parametrize("tag", ["q", "r"])
def test_restatement_reproduces_the_reference(path, tag):
    z = _z()
    pts, grids, xf, w = _golden(path)
    contract, quantise = path == "con", tag == "q"
    # the generator's inputs are the ones cat_triplane_ref makes today
    pts_now, grids_now, xf_now, _ = R.make_case("odd", contract)
    assert torch.equal(pts, pts_now) and all(torch.equal(a, b) for la, lb in zip(grids, grids_now) for a, b in zip(la, lb))
    assert all(torch.equal(xf[k], xf_now[k]) for k in xf)
    a64 = (pts.double(), R.as64(grids), 2, quantise, R.xf64(xf), contract)
    out64 = R.sample(*a64)
    gp64, gpts64 = R.closed_form_grads(*a64, w.double())
    p32 = pts.clone().requires_grad_(not contract)
    g32 = [[p.clone().requires_grad_(True) for p in level] for level in grids]
    out32 = R.torch_formula(p32, g32, 2, quantise, xf, contract)
    leaves = [p for level in g32 for p in level] + ([] if contract else [p32])
    grads32 = torch.autograd.grad(out32, leaves, w)
    checks = [_criterion("features", z[f"{path}_{tag}_feat"], out32.detach(), out64)]
    for i in range(6):
        l, p = divmod(i, 3)
        checks.append(_criterion(f"d plane {l}{p}", z[f"{path}_{tag}_gp{l}{p}"], grads32[i], gp64[i].reshape(grads32[i].shape)))
    if not contract:
        keep = ~R.near_texel_boundary(pts, R.plane_shapes((5, 7, 3), (1, 2)), xf, contract)
        checks.append(_criterion("d pts", z[f"{path}_{tag}_gpts"][keep.numpy()], grads32[6][keep], gpts64[keep]))
    assert all(ok for ok, _ in checks), [info for ok, info in checks if not ok]
    if tag == "r":
        assert int(z[f"{path}_r_zero"]) == 0


def test_total_bits_is_the_arm_rate_of_the_rounded_planes():
    z = _z()
    assert float(z["con_q_bits"]) == float(z["pln_q_bits"])        # the rate does not depend on the points
    bits64, bits32 = 0.0, torch.zeros((), dtype=torch.float32)
    for p in range(3):
        params = [z[f"arm_{10 * p + j}"] for j in range(10)]
        levels = [np.round(z[f"plane_{l}_{p}"] * 16) for l in range(2)]
        bits64 += float(arm_ref.forward64(levels, params)["rate"].sum())
        bits32 = bits32 + arm_ref.rate_torch([torch.as_tensor(y) for y in levels], [torch.as_tensor(v) for v in params])[0].sum()
    e_ref, e_t32 = abs(float(z["con_q_bits"]) - bits64), abs(float(bits32) - bits64)
    print(f"total_bits: reference {float(z['con_q_bits']):.6f}  float64 {bits64:.6f}  e_ref {e_ref:.3e}  e_t32 {e_t32:.3e}")
    assert e_ref <= FACTOR * e_t32, (e_ref, e_t32)


def test_contraction_below_at_and_above_one():
    from gauspcc_amd.cat_triplane import TriPlaneField

    z = _z()
    x = torch.as_tensor(z["con_x"])
    mag = torch.linalg.norm(x.double(), dim=-1)
    assert bool((mag < 1).any()) and bool((mag == 1).any()) and bool((mag > 1).any())
    y64 = R.contract_to_unisphere(x.double())
    ok, info = _criterion("contract_to_unisphere", z["con_unisphere"], R.contract_to_unisphere(x), y64)
    assert ok, info
    at_one = mag == 1
    assert torch.equal(torch.as_tensor(z["con_unisphere"])[at_one], x[at_one] / 4 + 0.5)    # mag = 1 takes the inner branch: x itself
    field = TriPlaneField(1.0, CONFIG, [1, 2], True, 10, device="cpu")
    unit = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    ours = field.contract_to_unisphere(x, unit)
    ok, info = _criterion("TriPlaneField.contract_to_unisphere", ours, R.contract_to_unisphere(x), y64)
    assert ok, info
    _, _, xf, _ = _golden("con")
    n64 = R.contracted_to_box(y64, xf["aabb"].double(), xf["con_aabb"].double())
    ok, info = _criterion("con_normalize_aabb", z["con_normalized"], R.contracted_to_box(R.contract_to_unisphere(x), xf["aabb"], xf["con_aabb"]), n64)
    assert ok, info
    assert bool(z["con_origin_is_nan"]) and torch.isnan(field.contract_to_unisphere(torch.zeros(1, 3), unit)).all()
    assert torch.isnan(R.contract_to_unisphere(torch.zeros(1, 3, dtype=torch.float64))).all()


@pytest.mark.parametrize("contract", [True, False], ids=["contract", "plain"])
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_fixture_conditions(case, contract):
    name, N, C, res, mult, _, _ = case
    pts, grids, xf, shapes = R.make_case(name, contract)
    assert pts.shape == (N, 3) and [tuple(p.shape) for level in grids for p in level] == [(1, C, H, W) for H, W in shapes]
    # points clamped at each of the four borders of some plane
    assert {b for _, b in R.borders_clamped(pts, shapes, xf, contract)} == {"left", "right", "top", "bottom"}
    # a point exactly on a texel centre: the first point in every case (clamped onto a corner texel on every plane), and on the
    # normalize_aabb path, whose arithmetic is exact for it, the third one without the help of the clamp
    assert R.on_texel_centre(pts[:1], shapes, xf, contract)
    if not contract and N >= 20:
        assert R.on_texel_centre(pts[2:3], shapes, xf, contract, interior=True)
    # texels whose 16 v lies exactly on .5, and ties go to even
    for level in grids:
        for p in level:
            v = p.reshape(-1)[[0, 1, -1]] * 16
            assert v.tolist() == [0.5, 1.5, -2.5] and R.quantised(p).reshape(-1)[[0, 1, -1]].tolist() == [0.0, 2.0 / 16, -2.0 / 16]
    # the near-boundary mask leaves out at most 5 % of the points
    share = float(R.near_texel_boundary(pts, shapes, xf, contract).float().mean())
    print(f"{name} {'contract' if contract else 'plain'}: {100 * share:.2f} % of the points near a texel boundary")
    assert share <= 0.05, share


def test_cluster_case_sits_inside_one_texel():
    for contract in (True, False):
        pts, _, xf, shapes = R.make_case("cluster", contract)
        g = R.normalised(pts.double(), R.xf64(xf), contract)[pts.shape[0] // 2:]
        for i, (H, W) in enumerate(shapes):
            for u in R.pixels(g, i % 3, H, W):
                assert float(torch.floor(u).max() - torch.floor(u).min()) == 0.0


def test_state_dict_matches_the_reference():
    from gauspcc_amd.cat_triplane import TriPlaneField

    z = _z()
    keys = [str(k) for k in z["keys"]]
    shapes = [tuple(int(v) for v in z[f"shapes_{i}"]) for i in range(len(keys))]
    field = TriPlaneField(1.0, CONFIG, [1, 2], True, 10, device="cpu")
    sd = field.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert all(v.device.type == "cpu" for v in sd.values())
    assert field.feat_dim == 18 and field.output_dim == 3 and field.n_ctx_rowcol == 2 and field.total_bits == 0
    assert list(field.resolutions) == [5, 7, 3] and list(field.multiscale_res_multipliers) == [1, 2]
    # the reference's initial values: planes in +-0.01, identity transform, aabb with the upper corner first
    assert all(float(p.detach().abs().max()) <= 0.01 for level in field.grids for p in level)
    assert torch.equal(field.aabb, torch.tensor([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])) and torch.equal(field.rotation_matrix, torch.eye(3))
    assert torch.equal(field.log_2_encoder_gains, torch.arange(0., 5))
    new = {k: torch.randn(s) for k, s in zip(keys, shapes)}
    field.load_state_dict(new)
    assert all(torch.equal(field.state_dict()[k], new[k]) for k in keys)


def test_set_aabb_and_rotation_follow_the_reference():
    from gauspcc_amd.cat_triplane import TriPlaneField

    field = TriPlaneField(1.0, CONFIG, [1, 2], True, 10, device="cpu")
    x = torch.tensor(_z()["con_x"])
    field.set_aabb(x, torch.tensor([3.0, 2.0, 1.0]), torch.tensor([-1.0, -2.0, -3.0]))
    y = field.contract_to_unisphere(x, torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]))
    assert torch.equal(field.con_aabb, torch.stack([y.min(0)[0], y.max(0)[0]])) and torch.equal(field.aabb, torch.tensor([[-1.0] * 3, [1.0] * 3]))
    plain = TriPlaneField(1.0, CONFIG, [1, 2], False, 10, device="cpu")
    plain.set_aabb(x, torch.tensor([3.0, 2.0, 1.0]), torch.tensor([-1.0, -2.0, -3.0]))
    assert torch.equal(plain.aabb, torch.tensor([[-1.0, -2.0, -3.0], [3.0, 2.0, 1.0]]))
    plain.set_rotation_matrix(torch.eye(3) * 2, torch.ones(3), torch.ones(3) * 3)
    assert torch.equal(plain.rotation_matrix, torch.eye(3) * 2) and not plain.rotation_matrix.requires_grad
    assert list(plain.state_dict().keys()) == list(field.state_dict().keys())


def test_argument_errors():
    from gauspcc_amd.cat_triplane import interpolate_ms_features, ms_triplane_sample

    pts = torch.zeros(4, 3)
    level = [torch.zeros(1, 3, 4, 5), torch.zeros(1, 3, 6, 5), torch.zeros(1, 3, 6, 4)]
    aabb = torch.tensor([[1.0] * 3, [-1.0] * 3])
    with pytest.raises(ValueError, match="grid_dimensions"):
        interpolate_ms_features(pts, [level], 3, True, None)
    with pytest.raises(ValueError, match="concat_features"):
        interpolate_ms_features(pts, [level], 2, False, None)
    with pytest.raises(ValueError, match="4 planes"):
        ms_triplane_sample(pts, [level + [torch.zeros(1, 3, 4, 4)]], aabb=aabb)
    with pytest.raises(ValueError, match="channels"):
        ms_triplane_sample(pts, [level, [torch.zeros(1, 2, 8, 10), torch.zeros(1, 3, 12, 10), torch.zeros(1, 3, 12, 8)]], aabb=aabb)
    with pytest.raises(ValueError, match="outside"):
        ms_triplane_sample(pts, [[torch.zeros(1, 3, 1, 5)] + level[1:]], aabb=aabb)
    with pytest.raises(ValueError, match="levels"):
        ms_triplane_sample(pts, [level] * 9, aabb=aabb)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        ms_triplane_sample(torch.zeros(4, 2), [level], aabb=aabb)
    with pytest.raises(ValueError, match="contract must hold"):
        ms_triplane_sample(pts, [level], contract=(aabb, aabb))
    with pytest.raises(ValueError, match="must hold 6 values"):
        ms_triplane_sample(pts, [level], aabb=torch.zeros(3))
    with pytest.raises(TypeError, match="float32"):
        ms_triplane_sample(pts.double(), [level], aabb=aabb)
    with pytest.raises(TypeError, match="float32"):
        ms_triplane_sample(pts, [[p.half() for p in level]], aabb=aabb)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ms_triplane_sample(pts, [[None] * 3], aabb=aabb)
    with pytest.raises(RuntimeError, match="CUDA tensor"):          # well-formed, but on the CPU: there is no CPU path
        ms_triplane_sample(pts, [level], aabb=aabb)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        interpolate_ms_features(pts, [level], 2, True, None)


def test_library_exports_the_entry_points():
    import ctypes

    from gauspcc_amd import _lib

    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gsge_msplane_forward", "gsge_msplane_backward"):
        assert name in _lib.EXPORTS and hasattr(so, name)
