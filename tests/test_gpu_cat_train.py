"""GPU tests of CAT-3DGS's training branch: the chain rate kernels (gsac_chain_rate_forward / _backward through
entropy_models.chain_rate) against the staged path (torch adds, then one `rate` per stage), the step rule with base 1.1
(gsnn_noise_forward_b through quant_noise) and gauspcc_amd.cat_renderer.generate_neural_gaussians against tests/cat_branch_ref.py and
against what the reference's own Python computed (tests/golden/cat_train.npz).

Error rule of the sum and gradient comparisons (tests/test_gpu_mlp_train.py's): per tensor, e_dev = max |device - float64| must not exceed
4 x e_t32 = max |the float32 torch program on the same GPU - float64|.  Per element chain_rate is bit-equal to the staged path (the same
float32 expressions); only its per-row sums d_Q and d_mask are added in another order."""
import os
import types

import numpy as np
import pytest
import torch

from tests import cat_train_cases as cc
from tests.cat_branch_ref import ShadowModel, cat_branch_ref, chain_rate_staged
from tests.rate_ref import rate_torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
Q0 = (1, 0.001, 0.2)
TOL = (2e-5, 2e-5, 2e-5, 2e-5, 5e-5, 2e-5)      # tests/test_gpu_ng_train.py::test_generate_training_matches_reference_branch
RATE_RTOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cat_train.npz")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


@pytest.fixture(scope="module")
def arrays():
    return cc.inputs()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _launches():
    from gauspcc_amd import _lib
    return _lib.lib().gpcc_debug_launches(0)


def _worst(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max()) if a.numel() else 0.0


# ---- kernel (a): chain_rate -------------------------------------------------------------------------------------------------------------

def _table(F, K, groups, on):
    from gauspcc_amd.cat_codec import stage_table
    view = types.SimpleNamespace(feat_dim=F, n_offsets=K, chcm_slices_list=list(groups), num_feat_slices=len(groups), chcm_for_scaling=on, chcm_for_offsets=on,
                                 mlp_chcm_list=[True] * (len(groups) - 1), mlp_chcm_scaling=True, mlp_chcm_offsets=True)
    return stage_table(view)


def _chain_case(m, groups, K, on, seed):
    """float32 CPU tensors: a context of width W inside a wider matrix, attributes near their means, and the edge rows: Q below the floor
    (which also puts x outside the clamp), a negative scale + dscale, likelihoods below 1e-6, mask zeros"""
    F = sum(groups)
    W = 2 * F + 12 + 6 * K + 3
    g = torch.Generator().manual_seed(seed)
    stages = _table(F, K, groups, on)
    wide = torch.randn(m, W + 5, generator=g)
    ctx = wide[:, 2:2 + W]
    ctx[:, :F] = torch.exp(torch.randn(m, F, generator=g) * 0.5)                                   # scales
    ctx[:, 2 * F + 6:2 * F + 12] = torch.exp(torch.randn(m, 6, generator=g) * 0.5 - 3)
    ctx[:, 2 * F + 12 + 3 * K:2 * F + 12 + 6 * K] = torch.exp(torch.randn(m, 3 * K, generator=g) * 0.5 - 1)
    ctx[:, 2 * F:2 * F + 6] = 0.08 + 0.02 * torch.randn(m, 6, generator=g)
    feat = ctx[:, F:2 * F] + torch.randn(m, F, generator=g)
    scaling = ctx[:, 2 * F:2 * F + 6] + 0.05 * torch.randn(m, 6, generator=g)
    offsets = ctx[:, 2 * F + 12:2 * F + 12 + 3 * K] + 0.3 * torch.randn(m, 3 * K, generator=g)
    feat.view(-1)[3::11] += 40.0                                                                  # L < 1e-6
    Q = torch.tensor(Q0).view(1, 3) * (1.1 + torch.tanh(torch.randn(m, 3, generator=g)))
    Q[2::5, 0] = 1e-12                                                                           # below the floor; x leaves the clamp window
    Q[1::7, 2] = 0.0
    ctx[1::3, 1] = -0.5                                                                          # a negative scale
    res = [None if st["mlp"] is None else 0.1 * torch.randn(m, 2 * st["ch"], generator=g) for st in stages]
    for st, r in zip(stages, res):
        if r is not None:
            r[::4, st["ch"]] = -5.0                                                              # scale + dscale < 0
    mask = (torch.rand(m, K, 1, generator=g) > 0.3).float()
    xm = torch.stack([feat.mean(), scaling.mean(), offsets.mean()])
    up = torch.randn(m, F + 6 + 3 * K, generator=g)
    return dict(wide=wide, W=W, feat=feat.clone(), scaling=scaling.clone(), offsets=offsets.clone().view(m, K, 3), Q=Q, res=res, mask=mask, xm=xm, up=up,
                stages=stages, F=F, K=K)


def _leaves(c, dtype):
    """the case on the device in `dtype`, every differentiable input a leaf; ctx is a strided view of the wide leaf"""
    to = lambda t: t.to(DEV, dtype).requires_grad_(True)   # noqa: E731
    d = dict(wide=to(c["wide"]), feat=to(c["feat"]), scaling=to(c["scaling"]), offsets=to(c["offsets"]), Q=to(c["Q"]), mask=to(c["mask"]),
             res=[None if r is None else to(r) for r in c["res"]])
    d["ctx"] = d["wide"][:, 2:2 + c["W"]]
    return d


def _grads(d, bits, up):
    wanted = [d["wide"], d["feat"], d["scaling"], d["offsets"], d["Q"], d["mask"]] + [r for r in d["res"] if r is not None]
    gs = torch.autograd.grad(bits, wanted, up.to(bits), allow_unused=True)
    out = dict(zip(("wide", "feat", "scaling", "offsets", "Q", "mask"), gs[:6]))
    out["res"] = list(gs[6:])
    return out


@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("K", [1, 10])
@pytest.mark.parametrize("groups", [(12, 12, 13, 13), (25, 25), (50,)])
@pytest.mark.parametrize("m", [1, 7, 257, 1000])
def test_chain_rate_matches_the_staged_path(m, groups, K, on):
    from gauspcc_amd.entropy_models import chain_rate, rate

    c = _chain_case(m, groups, K, on, seed=m + len(groups) + K + on)
    F, W, stages = c["F"], c["W"], c["stages"]
    xm = c["xm"].to(DEV)
    d = _leaves(c, torch.float32)
    assert m < 2 or not d["ctx"].is_contiguous()
    before = _launches()
    bits = chain_rate(d["ctx"], d["feat"], d["scaling"], d["offsets"], d["Q"], xm, stages, d["res"], offset_mask=d["mask"])
    assert _launches() == before + 1                                         # one launch
    s = _leaves(c, torch.float32)
    staged = chain_rate_staged(s["ctx"], s["feat"], s["scaling"], s["offsets"], s["Q"], xm, stages, s["res"], s["mask"], rate_fn=rate)
    assert bits.shape == (m, F + 6 + 3 * K) and torch.equal(bits, staged)    # bit-equal forward
    assert (bits[:, F + 6:][(c["mask"].to(DEV).repeat(1, 1, 3).view(m, -1) == 0)] == 0).all()
    got = _grads(d, bits, c["up"])
    want = _grads(s, staged, c["up"])
    for k in ("feat", "scaling", "offsets"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["wide"][:, 2:2 + W - 3], want["wide"][:, 2:2 + W - 3])
    assert torch.count_nonzero(got["wide"][:, :2]) == 0 and torch.count_nonzero(got["wide"][:, 2 + W - 3:]) == 0      # adj columns and the margin: 0
    assert len(got["res"]) == len(want["res"]) and all(torch.equal(a, b) for a, b in zip(got["res"], want["res"]))
    assert (got["feat"].abs().sum() > 0) and got["wide"][:, 2:2 + F].abs().sum() > 0
    # the per-row sums against float64
    f = _leaves(c, torch.float64)
    f64 = chain_rate_staged(f["ctx"], f["feat"], f["scaling"], f["offsets"], f["Q"], xm.double(), stages, f["res"], f["mask"], rate_fn=rate_torch)
    ref = _grads(f, f64, c["up"])
    for k in ("Q", "mask"):
        e_dev, e_t32 = _worst(got[k], ref[k]), _worst(want[k], ref[k])
        print(f"m={m} groups={groups} K={K} on={on} d_{k}: e_dev {e_dev:.3e} e_t32 {e_t32:.3e}")
        assert e_dev <= 4 * e_t32, (k, e_dev, e_t32)


def test_chain_rate_is_reproducible_on_a_side_stream():
    from gauspcc_amd.entropy_models import chain_rate

    c = _chain_case(257, (12, 12, 13, 13), 10, True, seed=3)
    xm = c["xm"].to(DEV)

    def once():
        d = _leaves(c, torch.float32)
        bits = chain_rate(d["ctx"], d["feat"], d["scaling"], d["offsets"], d["Q"], xm, c["stages"], d["res"], offset_mask=d["mask"])
        g = _grads(d, bits, c["up"])
        return [bits] + [g[k] for k in ("wide", "feat", "scaling", "offsets", "Q", "mask")] + g["res"]

    first = once()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = once()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_chain_rate_without_mask_residuals_or_rows():
    from gauspcc_amd.entropy_models import chain_rate, rate

    c = _chain_case(64, (25, 25), 10, False, seed=9)
    xm = c["xm"].to(DEV)
    d = _leaves(c, torch.float32)
    res = [None] * len(c["stages"])
    bits = chain_rate(d["ctx"], d["feat"], d["scaling"], d["offsets"].view(64, 30), d["Q"], list(xm), c["stages"], res)
    want = chain_rate_staged(d["ctx"], d["feat"], d["scaling"], d["offsets"], d["Q"], xm, c["stages"], res, None, rate_fn=rate)
    assert torch.equal(bits, want)
    before = _launches()
    e = {k: v[:0] if isinstance(v, torch.Tensor) else v for k, v in d.items()}
    empty = chain_rate(e["ctx"], e["feat"], e["scaling"], e["offsets"], e["Q"], xm, c["stages"], res, offset_mask=e["mask"])
    empty.sum().backward()
    assert empty.shape == (0, 86) and _launches() == before and d["wide"].grad.shape == d["wide"].shape


def test_chain_rate_rejects_what_it_cannot_read():
    from gauspcc_amd.entropy_models import chain_rate

    c = _chain_case(8, (25, 25), 10, True, seed=1)
    d = _leaves(c, torch.float32)
    xm, st = c["xm"].to(DEV), c["stages"]
    args = lambda **kw: {**dict(ctx=d["ctx"], feat=d["feat"], scaling=d["scaling"], offsets=d["offsets"], Q=d["Q"], x_means=xm, stages=st, residuals=d["res"]), **kw}   # noqa: E731
    with pytest.raises(TypeError, match="float32"):
        chain_rate(**args(feat=d["feat"].double()))
    with pytest.raises(RuntimeError, match="CUDA"):
        chain_rate(**args(Q=d["Q"].cpu()))
    with pytest.raises(ValueError, match="Q of shape"):
        chain_rate(**args(Q=d["Q"][:, :2]))
    with pytest.raises(ValueError, match="residuals"):
        chain_rate(**args(residuals=d["res"][:-1]))
    with pytest.raises(ValueError, match=r"residuals\[1\]"):
        chain_rate(**args(residuals=[None, d["res"][1][:, :-1]] + d["res"][2:]))
    with pytest.raises(ValueError, match="price"):
        chain_rate(**args(stages=st[:-1], residuals=d["res"][:-1]))
    with pytest.raises(ValueError, match="overlaps"):
        chain_rate(**args(stages=[st[0], dict(st[1], mean_col=st[0]["mean_col"])] + st[2:]))
    with pytest.raises(ValueError, match="x_means"):
        chain_rate(**args(x_means=xm[:2]))
    with pytest.raises(ValueError, match="offset_mask"):
        chain_rate(**args(offset_mask=d["mask"][:, :3]))


# ---- kernel (b): the step rule with base 1.1 --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [63, 257, 3000])
def test_quant_noise_with_base(n):
    from gauspcc_amd.neural_gaussians import quant_noise

    g = torch.Generator().manual_seed(n)
    widths = (50, 6, 30)
    xs = [torch.randn(n, w, generator=g) for w in widths]
    us = [torch.rand(n, w, generator=g) - 0.5 for w in widths]
    grid = torch.randn(n, 175, generator=g)
    ups = [torch.randn(n, w, generator=g) for w in widths] + [torch.randn(n, 3, generator=g)]

    def formula(dtype):
        leaf = grid.to(DEV, dtype).requires_grad_(True)
        qs = [q0 * (1.1 + torch.tanh(leaf[:, 172 + j:173 + j])) for j, q0 in enumerate(Q0)]
        outs = [x.to(DEV, dtype) + u.to(DEV, dtype) * q for x, u, q in zip(xs, us, qs)] + [torch.cat(qs, dim=1)]
        torch.autograd.backward(outs, [u.to(DEV, dtype) for u in ups])
        return outs, leaf.grad

    dgrid = grid.to(DEV).requires_grad_(True)
    out = quant_noise([x.to(DEV) for x in xs], [u.to(DEV) for u in us], Q0, dgrid[:, -3:], base=1.1)
    torch.autograd.backward(list(out), [u.to(DEV) for u in ups])
    (o64, g64), (o32, g32) = formula(torch.float64), formula(torch.float32)
    for name, dv, t32, t64 in [(f"y{j}", out[j], o32[j], o64[j]) for j in range(3)] + [("Q", out[3], o32[3], o64[3]), ("d_adj", dgrid.grad, g32, g64)]:
        e_dev, e_t32 = _worst(dv, t64), _worst(t32, t64)
        print(f"n={n} base=1.1 {name}: e_dev {e_dev:.3e} e_t32 {e_t32:.3e}")
        assert e_dev <= 4 * e_t32, (name, e_dev, e_t32)
    # the constant regime: Q0 * 1.1 formed in double
    *ys, Q = quant_noise([x.to(DEV) for x in xs], [u.to(DEV) for u in us], [q * 1.1 for q in Q0])
    for j, q0 in enumerate(Q0):
        assert torch.equal(Q[:, j], torch.full((n,), q0 * 1.1, device=DEV)) and torch.equal(ys[j], xs[j].to(DEV) + us[j].to(DEV) * torch.tensor(q0 * 1.1, device=DEV))


def test_base_one_is_the_old_entry_point():
    import ctypes as C

    from gauspcc_amd import _lib, runtime
    from gauspcc_amd.neural_gaussians import quant_noise
    from gauspcc_amd.runtime import ptrs

    n, widths = 257, (50, 6, 30)
    xs = [torch.randn(n, w, device=DEV) for w in widths]
    us = [torch.rand(n, w, device=DEV) - 0.5 for w in widths]
    grid = torch.randn(n, 175, device=DEV)
    new = quant_noise(xs, us, Q0, grid[:, -3:], base=1.0)
    default = quant_noise(xs, us, Q0, grid[:, -3:])
    ys, q = [torch.empty_like(x) for x in xs], torch.empty(n, 3, device=DEV)
    adj = grid[:, -3:]
    _lib.check(_lib.lib().gsnn_noise_forward(runtime.context(DEV), n, 3, ptrs(xs), ptrs(us), (C.c_int64 * 3)(*widths), (C.c_double * 3)(*Q0), adj.data_ptr(),
                                             adj.stride(0), (C.c_int * 3)(0, 1, 2), ptrs(ys), q.data_ptr(), runtime.stream_ptr(DEV)))
    torch.cuda.synchronize()
    for a, b, c in zip(new, default, ys + [q]):
        assert torch.equal(a, c) and torch.equal(b, c)


# ---- the branch -------------------------------------------------------------------------------------------------------------------------

def _device_model(arrays, name, decoded=False, dtype=torch.float32):
    from gauspcc_amd import entropy_models

    pc, cam, vis, wmask = cc.model(arrays, name, torch, DEV, dtype, decoded=decoded)
    pc.entropy_gaussian = entropy_models.Entropy_gaussian(Q=1, q_floor=1e-9)
    return pc, cam, vis, wmask


def _replayed(arrays, tag, fn, monkeypatch):
    from gauspcc_amd import cat_renderer

    replay = cc.Replay(arrays, tag, torch)
    monkeypatch.setattr(cat_renderer, "_uniform_like", replay.uniform_like)
    monkeypatch.setattr(cat_renderer, "_rand_like", replay.rand_like)
    res = fn()
    assert not replay.queue
    return res


def _check(got, want, train, rates):
    n = 6 if train else 5
    if train:
        assert torch.equal(got[6], want[6]) and got[6].dtype == torch.bool
    for i in range(n):
        assert got[i].shape == want[i].shape and got[i].dtype == want[i].dtype, i
        err = _worst(got[i], want[i])
        print(f"output {i}: {err:.3e}")
        assert torch.allclose(got[i], want[i], atol=TOL[i], rtol=TOL[i]), (i, err)
    assert not rates or all(isinstance(got[i], torch.Tensor) for i in range(7, 11))
    for i in range(7, 12) if train else [6]:
        if isinstance(want[i], torch.Tensor):
            assert rates or i in (6, 11)
            print(f"scalar {i}: {float(got[i].detach()):.7f} against {float(want[i].detach()):.7f}")
            assert torch.allclose(got[i], want[i], rtol=RATE_RTOL), i
        else:       # None below the rate branch; feat_rate the integer 0 where no context ran
            assert (got[i] is None and want[i] is None) or (not isinstance(got[i], torch.Tensor) and got[i] == want[i] == 0), i


@pytest.mark.parametrize("tag", [r[0] for r in cc.RUNS])
def test_branch_matches_the_reference_fixture(tag, arrays, golden, monkeypatch):
    """on the device, the recorded draws replayed: what the reference's own Python computed, within the fixture's stored tolerances, and
    the float32 restatement on the same GPU"""
    from gauspcc_amd import cat_renderer

    assert str(golden["inputs_sha256"]) == cc.sha256_of(arrays)
    _, name, train, step, wm, decoded = cc.run(tag)
    pc, cam, vis, wmask = _device_model(arrays, name, decoded)
    mask = wmask if wm else None
    with torch.no_grad():
        res = _replayed(arrays, tag, lambda: cat_renderer.generate_neural_gaussians(cam, pc, vis, is_training=train, step=step, mask=mask), monkeypatch)
    assert pc.bound_updates == (1 if train and step == 10000 else 0)
    ran = not decoded and (cc.rate_branch(step) if train else (step >= 10000 or step == -1))
    assert pc.feature_net.calls == ([step] if ran else [])
    cc.compare(res, golden, tag)
    pc2, _, _, _ = _device_model(arrays, name, decoded)
    with torch.no_grad():
        want = _replayed(arrays, tag, lambda: cat_branch_ref(cam, pc2, vis, step, is_training=train, mask=mask), monkeypatch)
    _check(res, want, train, train and cc.rate_branch(step))
    if not train:
        assert isinstance(res[5], float if ran else int) and res[5] >= 0          # time_sub


def _logit_masks(pc):
    """the model's {0, 1} masks as trainable logits behind CAT-3DGS's straight-through get_mask"""
    pc._mask = ((pc._mask01 * 2 - 1) * 6).clone().requires_grad_(True)

    def get_mask(weighted_mask=None):
        s = torch.sigmoid(pc._mask)
        if weighted_mask is not None:
            s = s * weighted_mask
        return ((s > 0.01).to(s.dtype) - s).detach() + s

    def get_mask_anchor(weighted_mask=None):
        with torch.no_grad():
            return torch.sum(get_mask(weighted_mask), dim=1)[:, 0] > 0
    pc.get_mask, pc.get_mask_anchor = get_mask, get_mask_anchor


def _loss(res, R):
    return sum((o * r.to(o)).sum() for o, r in zip(res[:6], R)) + res[7] + res[11]


def test_gradients_match_float64(arrays, monkeypatch):
    """loss = sum(outputs * fixed weights) + bit_per_param + feat_rate at step 12000 with the recorded draws: the drop-in's gradients of the
    anchors, feat, offsets, scalings, _mask, every view MLP, every chcm MLP and the stand-in feature_net against the float64 restatement,
    within 4 x the float32 restatement's own error"""
    from gauspcc_amd import cat_renderer

    tag, step = "train12000", 12000
    pc, cam, vis, _ = _device_model(arrays, "main")
    _logit_masks(pc)
    leaves = {"get_anchor": pc.get_anchor, "_anchor_feat": pc._anchor_feat, "_offset": pc._offset, "_scaling": pc.get_scaling, "_mask": pc._mask}
    for p in leaves.values():
        p.requires_grad_(True)
    mods = [("feature_net", pc.feature_net), ("chcm_list", pc.get_chcm_mlp_list), ("chcm_scaling", pc.get_chcm_mlp_scaling), ("chcm_offsets", pc.get_chcm_mlp_offsets),
            ("opacity", pc.get_opacity_mlp), ("cov", pc.get_cov_mlp), ("color", pc.get_color_mlp)]
    for name, m in mods:
        for k, p in m.named_parameters():
            leaves[f"{name}.{k}"] = p

    def device_run():
        for p in leaves.values():
            p.grad = None
        res = _replayed(arrays, tag, lambda: cat_renderer.generate_neural_gaussians(cam, pc, vis, is_training=True, step=step), monkeypatch)
        return res

    res = device_run()
    gen = torch.Generator(device=DEV).manual_seed(11)
    R = [torch.randn(o.shape, device=DEV, generator=gen) for o in res[:6]]
    _loss(res, R).backward()
    got = {k: p.grad.detach().clone() for k, p in leaves.items()}
    res2 = device_run()
    _loss(res2, R).backward()
    assert all(torch.equal(a, b) for a, b in zip(res[:11], res2[:11]))                 # two runs are bit-identical
    assert all(torch.equal(got[k], p.grad) for k, p in leaves.items())
    for k, v in got.items():
        assert torch.count_nonzero(v) > 0, f"no gradient reaches {k}"
    ref = {}
    for dtype in (torch.float64, torch.float32):
        sh = ShadowModel(pc, dtype)
        sh.get_anchor.requires_grad_(True)
        out = _replayed(arrays, tag, lambda: cat_branch_ref(cam, sh, vis, step), monkeypatch)
        assert torch.equal(out[6], res[6])
        _loss(out, R).backward()
        ref[dtype] = dict(sh.trainable(), get_anchor=sh.get_anchor)
        ref[dtype] = {k: p.grad for k, p in ref[dtype].items()}
    assert set(ref[torch.float64]) == set(got), set(ref[torch.float64]) ^ set(got)
    bad = []
    for k, want in ref[torch.float64].items():
        e_dev, e_t32 = _worst(got[k], want), _worst(ref[torch.float32][k], want)
        print(f"{k}: e_dev {e_dev:.3e} e_t32 {e_t32:.3e} (largest |gradient| {float(want.abs().max()):.3e})")
        if not e_dev <= 4 * e_t32:
            bad.append((k, e_dev, e_t32))
    assert not bad, bad


def _synth(n, seed=3, **kw):
    from gauspcc_amd import entropy_models
    from gauspcc_amd.synth import SyntheticGaussianModelCAT

    pc = SyntheticGaussianModelCAT(n, seed=seed, device="cuda:0", chcm_for_scaling=True, chcm_for_offsets=True, **kw)
    with torch.no_grad():   # opacity outputs well away from 0: the keep sets of the programs compared must agree
        pc.mlp_opacity[2].weight.mul_(0.05)
        pc.mlp_opacity[2].bias.copy_(torch.tensor([2.0, -2.0] * (pc.n_offsets // 2) + [2.0] * (pc.n_offsets % 2), device=DEV))
    pc.entropy_gaussian = entropy_models.Entropy_gaussian(Q=1, q_floor=1e-9)
    return pc


def _cam(pc):
    return types.SimpleNamespace(camera_center=pc.get_anchor.mean(dim=0) + torch.tensor([0.0, 0.0, -2.0], device=DEV))


def _vis(n, frac=0.8):
    return torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) < frac


@pytest.mark.parametrize("visible", ["most", "all"])
@pytest.mark.parametrize("step", [5000, 12000, -1])
def test_seeded_run_draws_as_the_restatement(step, visible):
    """no hooks replaced: under one torch.manual_seed the drop-in and the float32 restatement (sharing the model's TriPlaneField head, which
    draws first) choose the same anchors and add the same noise"""
    from gauspcc_amd.cat_renderer import generate_neural_gaussians

    pc = _synth(3000)
    n = pc.get_anchor.shape[0]
    cam, vis = _cam(pc), (_vis(n) if visible == "most" else None)
    torch.manual_seed(step + 20)
    with torch.no_grad():
        got = generate_neural_gaussians(cam, pc, vis, is_training=True, step=step)
    after = torch.rand(1, device=DEV)
    shadow = ShadowModel(pc, torch.float32, feature_net=pc.feature_net)
    torch.manual_seed(step + 20)
    with torch.no_grad():
        want = cat_branch_ref(cam, shadow, vis, step)
    assert torch.equal(after, torch.rand(1, device=DEV))         # both programs drew as many numbers
    _check(got, want, True, cc.rate_branch(step))


def test_feat_dim_32_with_the_feature_bank():
    from gauspcc_amd.cat_renderer import generate_neural_gaussians

    pc = _synth(1000, feat_dim=32, n_offsets=5, chcm_slices_list=(16, 16), use_feat_bank=True)
    n = pc.get_anchor.shape[0]
    cam, vis = _cam(pc), _vis(n)
    for train in (True, False):
        torch.manual_seed(4)
        got = generate_neural_gaussians(cam, pc, vis, is_training=train, step=12000)
        torch.manual_seed(4)
        with torch.no_grad():
            want = cat_branch_ref(cam, ShadowModel(pc, torch.float32, feature_net=pc.feature_net), vis, 12000, is_training=train)
        if train:
            _check(got, want, True, True)
            got[7].backward()
            assert torch.count_nonzero(pc.mlp_chcm_list[0][0].weight.grad) > 0
        else:
            assert len(got) == 7 and got[0].shape[0] > 0 and all(torch.isfinite(g).all() for g in got[:5])


def test_edges(arrays, monkeypatch):
    from gauspcc_amd import cat_renderer

    pc, cam, vis, wmask = _device_model(arrays, "main")
    n = pc.get_anchor.shape[0]
    none = torch.zeros(n, dtype=torch.bool, device=DEV)
    shapes = [(0, 3), (0, 3), (0, 1), (0, 3), (0, 4), (0, 1), (0,)]
    for step in (5000, 12000):      # nothing visible: the reference's tensor program on empty tensors (0 / 0 in the rates)
        out = cat_renderer.generate_neural_gaussians(cam, pc, none, is_training=True, step=step)
        assert len(out) == 12 and [tuple(o.shape) for o in out[:7]] == shapes
        assert all(o is None for o in out[7:11]) if step == 5000 else all(torch.isnan(o) for o in out[7:11])
    # un-decoded, nothing visible, evaluation: from step 10000 on feature_net runs on the (0, 3) anchor, is timed, and its rate comes back
    feature_net, calls = pc.feature_net, []

    def recording(anchor, itr=-1):
        calls.append((tuple(anchor.shape), feature_net(anchor, itr=itr)))
        return calls[-1][1]
    pc.feature_net = recording
    out = cat_renderer.generate_neural_gaussians(cam, pc, none, is_training=False, step=12000)
    assert len(out) == 7 and [tuple(o.shape) for o in out[:5]] == shapes[:5]
    assert len(calls) == 1 and calls[0][0] == (0, 3) and out[6] is calls[0][1][1] and type(out[5]) is float
    out = cat_renderer.generate_neural_gaussians(cam, pc, none, is_training=False, step=5000)
    assert len(out) == 7 and [tuple(o.shape) for o in out[:5]] == shapes[:5]
    assert len(calls) == 1 and type(out[5]) is int and out[5] == 0 and type(out[6]) is int and out[6] == 0
    pc.feature_net = feature_net
    # nothing chosen: the chain launches nothing, the MLPs are not run, the rates are 0 / 0
    monkeypatch.setattr(cat_renderer, "_rand_like", lambda t: torch.ones_like(t))
    torch.manual_seed(0)
    out = cat_renderer.generate_neural_gaussians(cam, pc, vis, is_training=True, step=12000)
    assert out[0].shape[0] > 0 and all(torch.isnan(o) for o in out[7:11]) and torch.isfinite(out[11])
    sum(o.sum() for o in out[:5]).backward()
    monkeypatch.undo()
    # visible_mask=None is every anchor; mask= reaches get_mask and get_mask_anchor
    torch.manual_seed(1)
    with torch.no_grad():
        a = cat_renderer.generate_neural_gaussians(cam, pc, None, is_training=True, step=12000, mask=wmask)
    torch.manual_seed(1)
    with torch.no_grad():
        b = cat_renderer.generate_neural_gaussians(cam, pc, torch.ones(n, dtype=torch.bool, device=DEV), is_training=True, step=12000, mask=wmask)
        c = cat_renderer.generate_neural_gaussians(cam, pc, None, is_training=True, step=2000)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[6].sum() < c[6].sum()
    # a context of another width is refused
    pc.feature_net = lambda anchor, itr=-1: (anchor.new_zeros(anchor.shape[0], 170), 0)
    with pytest.raises(ValueError, match="feature_net"):
        cat_renderer.generate_neural_gaussians(cam, pc, vis, is_training=True, step=12000)
    torch.cuda.synchronize()


def test_it_trains():
    """twenty Adam steps on the features, the context head and the channel-context MLPs lower bit_per_param (looked at under one fixed seed)"""
    from gauspcc_amd.cat_renderer import generate_neural_gaussians

    pc = _synth(3000, seed=9)
    n = pc.get_anchor.shape[0]
    cam, vis = _cam(pc), _vis(n)
    mods = [pc.mlp_chcm_list, pc.mlp_chcm_scaling, pc.mlp_chcm_offsets]
    params = [pc._anchor_feat] + [p for m in mods for p in m.parameters()] + list(pc.feature_net.get_mlp_parameters())
    for p in params:
        p.requires_grad_(True)

    def bits(seed):
        torch.manual_seed(seed)
        return generate_neural_gaussians(cam, pc, vis, is_training=True, step=12000)[7]

    with torch.no_grad():
        before = float(bits(1000))
    opt = torch.optim.Adam(params, lr=2e-4)      # steps of at most 4e-3 per weight in all: the scaling heads' scales are of order 0.05
    for it in range(20):
        opt.zero_grad()
        bits(it).backward()
        opt.step()
    with torch.no_grad():
        after = float(bits(1000))
    print(f"bit_per_param {before:.4f} -> {after:.4f}")
    assert np.isfinite(after) and after < before, (before, after)
