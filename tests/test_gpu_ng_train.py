"""GPU tests of the neural-Gaussian training path (gsnn_forward_train / gsnn_backward through neural_gaussians_train and
generate_neural_gaussians(is_training=True)) against the float64 restatement tests/ng_train_ref.py."""
import math
import types

import pytest
import torch

from tests.ng_train_ref import fixture, ng_train_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def _fixture(n, F, K, bank, mask_after, seed):
    return fixture(n, F, K, bank, mask_after, seed, DEV)


def _pc(ps, bank):
    """a model object whose MLPs hold float32 copies of the parameters"""
    def seq(w1, b1, w2, b2):
        l1, l2 = torch.nn.Linear(w1.shape[1], w1.shape[0]), torch.nn.Linear(w2.shape[1], w2.shape[0])
        with torch.no_grad():
            l1.weight.copy_(w1); l1.bias.copy_(b1); l2.weight.copy_(w2); l2.bias.copy_(b2)
        return torch.nn.Sequential(l1, torch.nn.ReLU(True), l2).to(DEV)
    pc = types.SimpleNamespace(use_feat_bank=bank)
    pc.get_featurebank_mlp = seq(*ps[0:4]) if bank else None
    pc.get_opacity_mlp, pc.get_cov_mlp, pc.get_color_mlp = seq(*ps[4:8]), seq(*ps[8:12]), seq(*ps[12:16])
    return pc


def _pc_params(pc, bank):
    out = []
    for s in ([pc.get_featurebank_mlp] if bank else []) + [pc.get_opacity_mlp, pc.get_cov_mlp, pc.get_color_mlp]:
        out += [s[0].weight, s[0].bias, s[2].weight, s[2].bias]
    return out


def _run(ts, pc, mask_after, R=None, stream_fn=None):
    from gauspcc_amd.neural_gaussians import neural_gaussians_train

    ins = [t.float().detach().clone().requires_grad_(True) for t in ts[:5]]
    out = neural_gaussians_train(*ins, ts[5].float(), pc, mask_after_opacity=mask_after)
    if R is None:
        return out, None
    if stream_fn is not None:
        stream_fn()
    loss = sum((o * r).sum() for o, r in zip(out[:6], R))
    for p in _pc_params(pc, pc.use_feat_bank):
        p.grad = None
    loss.backward()
    return out, [t.grad for t in ins] + [p.grad.clone() for p in _pc_params(pc, pc.use_feat_bank)]


FWD = [(32, 5, False, False, 15), (32, 10, True, False, 3001), (32, 10, True, True, 3001), (50, 10, False, False, 20011), (50, 10, False, True, 20011),
       (32, 17, False, False, 2000), (50, 17, False, True, 2000), (32, 17, True, True, 999), (50, 5, False, True, 200003), (32, 10, True, False, 200003)]


@pytest.mark.parametrize("F,K,bank,mask_after,n", FWD)
def test_forward_matches_restatement(F, K, bank, mask_after, n):
    ts, ps = _fixture(n, F, K, bank, mask_after, seed=F * 7 + K + n % 97)
    ref = ng_train_ref(*ts, ps, mask_after)
    out, _ = _run(ts, _pc(ps, bank), mask_after)
    assert torch.equal(out[6], ref[6])
    for name, a, b, tol in zip(("xyz", "color", "opacity", "scaling", "rot", "neural_opacity"), out[:6], ref[:6], (2e-5,) * 4 + (5e-5, 2e-5)):
        assert a.shape == b.shape and a.dtype == torch.float32, name
        assert torch.allclose(a.double(), b, atol=tol, rtol=tol), (name, (a.double() - b).abs().max().item())
    assert out[6].dtype == torch.bool and out[5].shape == (ts[0].shape[0] * K, 1)


@pytest.mark.parametrize("F,K,bank,n", [(32, 5, False, 15),        # less than one 16-anchor tile
                                        (32, 10, True, 3001),       # ragged last tile, matrix-pipe path, feature bank
                                        (50, 17, False, 2000)])     # K > 16: the lane kernels and k_assemble
def test_training_forward_equals_inference_forward(F, K, bank, n):
    """HAC's order: the training kernels multiply by a mask of exactly 1.0f and otherwise evaluate the inference kernels' expressions, so the
    five tensors of neural_gaussians_train equal generate_neural_gaussians' for a decoded model holding the same tensors, bit for bit."""
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians, neural_gaussians_train

    ts, ps = _fixture(n, F, K, bank, False, seed=F + K + n % 83)
    n = ts[0].shape[0]
    if n > 16 and n % 16 == 0:          # the fixture leaves anchors out: keep the last tile ragged
        n -= 1
    anchor, feat, off, sc, masks = (t[:n].float() for t in ts[:5])
    assert (n < 16) if K == 5 else (n > 16 and n % 16)
    pc = _pc(ps, bank)
    pc.decoded_version, pc.feat_dim, pc.n_offsets = True, F, K
    pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc.get_mask = anchor, feat, off, sc, masks
    cam = types.SimpleNamespace(camera_center=ts[5].float())
    want = generate_neural_gaussians(cam, pc, None)[:5]
    got = neural_gaussians_train(anchor, feat, off, sc, masks, cam.camera_center, pc)
    assert 0 < want[0].shape[0] < n * K and int(got[6].sum()) == want[0].shape[0]
    for name, a, b in zip(("xyz", "color", "opacity", "scaling", "rot"), got[:5], want):
        assert a.shape == b.shape and torch.equal(a, b), name


def _upstream(out, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(o.shape, device=DEV, generator=g) for o in out[:6]]


GRAD = [(32, 5, False, False, 301), (32, 10, True, False, 4001), (32, 10, True, True, 4001), (50, 10, False, False, 5003), (50, 10, False, True, 5003),
        (50, 17, False, False, 1500), (32, 17, True, True, 1500), (50, 10, False, False, 200003)]


@pytest.mark.parametrize("F,K,bank,mask_after,n", GRAD)
def test_gradients_match_float64(F, K, bank, mask_after, n):
    ts, ps = _fixture(n, F, K, bank, mask_after, seed=F + 3 * K + n % 89)
    pc = _pc(ps, bank)
    out, _ = _run(ts, pc, mask_after)
    R = _upstream(out, 11)
    _, got = _run(ts, pc, mask_after, R)
    ins = [t.clone().requires_grad_(True) for t in ts[:5]]
    pr = [None if p is None else p.clone().requires_grad_(True) for p in ps]
    ref = ng_train_ref(*ins, ts[5], pr, mask_after)
    sum((o * r.double()).sum() for o, r in zip(ref[:6], R)).backward()
    want = [t.grad for t in ins] + [p.grad for p in pr if p is not None]
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, i
        rel = (a.double() - b).norm() / max(b.norm().item(), 1e-30)
        assert rel < 5e-5, (i, rel.item())


def test_gradients_bitwise_reproducible():
    from gauspcc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

    ts, ps = _fixture(250007, 50, 10, False, False, seed=5)
    pc = _pc(ps, False)
    out, _ = _run(ts, pc, False)
    R = _upstream(out, 3)
    _, g0 = _run(ts, pc, False, R)
    _, g1 = _run(ts, pc, False, R)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _, g2 = _run(ts, pc, False, R)
    torch.cuda.synchronize()

    def other_call():   # a rasteriser forward between forward and backward
        W = H = 64
        view = torch.eye(4, device=DEV); view[3, 2] = 6.0
        P = torch.zeros(4, 4, device=DEV); P[0, 0] = P[1, 1] = 1.0; P[3, 2] = 1.0; P[2, 2] = 1.0; P[2, 3] = -0.01
        st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3, device=DEV), scale_modifier=1.0,
                                           viewmatrix=view, projmatrix=(view @ P.T).contiguous(), sh_degree=0, campos=torch.zeros(3, device=DEV),
                                           prefiltered=False, debug=False)
        with torch.no_grad():
            m = out[0][:1000].detach()
            GaussianRasterizer(st)(means3D=m, means2D=None, shs=None, colors_precomp=out[1][:1000].detach(), opacities=out[2][:1000].detach(),
                                   scales=out[3][:1000].detach(), rotations=out[4][:1000].detach(), cov3D_precomp=None)
    _, g3 = _run(ts, pc, False, R, stream_fn=other_call)
    for a, b, c, d in zip(g0, g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_edge_cases():
    from gauspcc_amd._lib import GpccError
    from gauspcc_amd.neural_gaussians import neural_gaussians_train

    ts, ps = _fixture(100, 32, 5, False, False, seed=1)
    pc = _pc(ps, False)
    # n == 0
    empty = [t[:0].float().requires_grad_(True) for t in ts[:5]]
    out = neural_gaussians_train(*empty, ts[5].float(), pc)
    assert out[0].shape == (0, 3) and out[5].shape == (0, 1) and out[6].shape == (0,)
    (out[5].sum() + out[0].sum()).backward()
    assert all(torch.count_nonzero(p.grad) == 0 for p in _pc_params(pc, False))
    # every anchor fully masked (HAC): nothing kept, the neural_opacity gradient still reaches the masks and the opacity MLP
    ins = [t.float().clone().requires_grad_(True) for t in ts[:5]]
    with torch.no_grad():
        ins[4].zero_()
    for p in _pc_params(pc, False):
        p.grad = None
    out = neural_gaussians_train(*ins, ts[5].float(), pc)
    assert out[0].shape[0] == 0 and not out[6].any()
    (out[5] * torch.randn_like(out[5])).sum().backward()
    assert torch.count_nonzero(ins[4].grad) > 0 and torch.count_nonzero(ins[0].grad) == 0
    assert torch.count_nonzero(pc.get_color_mlp[0].weight.grad) == 0
    with pytest.raises(GpccError):
        bad = [torch.zeros(4, 3, device=DEV), torch.zeros(4, 40, device=DEV), torch.zeros(4, 5, 3, device=DEV), torch.ones(4, 6, device=DEV),
               torch.ones(4, 5, 1, device=DEV)]
        neural_gaussians_train(*bad, ts[5].float(), pc)


# ---- the reference's call shape -----------------------------------------------------------------------------------------------------

class _Entropy(torch.nn.Module):
    """test-side stand-in for HAC's entropy_gaussian: bits of x under N(mean, scale) over a bin of width Q"""
    def forward(self, x, mean, scale, Q, x_mean=None):
        scale = torch.clamp(scale, min=1e-9)
        d = torch.distributions.normal.Normal(mean, scale)
        p = d.cdf(x + 0.5 * Q) - d.cdf(x - 0.5 * Q)
        return -torch.log2(torch.clamp(p, min=1e-6))


def _synth(n, seed=3):
    from gauspcc_amd.synth import SyntheticGaussianModel

    pc = SyntheticGaussianModel(n, seed=seed, device="cuda:0")
    with torch.no_grad():   # opacity outputs well away from 0: the keep sets of the two programs must agree
        pc.mlp_opacity[2].weight.mul_(0.05)
        pc.mlp_opacity[2].bias.copy_(torch.tensor([2.0, -2.0] * (pc.n_offsets // 2) + [2.0] * (pc.n_offsets % 2), device=DEV))
    pc.entropy_gaussian = _Entropy()
    pc.bound_updates = 0

    def update_anchor_bound():
        pc.bound_updates += 1
    pc.update_anchor_bound = update_anchor_bound
    return pc


def _ref_branch(cam, pc, visible_mask, step):
    """torch restatement of HAC's training branch (noise, rate terms, then the core in float32)"""
    F, K = pc.feat_dim, pc.n_offsets
    anchor = pc.get_anchor[visible_mask]
    feat = pc._anchor_feat[visible_mask]
    offs = pc._offset[visible_mask]
    scl = pc.get_scaling[visible_mask]
    masks = pc.get_mask[visible_mask]
    ma = pc.get_mask_anchor[visible_mask]
    rate = (ma.sum() / ma.numel()).detach()
    bits = [None] * 4
    if 3000 < step <= 10000:
        feat = feat + torch.empty_like(feat).uniform_(-0.5, 0.5) * 1
        scl = scl + torch.empty_like(scl).uniform_(-0.5, 0.5) * 0.001
        offs = offs + torch.empty_like(offs).uniform_(-0.5, 0.5) * 0.2
    if step > 10000:
        c = pc.get_grid_mlp(pc.calc_interp_feat(anchor))
        mean, scale, ms, ss, mo, so, qf, qs, qo = torch.split(c, [F, F, 6, 6, 3 * K, 3 * K, 1, 1, 1], dim=-1)
        qf, qs, qo = 1 * (1 + torch.tanh(qf)), 0.001 * (1 + torch.tanh(qs)), 0.2 * (1 + torch.tanh(qo))
        feat = feat + torch.empty_like(feat).uniform_(-0.5, 0.5) * qf
        scl = scl + torch.empty_like(scl).uniform_(-0.5, 0.5) * qs
        offs = offs + torch.empty_like(offs).uniform_(-0.5, 0.5) * qo.unsqueeze(1)
        ch = (torch.rand_like(anchor[:, 0]) <= 0.05) & ma.to(torch.bool)
        bf = pc.entropy_gaussian(feat[ch], mean[ch], scale[ch], qf[ch])
        bs = pc.entropy_gaussian(scl[ch], ms[ch], ss[ch], qs[ch])
        bo = pc.entropy_gaussian(offs[ch].view(-1, 3 * K), mo[ch], so[ch], qo[ch]) * masks[ch].repeat(1, 1, 3).view(-1, 3 * K)
        bits = [(bf.sum() + bs.sum() + bo.sum()) / (bf.numel() + bs.numel() + bo.numel()) * rate,
                bf.sum() / bf.numel() * rate, bs.sum() / bs.numel() * rate, bo.sum() / bo.numel() * rate]
    params = [None] * 4 + _pc_params(pc, False)
    t = torch.tanh(pc.mlp_opacity(torch.cat([feat, *(lambda v: (v / v.norm(dim=1, keepdim=True), v.norm(dim=1, keepdim=True)))(anchor - cam.camera_center)], 1)))
    out = ng_train_ref(anchor, feat, offs, scl, masks, cam.camera_center, params, False)
    return list(out) + bits, t, masks


@pytest.mark.parametrize("step", [2000, 5000, 10000, 12000])
def test_generate_training_matches_reference_branch(step):
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians

    pc = _synth(3000)
    cam = types.SimpleNamespace(camera_center=pc.get_anchor.mean(dim=0) + torch.tensor([0.0, 0.0, -2.0], device=DEV))
    vis = torch.rand(3000, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) < 0.8
    torch.manual_seed(step)
    got = generate_neural_gaussians(cam, pc, vis, is_training=True, step=step)
    assert pc.bound_updates == (1 if step == 10000 else 0)
    torch.manual_seed(step)
    with torch.no_grad():
        want, t, masks = _ref_branch(cam, pc, vis, step)
    assert len(got) == 11
    live = masks.view(-1) != 0
    assert not ((t.reshape(-1).abs() < 1e-4) & live).any()
    assert torch.equal(got[6], want[6]) and got[6].dtype == torch.bool
    for i, tol in zip(range(6), (2e-5, 2e-5, 2e-5, 2e-5, 5e-5, 2e-5)):
        assert got[i].shape == want[i].shape and got[i].dtype == want[i].dtype, i
        assert torch.allclose(got[i], want[i], atol=tol, rtol=tol), (i, (got[i] - want[i]).abs().max().item())
    for i in range(7, 11):
        if step > 10000:
            assert torch.allclose(got[i], want[i], rtol=1e-5), i
        else:
            assert got[i] is None and want[i] is None
    (got[0].sum() + got[3].sum() + got[5].sum()).backward()
    assert pc.mlp_cov[0].weight.grad is not None and pc.mlp_opacity[2].bias.grad is not None


def test_hac_plus_model_names_the_core():
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians
    from gauspcc_amd.synth import SyntheticGaussianModelPlus

    pc = SyntheticGaussianModelPlus(200, seed=1, device="cuda:0")
    cam = types.SimpleNamespace(camera_center=torch.zeros(3, device=DEV))
    with pytest.raises(NotImplementedError, match="neural_gaussians_train"):
        generate_neural_gaussians(cam, pc, None, is_training=True, step=0)


def test_it_trains():
    """~200 Adam steps of the MLPs and features through the library's rasteriser in training mode towards an image rendered from perturbed
    MLP weights and features"""
    from gauspcc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians

    pc = _synth(4000, seed=9)
    W = H = 96
    with torch.no_grad():
        a = pc.get_anchor
        ctr = a.mean(dim=0)
        ext = float((a.max(dim=0).values - a.min(dim=0).values).max())
    eye = ctr + torch.tensor([0.0, 0.0, -1.6 * ext], device=DEV)
    Rt = torch.eye(4, device=DEV); Rt[:3, 3] = -eye
    fov = math.radians(60)
    zn, zf = 0.01, 100.0
    P = torch.zeros(4, 4, device=DEV)
    P[0, 0] = P[1, 1] = 1 / math.tan(fov / 2); P[3, 2] = 1.0; P[2, 2] = zf / (zf - zn); P[2, 3] = -(zf * zn) / (zf - zn)
    view = Rt.T.contiguous()
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(fov / 2), tanfovy=math.tan(fov / 2), bg=torch.zeros(3, device=DEV),
                                       scale_modifier=1.0, viewmatrix=view, projmatrix=(view @ P.T).contiguous(), sh_degree=0, campos=eye, prefiltered=False,
                                       debug=False)
    rast = GaussianRasterizer(st)
    cam = types.SimpleNamespace(camera_center=eye)
    with torch.no_grad():
        pc._scaling.add_(3.0)       # footprints of a few pixels at this distance

    def render():
        xyz, color, opacity, scaling, rot = generate_neural_gaussians(cam, pc, None, is_training=True, step=0)[:5]
        return rast(means3D=xyz, means2D=torch.zeros_like(xyz), shs=None, colors_precomp=color, opacities=opacity, scales=scaling, rotations=rot,
                    cov3D_precomp=None)[0]

    params = [pc._anchor_feat] + [p for m in (pc.mlp_opacity, pc.mlp_cov, pc.mlp_color) for p in m.parameters()]
    saved = [p.detach().clone() for p in params]
    g = torch.Generator(device=DEV).manual_seed(4)
    with torch.no_grad():
        for p in params:
            p.add_(torch.randn(p.shape, device=DEV, generator=g) * 0.1 * (p.abs().mean() + 1e-3))
        target = render().detach()
        for p, s in zip(params, saved):
            p.copy_(s)
    for p in params:
        p.requires_grad_(True)
    opt = torch.optim.Adam(params, lr=2e-3)
    losses = []
    for it in range(200):
        opt.zero_grad()
        loss = ((render() - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[0] > 0 and min(losses[-10:]) < 0.5 * losses[0], (losses[0], losses[-10:])
