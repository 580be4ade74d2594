"""GPU tests of HAC++'s training branch: the quantisation-noise kernels (gsnn_noise_forward / gsnn_noise_backward through quant_noise),
the row expansion (gpcc_expand_rows through select_rows) and gauspcc_amd.hac_plus_renderer.generate_neural_gaussians(is_training=True)
against tests/hacpp_branch_ref.py and against what the reference's own Python computed (tests/golden/hacpp_train.npz).

Error rule of the kernel and gradient comparisons (tests/test_gpu_mlp_train.py's): per tensor, e_dev = max |device - float64| must not exceed
4 x e_t32 = max |the float32 torch formula on the same GPU - float64|.  A yardstick taken over a handful of values is a lottery (the
float32 formula may land on the float64 value by luck), so the n = 1 backward cases draw g, u and gQ as multiples of 1/8 and 1/16: every
product and sum is then exact in float32 in any order, and what is compared is the tanh chain, which the kernel evaluates in autograd's order."""
import os
import types

import numpy as np
import pytest
import torch

from tests import hacpp_train_cases as hc
from tests.hacpp_branch_ref import ShadowModel, hacpp_branch_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
Q0 = (1, 0.001, 0.2)
STEPS = (2000, 5000, 10000, 12000)
TOL = (2e-5, 2e-5, 2e-5, 2e-5, 5e-5, 2e-5)      # tests/test_gpu_ng_train.py::test_generate_training_matches_reference_branch
RATE_RTOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def _launches():
    from gauspcc_amd import _lib
    return _lib.lib().gpcc_debug_launches(0)


# ---- kernel (a): quant_noise ------------------------------------------------------------------------------------------------------------

def _noise_case(n, widths, adj_cols, seed, dyadic=False):
    """xs, us, gs (upstream of the ys), gq and adj: a view of the last three columns of an (n, adj_cols) matrix, or None"""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, w, generator=g) for w in widths]
    if dyadic:
        us = [torch.randint(-8, 8, (n, w), generator=g).float() / 16 for w in widths]
        gs = [torch.randint(-8, 9, (n, w), generator=g).float() / 8 for w in widths]
        gq = torch.randint(-8, 9, (n, len(widths)), generator=g).float() / 8
    else:
        us = [torch.rand(n, w, generator=g) - 0.5 for w in widths]
        gs = [torch.randn(n, w, generator=g) for w in widths]
        gq = torch.randn(n, len(widths), generator=g)
    grid = None if adj_cols is None else torch.randn(n, adj_cols, generator=g)
    return xs, us, gs, gq, grid


def _formula(xs, us, grid, dtype, nattr):
    """the torch formula in `dtype` on the device: (ys, Q (n, nattr), the adj leaf or None)"""
    xs = [x.to(DEV, dtype).requires_grad_(True) for x in xs]
    us = [u.to(DEV, dtype) for u in us]
    n = xs[0].shape[0]
    if grid is None:
        qs = [torch.full((n, 1), q0, dtype=dtype, device=DEV) for q0 in Q0[:nattr]]
        leaf = None
    else:
        leaf = grid.to(DEV, dtype).requires_grad_(True)
        adj = leaf[:, -3:]
        qs = [q0 * (1 + torch.tanh(adj[:, j:j + 1])) for j, q0 in enumerate(Q0[:nattr])]
    ys = [x + u * q for x, u, q in zip(xs, us, qs)]
    return xs, ys, torch.cat(qs, dim=1), leaf


def _worst(a, b):
    return float((a.detach().double() - b.detach()).abs().max()) if a.numel() else 0.0


@pytest.mark.parametrize("adj_cols", [225, 167, None])
@pytest.mark.parametrize("widths", [(50, 6, 30), (32, 6, 3)])
@pytest.mark.parametrize("n", [0, 1, 63, 257, 3000])
def test_quant_noise_matches_the_formula(n, widths, adj_cols):
    from gauspcc_amd.neural_gaussians import quant_noise

    xs, us, gs, gq, grid = _noise_case(n, widths, adj_cols, seed=n + widths[0] + (adj_cols or 0), dyadic=n == 1)
    before = _launches()
    dx = [x.to(DEV).requires_grad_(True) for x in xs]
    dgrid = None if grid is None else grid.to(DEV).requires_grad_(True)
    adj = None if dgrid is None else dgrid[:, -3:]
    assert adj is None or n < 2 or not adj.is_contiguous()
    out = quant_noise(dx, [u.to(DEV) for u in us], Q0, adj)
    ys, Q = out[:3], out[3]
    assert Q.shape == (n, 3) and all(y.shape == x.shape and y.dtype == torch.float32 for y, x in zip(ys, xs))
    _, y64, q64, leaf64 = _formula(xs, us, grid, torch.float64, 3)
    _, y32, q32, leaf32 = _formula(xs, us, grid, torch.float32, 3)
    for name, d, t32, t64 in [(f"y{j}", ys[j], y32[j], y64[j]) for j in range(3)] + [("Q", Q, q32, q64)]:
        e_dev, e_t32 = _worst(d, t64.detach()), _worst(t32.detach(), t64.detach())
        print(f"n={n} widths={widths} adj={adj_cols} {name}: e_dev {e_dev:.3e} e_t32 {e_t32:.3e}")
        assert e_dev <= 4 * e_t32, (name, e_dev, e_t32)
    # backward: dx is g itself, d_adj against the float64 formula
    up = [g.to(DEV) for g in gs]
    seen = {}
    mids = [x * 1.0 for x in dx]          # non-leaves, so that the tensor autograd hands on can be looked at
    for j, m in enumerate(mids):
        m.register_hook(lambda g, j=j: seen.__setitem__(j, g))
    out = quant_noise(mids, [u.to(DEV) for u in us], Q0, adj)
    torch.autograd.backward(list(out), up + [gq.to(DEV)])
    for j in range(3):
        assert seen[j].data_ptr() == up[j].data_ptr() or n == 0, j
        assert torch.equal(dx[j].grad, up[j])
    if grid is not None:
        for ys_, q_, leaf in ((y64, q64, leaf64), (y32, q32, leaf32)):
            torch.autograd.backward(list(ys_) + [q_], [g.to(DEV, leaf.dtype) for g in gs] + [gq.to(DEV, leaf.dtype)])
        assert torch.count_nonzero(dgrid.grad[:, :-3]) == 0
        e_dev, e_t32 = _worst(dgrid.grad[:, -3:], leaf64.grad[:, -3:]), _worst(leaf32.grad[:, -3:], leaf64.grad[:, -3:])
        print(f"n={n} widths={widths} adj={adj_cols} d_adj: e_dev {e_dev:.3e} e_t32 {e_t32:.3e}")
        assert e_dev <= 4 * e_t32, ("d_adj", e_dev, e_t32)
        # two runs are bit-identical
        first = dgrid.grad.clone()
        dgrid.grad = None
        out2 = quant_noise([x.detach() for x in dx], [u.to(DEV) for u in us], Q0, dgrid[:, -3:])
        assert all(torch.equal(a, b) for a, b in zip(out, out2))
        torch.autograd.backward(list(out2), up + [gq.to(DEV)])
        assert torch.equal(first, dgrid.grad)
    if n == 0:
        assert _launches() == before


def test_quant_noise_single_attribute_and_saturation():
    from gauspcc_amd.neural_gaussians import quant_noise

    xs, us, gs, gq, grid = _noise_case(257, (30,), 225, seed=5)
    dgrid = grid.to(DEV).requires_grad_(True)
    y, Q = quant_noise([xs[0].to(DEV).view(257, 10, 3)], [us[0].to(DEV).view(257, 10, 3)], [0.2], dgrid[:, -1:])
    assert y.shape == (257, 10, 3) and Q.shape == (257, 1)
    want = xs[0].double().to(DEV) + us[0].double().to(DEV) * (0.2 * (1 + torch.tanh(grid[:, -1:].double().to(DEV))))
    assert float((y.detach().view(257, 30).double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())
    (y.view(257, 30) * gs[0].to(DEV)).sum().backward()
    w64 = grid[:, -1:].double().to(DEV).requires_grad_(True)
    ((xs[0].double().to(DEV) + us[0].double().to(DEV) * (0.2 * (1 + torch.tanh(w64)))) * gs[0].double().to(DEV)).sum().backward()
    assert torch.allclose(dgrid.grad[:, -1:].double(), w64.grad, rtol=1e-5, atol=1e-6)
    # saturated tanh: the step is 0 or 2 Q0, the gradient exactly 0
    sat = torch.full((64, 3), 20.0, device=DEV)
    sat[::2] = -20.0
    sat.requires_grad_(True)
    xs3 = [torch.randn(64, w, device=DEV) for w in (50, 6, 30)]
    us3 = [torch.rand(64, w, device=DEV) - 0.5 for w in (50, 6, 30)]
    *ys, Q = quant_noise(xs3, us3, Q0, sat)
    q0 = torch.tensor(Q0, device=DEV)
    assert torch.equal(Q[::2], torch.zeros(32, 3, device=DEV)) and torch.equal(Q[1::2], (2 * q0).expand(32, 3))
    for x, u, y, q in zip(xs3, us3, ys, q0):
        assert torch.equal(y[::2], x[::2]) and torch.equal(y[1::2], x[1::2] + u[1::2] * (2 * q))
    (sum((y * torch.randn_like(y)).sum() for y in ys) + (Q * 3).sum()).backward()
    assert torch.count_nonzero(sat.grad) == 0 and sat.grad.shape == (64, 3)


def test_quant_noise_rejects_what_it_cannot_read():
    from gauspcc_amd.neural_gaussians import quant_noise

    x, u = torch.zeros(4, 6, device=DEV), torch.zeros(4, 6, device=DEV)
    with pytest.raises(ValueError, match=r"xs\[0\]"):
        quant_noise([x.double()], [u], [1.0])
    with pytest.raises(ValueError, match=r"us\[0\]"):
        quant_noise([x], [u.cpu()], [1.0])
    with pytest.raises(ValueError, match="adj"):
        quant_noise([x], [u], [1.0], torch.zeros(3, 1, device=DEV))
    with pytest.raises(ValueError, match="1..3"):
        quant_noise([x] * 4, [u] * 4, [1.0] * 4)


# ---- kernel (b): select_rows ------------------------------------------------------------------------------------------------------------

def _rows_case(n, kind, seed):
    g = torch.Generator().manual_seed(seed)
    mask = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool), "random": torch.rand(n, generator=g) < 0.4}[kind]
    ts = [torch.randn(n, w, generator=g) for w in (1, 3, 6, 30, 50)] + [torch.randn(n, 10, 3, generator=g)]
    return mask.to(DEV), [t.to(DEV) for t in ts]


@pytest.mark.parametrize("kind", ["none", "all", "random"])
@pytest.mark.parametrize("n", [0, 1, 5000])
def test_select_rows_is_the_indexing(n, kind):
    from gauspcc_amd.densify import select_rows

    mask, ts = _rows_case(n, kind, seed=n + len(kind))
    a = [t.clone().requires_grad_(True) for t in ts]
    b = [t.clone().requires_grad_(True) for t in ts]
    a[2].requires_grad_(False); b[2].requires_grad_(False)        # one that needs no gradient among ones that do
    got, want = select_rows(mask, *a), [t[mask] for t in b]
    ups = [torch.randn_like(w) for w in want]
    for x, y in zip(got, want):
        assert x.shape == y.shape and torch.equal(x, y)
    torch.autograd.backward(list(got), ups)
    torch.autograd.backward([y for y in want if y.requires_grad], [u for y, u in zip(want, ups) if y.requires_grad])
    for i, (x, y) in enumerate(zip(a, b)):
        if i == 2:
            assert x.grad is None
        else:
            assert x.grad.shape == y.grad.shape and torch.equal(x.grad, y.grad), i


def test_select_rows_limits():
    from gauspcc_amd.densify import select_rows

    n = 300
    mask = torch.rand(n, device=DEV) < 0.5
    ts = [torch.randn(n, 1 + i % 7, device=DEV).requires_grad_(True) for i in range(32)]
    got = select_rows(mask, *ts)
    sum((g * (i + 1)).sum() for i, g in enumerate(got)).backward()
    for i, t in enumerate(ts):
        assert torch.equal(got[i], t[mask]) and torch.equal(t.grad, (mask[:, None] * float(i + 1)).expand_as(t).to(torch.float32))
    with pytest.raises(ValueError, match="33 tensors"):
        select_rows(mask, *ts, ts[0])
    with pytest.raises(ValueError, match="tensor 1"):
        select_rows(mask, ts[0], ts[1].double())
    with pytest.raises(ValueError, match="mask"):
        select_rows(mask.float(), ts[0])
    before = _launches()
    empty = select_rows(mask[:0], ts[0][:0])
    empty[0].sum().backward()
    assert empty[0].shape == (0, 1) and _launches() == before


# ---- the branch -------------------------------------------------------------------------------------------------------------------------

def _synth(n, seed=3, **kw):
    from gauspcc_amd import entropy_models
    from gauspcc_amd.synth import SyntheticGaussianModelPlus

    pc = SyntheticGaussianModelPlus(n, seed=seed, device="cuda:0", **kw)
    for m in pc.encoding_xyz.modules():     # the hash grid records its graph, as in training
        if hasattr(m, "differentiable"):
            m.differentiable = True
    with torch.no_grad():   # opacity outputs well away from 0: the keep sets of the programs compared must agree
        pc.mlp_opacity[2].weight.mul_(0.05)
        pc.mlp_opacity[2].bias.copy_(torch.tensor([2.0, -2.0] * (pc.n_offsets // 2) + [2.0] * (pc.n_offsets % 2), device=DEV))
    pc.EG_mix_prob_2, pc.entropy_gaussian = entropy_models.Entropy_gaussian_mix_prob_2(Q=1), entropy_models.Entropy_gaussian(Q=1)
    pc.bound_updates = 0

    def update_anchor_bound():
        pc.bound_updates += 1
    pc.update_anchor_bound = update_anchor_bound
    return pc


def _cam(pc):
    return types.SimpleNamespace(camera_center=pc.get_anchor.mean(dim=0) + torch.tensor([0.0, 0.0, -2.0], device=DEV))


def _vis(n, frac=0.8):
    return torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) < frac


def _check(got, want, step):
    assert len(got) == 11 and len(want) == 11
    assert torch.equal(got[6], want[6]) and got[6].dtype == torch.bool
    assert not (want[5].abs() < 1e-4).any()
    for i, tol in enumerate(TOL):
        assert got[i].shape == want[i].shape and got[i].dtype == want[i].dtype, i
        err = float((got[i].detach() - want[i]).abs().max()) if got[i].numel() else 0.0
        print(f"step {step} output {i}: {err:.3e}")
        assert torch.allclose(got[i], want[i], atol=tol, rtol=tol), (i, err)
    for i in range(7, 11):
        if step > 10000:
            print(f"step {step} rate {i}: {float(got[i]):.7f} against {float(want[i]):.7f}")
            assert torch.allclose(got[i], want[i], rtol=RATE_RTOL), i
        else:
            assert got[i] is None and want[i] is None


@pytest.mark.parametrize("visible", ["most", "all"])
@pytest.mark.parametrize("step", STEPS)
def test_branch_matches_the_restatement(step, visible):
    from gauspcc_amd.hac_plus_renderer import generate_neural_gaussians

    pc = _synth(3000)
    cam, vis = _cam(pc), (_vis(3000) if visible == "most" else None)
    torch.manual_seed(step)
    got = generate_neural_gaussians(cam, pc, vis, is_training=True, step=step)
    after = torch.rand(1, device=DEV)
    assert pc.bound_updates == (1 if step == 10000 else 0)
    shadow = ShadowModel(pc, torch.float32)
    torch.manual_seed(step)
    with torch.no_grad():
        want = hacpp_branch_ref(cam, shadow, vis, step)
    assert torch.equal(after, torch.rand(1, device=DEV))         # both programs drew as many numbers
    assert shadow.bound_updates == (1 if step == 10000 else 0)
    _check(got, want, step)


class _OwnDeform(torch.nn.Module):
    """a caller's own channel-context module for feat_dim 32: one Linear on [feat | mean, scale, prob]"""
    def __init__(self, F):
        super().__init__()
        self.net = torch.nn.Linear(4 * F, 3 * F)

    def forward(self, fea_q, mean_scale):
        return torch.chunk(self.net(torch.cat([fea_q, mean_scale], dim=-1)), chunks=3, dim=-1)


def test_feat_dim_32_with_the_callers_deform_module():
    from gauspcc_amd.hac_plus_renderer import generate_neural_gaussians

    pc = _synth(1000, feat_dim=32, n_offsets=5)
    torch.manual_seed(2)
    pc.mlp_deform = _OwnDeform(32).to(DEV)
    cam, vis, step = _cam(pc), _vis(1000), 12000
    torch.manual_seed(step)
    got = generate_neural_gaussians(cam, pc, vis, is_training=True, step=step)
    torch.manual_seed(step)
    with torch.no_grad():
        want = hacpp_branch_ref(cam, ShadowModel(pc, torch.float32), vis, step)
    _check(got, want, step)
    got[7].backward()
    assert torch.count_nonzero(pc.mlp_deform.net.weight.grad) > 0


@pytest.mark.parametrize("step", [5000, 12000])
def test_nothing_visible(step):
    from gauspcc_amd.hac_plus_renderer import generate_neural_gaussians

    pc = _synth(500)
    torch.manual_seed(step)
    out = generate_neural_gaussians(_cam(pc), pc, torch.zeros(500, dtype=torch.bool, device=DEV), is_training=True, step=step)
    assert [tuple(o.shape) for o in out[:7]] == [(0, 3), (0, 3), (0, 1), (0, 3), (0, 4), (0, 1), (0,)]
    if step > 10000:
        assert all(torch.isfinite(b) for b in out[7:])
        out[7].backward()
        assert torch.count_nonzero(pc.mlp_grid[2].weight.grad) > 0
    torch.cuda.synchronize()


def test_inference_delegates():
    from gauspcc_amd import neural_gaussians
    from gauspcc_amd.hac_plus_renderer import generate_neural_gaussians

    pc = _synth(400)
    cam, vis = _cam(pc), _vis(400)
    a = generate_neural_gaussians(cam, pc, vis)
    b = neural_gaussians.generate_neural_gaussians(cam, pc, vis)
    assert len(a) == 6 and all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))
    pc.mlp_grid = torch.nn.Sequential(torch.nn.Linear(pc.encoding_xyz.output_dim, 8), torch.nn.ReLU(True), torch.nn.Linear(8, 175)).to(DEV)   # HAC's nine-way width
    with pytest.raises(ValueError, match="get_grid_mlp"):
        generate_neural_gaussians(cam, pc, vis, is_training=True, step=12000)


@pytest.mark.parametrize("step", hc.STEPS)
def test_branch_matches_the_reference_fixture(step, monkeypatch):
    """on the device, the recorded draws replayed: what the reference's own Python computed, within the fixture's stored tolerances"""
    from gauspcc_amd import entropy_models, hac_plus_renderer

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hacpp_train.npz"))
    arrays = hc.inputs()
    assert str(g["inputs_sha256"]) == hc.sha256_of(arrays)
    pc, cam, vis = hc.model(arrays, torch, DEV, torch.float32)
    pc.EG_mix_prob_2, pc.entropy_gaussian = entropy_models.Entropy_gaussian_mix_prob_2(Q=1), entropy_models.Entropy_gaussian(Q=1)
    replay = hc.Replay(arrays, step, torch)
    monkeypatch.setattr(hac_plus_renderer, "_uniform_like", replay.uniform_like)
    monkeypatch.setattr(hac_plus_renderer, "_rand_like", replay.rand_like)
    with torch.no_grad():
        res = hac_plus_renderer.generate_neural_gaussians(cam, pc, vis, is_training=True, step=step)
    assert not replay.queue and pc.bound_updates == (1 if step == 10000 else 0)
    hc.compare(res, g, step)


class _Tap:
    """calc_interp_feat that keeps what it returned, with its gradient"""
    def __init__(self, inner):
        self.inner, self.seen = inner, []

    def __call__(self, x):
        y = self.inner(x)
        y.retain_grad()
        self.seen.append(y)
        return y


class _Stored:
    """calc_interp_feat that hands out recorded features as leaves, in call order"""
    def __init__(self, feats, dtype):
        self.leaves, self.at = [f.detach().to(dtype).requires_grad_(True) for f in feats], 0

    def __call__(self, x):
        y = self.leaves[self.at]
        self.at += 1
        assert y.shape[0] == x.shape[0]
        return y


def _device_step(pc, cam, vis, step, seed, R=None, record=None):
    """one forward (and, with upstream weights R, backward of sum(out_i * R_i) + bit_per_param) of the drop-in; -> (outputs, {name: grad})"""
    from gauspcc_amd import hac_plus_renderer

    leaves = {"_anchor_feat": pc._anchor_feat, "_offset": pc._offset, "_scaling": pc._scaling, "_mask": pc._mask}
    for k, p in pc.encoding_xyz.named_parameters():
        leaves[f"hash.{k}"] = p
    for name, m in (("grid", pc.mlp_grid), ("deform", pc.mlp_deform), ("opacity", pc.mlp_opacity), ("cov", pc.mlp_cov), ("color", pc.mlp_color)):
        for k, p in m.named_parameters():
            leaves[f"mlp_{name}.{k}"] = p
    for p in leaves.values():
        p.requires_grad_(True)
        p.grad = None
    tap = _Tap(type(pc).calc_interp_feat.__get__(pc))
    pc.calc_interp_feat = tap
    uniform, rand = hac_plus_renderer._uniform_like, hac_plus_renderer._rand_like
    if record is not None:
        hac_plus_renderer._uniform_like = lambda t: record.append(uniform(t)) or record[-1]
        hac_plus_renderer._rand_like = lambda t: record.append(rand(t)) or record[-1]
    try:
        torch.manual_seed(seed)
        out = hac_plus_renderer.generate_neural_gaussians(cam, pc, vis, is_training=True, step=step)
    finally:
        hac_plus_renderer._uniform_like, hac_plus_renderer._rand_like = uniform, rand
        del pc.calc_interp_feat
    if R is None:
        return out, None, tap
    (sum((o * r).sum() for o, r in zip(out[:6], R)) + out[7]).backward()
    grads = {k: p.grad.detach().clone() for k, p in leaves.items()}
    for i, f in enumerate(tap.seen):
        grads[f"interp{i}"] = f.grad.detach().clone()
    return out, grads, tap


def test_gradients_match_float64():
    """loss = sum(outputs * fixed weights) + bit_per_param at step 12000.  The float64 and float32 restatements get the device run's draws and,
    as calc_interp_feat, the device run's hash-grid features as leaves (the hash grid has no float64 form; its own backward is
    tests/test_gpu_gridencoder_train.py's subject): the features' gradients are compared, the hash tables' must be there."""
    from gauspcc_amd import hac_plus_renderer

    pc = _synth(3000)
    cam, vis, step = _cam(pc), _vis(3000), 12000
    out, _, _ = _device_step(pc, cam, vis, step, seed=7)
    gen = torch.Generator(device=DEV).manual_seed(11)
    R = [torch.randn(o.shape, device=DEV, generator=gen) for o in out[:6]]
    draws = []
    out, got, tap = _device_step(pc, cam, vis, step, seed=7, R=R, record=draws)
    out2, got2, _ = _device_step(pc, cam, vis, step, seed=7, R=R)
    for a, b in zip(out[:7] + out[7:], out2[:7] + out2[7:]):
        assert torch.equal(a, b)                                    # two runs are bit-identical
    assert got.keys() == got2.keys() and all(torch.equal(got[k], got2[k]) for k in got)
    assert len(draws) == 7 and len(tap.seen) == 2
    for k, v in got.items():
        assert torch.count_nonzero(v) > 0, f"no gradient reaches {k}"
    ref = {}
    uniform, rand = hac_plus_renderer._uniform_like, hac_plus_renderer._rand_like
    try:
        for dtype in (torch.float64, torch.float32):
            queue = [d.to(dtype) for d in draws]
            hac_plus_renderer._uniform_like = hac_plus_renderer._rand_like = lambda t: queue.pop(0)
            interp = _Stored(tap.seen, dtype)
            sh = ShadowModel(pc, dtype, interp=interp)
            res = hacpp_branch_ref(cam, sh, vis, step)
            assert torch.equal(res[6], out[6]) and not queue
            (sum((o * r.to(dtype)).sum() for o, r in zip(res[:6], R)) + res[7]).backward()
            ref[dtype] = {k: p.grad for k, p in sh.trainable().items()}
            ref[dtype].update({f"interp{i}": f.grad for i, f in enumerate(interp.leaves)})
    finally:
        hac_plus_renderer._uniform_like, hac_plus_renderer._rand_like = uniform, rand
    bad = []
    for k, want in ref[torch.float64].items():
        e_dev, e_t32 = _worst(got[k], want), _worst(ref[torch.float32][k], want)
        print(f"{k}: e_dev {e_dev:.3e} e_t32 {e_t32:.3e} (largest |gradient| {float(want.abs().max()):.3e})")
        if not e_dev <= 4 * e_t32:
            bad.append((k, e_dev, e_t32))
    assert not bad, bad


def test_it_trains():
    """100 Adam steps on the context model, the channel-context MLP and the features lower bit_per_param (looked at under one fixed seed)"""
    from gauspcc_amd.hac_plus_renderer import generate_neural_gaussians

    pc = _synth(3000, seed=9)
    cam, vis = _cam(pc), _vis(3000)
    params = [pc._anchor_feat] + list(pc.mlp_grid.parameters()) + list(pc.mlp_deform.parameters())
    for p in params:
        p.requires_grad_(True)

    def bits(seed):
        torch.manual_seed(seed)
        return generate_neural_gaussians(cam, pc, vis, is_training=True, step=12000)[7]

    with torch.no_grad():
        before = float(bits(1000))
    opt = torch.optim.Adam(params, lr=2e-3)
    for it in range(100):
        opt.zero_grad()
        bits(it).backward()
        opt.step()
    with torch.no_grad():
        after = float(bits(1000))
    print(f"bit_per_param {before:.4f} -> {after:.4f}")
    assert np.isfinite(after) and after < before, (before, after)
