"""GPU tests of TC-GS's training branch: the context-row kernels (gsge_plane_rows_forward / _backward through triplane_rows), the one-launch
quantiser (gsnn_quantise through quantise_steps), gauspcc_amd.tcgs_renderer.generate_neural_gaussians against tests/tcgs_branch_ref.py and
against what the reference's own Python computed (tests/golden/tcgs_train.npz), and tcgs_codec.estimate_final_bits.

Accuracy criterion of the gradients (the project's rule, no tolerance fixed in advance): e_dev = max |device - float64| must not exceed
4 x e_t32 = max |float32 torch program on the same GPU - float64|."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triplane_ref as tref  # noqa: E402

from tests import tcgs_train_cases as tc  # noqa: E402
from tests.tcgs_branch_ref import PlaneRef, ShadowModel, estimate_bits_ref, tcgs_branch_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcgs_train.npz")
TOL = (2e-5, 2e-5, 2e-5, 2e-5, 5e-5, 2e-5)
RATE_RTOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


@pytest.fixture(scope="module")
def arrays():
    return tc.inputs()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _launches():
    from gauspcc_amd import _lib
    return _lib.lib().gpcc_debug_launches(0)


def _worst(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max()) if a.numel() else 0.0


def _biteq(a, b):
    """equal bit patterns: NaN payloads and signed zeros included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the context rows -------------------------------------------------------------------------------------------------------------------
# a forward workgroup owns floor(64 / K) anchors: K = 4 -> 16, K = 3 -> 21, K = 1 -> 64; the N below sit on, beside and past those sizes
ROW_N = {4: (1, 15, 16, 17, 21, 33), 3: (20, 21, 22, 43), 1: (1, 63, 64, 65, 129)}


def _row_case(N, K, C, T, H, W, repeat, seed):
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(3, C, H, W, generator=g)
    co = tref.make_coordinates(N, K, seed).float()          # inside and outside the contraction's ball, far outside the plane, the origin
    if N > 2:
        co[N // 2] = float("nan")                           # one NaN row: zero features, the tail still copied
    if repeat:
        co = co[:, 0, :].contiguous()
    tail = torch.randn(N, T, generator=g)
    up = torch.randn(N, K * 3 * C + T, generator=g)
    return planes.to(DEV), co.to(DEV), tail.to(DEV), up.to(DEV)


@pytest.mark.parametrize("repeat", [False, True], ids=["nk3", "repeat"])
@pytest.mark.parametrize("KCT", [(4, 50, 3), (1, 1, 3), (3, 7, 2), (4, 50, 0)], ids=lambda t: "K%d-C%d-T%d" % t)
def test_context_rows_are_the_sampler_and_the_tail(KCT, repeat):
    from gauspcc_amd.triplane import triplane_rows, triplane_sample

    K, C, T = KCT
    mx, mn = tref.bounds(device=DEV)
    for H, W in ((8, 8), (12, 16)):
        for N in ROW_N[K]:
            planes, co, tail, up = _row_case(N, K, C, T, H, W, repeat, seed=N + K + C)
            rep = K if repeat else None
            row = K * 3 * C

            def run(tail_is_coords=False):
                p, c = planes.clone().requires_grad_(True), co.clone().requires_grad_(True)
                t = c if tail_is_coords else tail.clone().requires_grad_(True)
                out = triplane_rows(p, c, t, mx, mn, tref.RADII, repeat=rep)
                u = up if not tail_is_coords else torch.cat([up[:, :row], up[:, :3]], dim=1)
                return (out.detach(), *torch.autograd.grad(out, (p, c) if tail_is_coords else (p, c, t), u))

            out, gp, gc, gt = run()
            p, c = planes.clone().requires_grad_(True), co.clone().requires_grad_(True)
            feat = triplane_sample(p, c, mx, mn, tref.RADII, repeat=rep)
            gp0, gc0 = torch.autograd.grad(feat, (p, c), up[:, :row].contiguous())
            tag = f"N={N} K={K} C={C} T={T} {H}x{W} repeat={repeat}"
            assert out.shape == (N, row + T), tag
            assert _biteq(out[:, :row], feat.detach()) and _biteq(out[:, row:], tail), tag       # the sampler's features; the tail's bits (T = 0: gsge_plane_forward)
            if N > 2:
                assert not out[N // 2, :row].any(), tag                                          # the NaN row: zeros
            assert _biteq(gp, gp0) and _biteq(gc, gc0), tag
            assert _biteq(gt, up[:, row:]), tag
            out2, gp2, gc2, gt2 = run()
            assert _biteq(out, out2) and _biteq(gp, gp2) and _biteq(gc, gc2), tag                # two runs are bitwise equal
            if repeat and T == 3:       # the tail is the coordinate tensor: autograd adds the two gradients
                _, gp3, gc3 = run(tail_is_coords=True)
                assert _biteq(gp3, gp0) and _biteq(gc3, gc0 + up[:, :3]), tag


@pytest.mark.parametrize("repeat", [0, 1])
def test_context_rows_write_nothing_past_the_tensor(repeat):
    """the forward into the middle of an over-allocated buffer: the bytes before and after the (N, K 3 C + T) tensor keep their pattern"""
    from gauspcc_amd import _lib, runtime

    mx, mn = tref.bounds(device=DEV)
    for K, C, T, N in ((4, 50, 3, 17), (3, 7, 2, 22), (1, 1, 3, 65), (4, 50, 0, 33)):
        planes, co, tail, _ = _row_case(N, K, C, T, 8, 8, bool(repeat), seed=N)
        total, pad = N * (K * 3 * C + T), 1024
        buf = torch.full((total + 2 * pad,), -123.25, device=DEV)
        out = buf[pad:pad + total]
        _lib.check(_lib.lib().gsge_plane_rows_forward(runtime.context(DEV), planes.data_ptr(), co.data_ptr(), mx.data_ptr(), mn.data_ptr(), float(tref.RADII),
                                                      N, K, repeat, C, 8, 8, tail.data_ptr() if T else None, T, out.data_ptr(),
                                                      runtime.Workspace(DEV).fn(), None, runtime.stream_ptr(DEV)))
        torch.cuda.synchronize()
        assert (buf[:pad] == -123.25).all() and (buf[pad + total:] == -123.25).all(), (K, C, T, N)
        assert not (out == -123.25).any()            # every element of the tensor is written


def test_context_rows_refuse_what_they_cannot_read():
    from gauspcc_amd.triplane import Triplane, triplane_rows

    mx, mn = tref.bounds(device=DEV)
    planes = torch.randn(3, 4, 8, 8, device=DEV)
    co = torch.rand(5, 3, device=DEV)
    with pytest.raises(ValueError, match="tail"):
        triplane_rows(planes, co, torch.zeros(5, 17, device=DEV), mx, mn, 1.5, repeat=4)
    with pytest.raises(ValueError, match="tail"):
        triplane_rows(planes, co, torch.zeros(4, 3, device=DEV), mx, mn, 1.5, repeat=4)
    with pytest.raises(TypeError, match="float32"):
        triplane_rows(planes, co, co.double(), mx, mn, 1.5, repeat=4)
    before = _launches()
    assert triplane_rows(planes, co[:0], co[:0], mx, mn, 1.5, repeat=4).shape == (0, 51) and _launches() == before
    tri = Triplane(4, 8, 3.0, device=DEV).to(DEV)
    rows, comp, rec = tri.context_rows(co, co, mx, mn, is_training=1, step=20000, repeat=4)
    assert rows.shape == (5, 51) and comp.shape[0] == 3 and rec.shape == tri.planes.shape
    assert tri.context_rows(co, co, mx, mn, is_training=1, step=12000, repeat=4)[1:] == (None, None)
    assert torch.equal(tri.context_rows(co, co, mx, mn, repeat=4), rows.detach())


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------------

def _ste_torch(x, q, m):
    q = q.view(-1, *([1] * (x.dim() - 1)))
    return torch.round(torch.clamp(x, min=m - 15000 * q, max=m + 15000 * q) / q) * q


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_quantise_steps_is_the_torch_expression(n):
    from gauspcc_amd.neural_gaussians import fixed_order_mean, quantise_steps

    g = torch.Generator().manual_seed(n)
    q0 = (1, 0.001, 0.3, 0.2)
    shapes = ((n, 50), (n, 6), (n, 10, 3), (n, 3))
    ctx = torch.randn(n, 175, generator=g).to(DEV)
    if n > 2:
        ctx[1, 172:] = -20.0                                # 1 + tanh(-20) = 0: Q = 0, the results are not finite
    xs = [(torch.randn(s, generator=g) * (1.0 if j != 1 else 0.05)).to(DEV) for j, s in enumerate(shapes)]
    xs[1].view(-1)[::5] += 40.0                             # beyond mean + 15000 Q (Q about 1e-3)
    xs[1].view(-1)[2::7] -= 60.0                            # and below mean - 15000 Q
    for sel in ((0, 1, 2), (3,), (1, 3)):
        x_sel, q_sel = [xs[j] for j in sel], [q0[j] for j in sel]
        cols = [172 + i for i in range(len(sel))]
        means = [x.mean() + 0.25 for x in x_sel]
        before = _launches()
        *ys, Q = quantise_steps(x_sel, q_sel, ctx, cols=cols, means=means)
        assert _launches() == before + 1                    # one launch
        *ys_v, Q_v = quantise_steps(x_sel, q_sel, ctx[:, 172:], means=means)
        assert _biteq(Q, Q_v) and all(_biteq(a, b) for a, b in zip(ys, ys_v))        # a column slice of the wider matrix, read in place
        assert Q.shape == (n, len(sel))
        for i, (x, y) in enumerate(zip(x_sel, ys)):
            want_q = q_sel[i] * (1 + torch.tanh(ctx[:, cols[i]]))
            ulp = torch.abs(torch.nextafter(want_q, torch.full_like(want_q, float("inf"))) - want_q)
            assert (torch.abs(Q[:, i] - want_q) <= 4 * ulp).all(), (sel, i)
            want = _ste_torch(x, Q[:, i], means[i].to(torch.float32))
            assert y.shape == x.shape and torch.equal(torch.isnan(y), torch.isnan(want)), (sel, i)
            ok = ~torch.isnan(want)
            assert _biteq(y[ok], want[ok]), (sel, i, _worst(y[ok], want[ok]))
            if n > 2:
                assert not torch.isfinite(y[1]).any()
        # no means: input.mean(), formed by the library's fixed-order sum
        *ys_n, Q_n = quantise_steps(x_sel, q_sel, ctx, cols=cols)
        m = fixed_order_mean(*x_sel)
        assert _biteq(m, fixed_order_mean(*x_sel))
        *ys_m, _ = quantise_steps(x_sel, q_sel, ctx, cols=cols, means=list(m))
        assert _biteq(Q_n, Q) and all(_biteq(a, b) for a, b in zip(ys_n, ys_m))
        for x, mj in zip(x_sel, m):
            exact = x.double().mean()
            assert abs(float(mj) - float(exact)) <= abs(float(exact)) * 2.0 ** -23 + 1e-30, (float(mj), float(exact))
            # x.mean() in float32: a pairwise sum of k terms is off by at most about log2(k) ulps of mean |x|; 16 covers k < 2^16
            assert abs(float(mj) - float(x.mean())) <= 16 * 2.0 ** -23 * float(x.double().abs().mean())


def test_quantise_steps_follows_use_clamp(monkeypatch):
    from gauspcc_amd import anchor_codec
    from gauspcc_amd.neural_gaussians import quantise_steps

    x = torch.tensor([[100.0, -100.0, 0.4]], device=DEV)
    adj = torch.zeros(1, 1, device=DEV)
    y, Q = quantise_steps([x], [0.001], adj, means=[0.0])
    q = Q[0, 0]
    assert float(q) == pytest.approx(0.001) and torch.equal(y, torch.round(torch.clamp(x, min=0.0 - 15000 * q, max=0.0 + 15000 * q) / q) * q)
    assert float(y[0, 0]) == pytest.approx(15.0) and float(y[0, 1]) == pytest.approx(-15.0) and float(y[0, 2]) == pytest.approx(0.4)
    monkeypatch.setattr(anchor_codec, "USE_CLAMP", False)
    y, _ = quantise_steps([x], [0.001], adj, means=[0.0])
    assert torch.equal(y, torch.round(x / Q[0, 0]) * Q[0, 0])


# ---- the branch against the reference's own Python --------------------------------------------------------------------------------------

def _device_model(arrays, decoded=False, dtype=torch.float32):
    from gauspcc_amd import entropy_models

    pc, cam, vis = tc.model(arrays, torch, DEV, dtype, decoded=decoded)
    pc.entropy_gaussian = entropy_models.Entropy_gaussian(Q=1)
    return pc, cam, vis


def _replayed(source, fn, monkeypatch):
    from gauspcc_amd import tcgs_renderer

    monkeypatch.setattr(tcgs_renderer, "_uniform_like", source.uniform_like)
    monkeypatch.setattr(tcgs_renderer, "_rand_like", source.rand_like)
    res = fn()
    assert not source.queue
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
    for i in range(7, 12) if train else []:
        if isinstance(want[i], torch.Tensor):
            assert rates
            print(f"scalar {i}: {float(got[i].detach()):.7f} against {float(want[i].detach()):.7f}")
            assert torch.allclose(got[i], want[i], rtol=RATE_RTOL), i
        else:
            assert got[i] is None and want[i] is None, i


@pytest.mark.parametrize("tag", [r[0] for r in tc.RUNS])
def test_branch_matches_the_reference_fixture(tag, arrays, golden, monkeypatch):
    """on the device, the recorded draws replayed: what the reference's own Python computed, within the fixture's stored tolerances (the kept
    set equal), the float32 restatement on the same GPU, and the hooks in the recorded order"""
    from gauspcc_amd import tcgs_renderer

    assert str(golden["inputs_sha256"]) == tc.sha256_of(arrays)
    _, train, step, with_vis, decoded = tc.run(tag)
    pc, cam, vis = _device_model(arrays, decoded)
    vis = vis if with_vis else None
    with torch.no_grad():
        res = _replayed(tc.Replay(arrays, tag, torch), lambda: tcgs_renderer.generate_neural_gaussians(cam, pc, vis, is_training=train, step=step), monkeypatch)
    assert pc.hooks == tc.expected_hooks(step, train)
    assert pc.triplane.calls == ([(True, step)] if train and step > 10000 else [(False, 0)] if not train and not decoded else [])
    tc.compare(res, golden, tag)
    pc2, _, _ = _device_model(arrays, decoded)
    with torch.no_grad():
        want = _replayed(tc.Replay(arrays, tag, torch), lambda: tcgs_branch_ref(cam, pc2, vis, step, is_training=train), monkeypatch)
    _check(res, want, train, train and step > 10000)
    if not train:
        assert isinstance(res[5], int if decoded else float) and res[5] >= 0          # time_sub


# ---- gradients on a second, seeded model ------------------------------------------------------------------------------------------------

class _Recorder:
    """the renderer's two hooks: the first run draws from torch's generator and records, later runs replay the record in their own dtype"""

    def __init__(self):
        self.record, self.queue = [], []

    def rewind(self):
        self.queue = list(self.record)

    def _next(self, t, draw):
        if self.queue:
            d = self.queue.pop(0)
            assert d.shape == t.shape
            return d.to(t.dtype)
        d = draw(t)
        self.record.append(d)
        return d

    def uniform_like(self, t):
        return self._next(t, lambda t: torch.empty_like(t).uniform_(-0.5, 0.5))

    def rand_like(self, t):
        return self._next(t, torch.rand_like)


def _seeded_model(n, tri, mlp, seed=5):
    from gauspcc_amd import entropy_models
    from gauspcc_amd.mlp import ContextMLP
    from gauspcc_amd.synth import SyntheticGaussianModelTC

    class Model(SyntheticGaussianModelTC):
        get_anchor = property(lambda self: self._anchor_leaf)

        def updatebbox(self):
            self.hooks.append("updatebbox")

        def init_knn_indice(self, k):
            self.hooks.append(("init_knn_indice", k))

    pc = Model(n, seed=seed, resolution=32, device="cuda:0")
    pc.hooks = []
    pc._anchor_leaf = (torch.round(pc._anchor / pc.voxel_size) * pc.voxel_size).detach().requires_grad_(True)
    with torch.no_grad():   # opacity outputs well away from 0: the keep sets of the programs compared must agree; planes with some relief
        pc.mlp_opacity[2].weight.mul_(0.05)
        pc.mlp_opacity[2].bias.copy_(torch.tensor([2.0, -2.0] * (pc.n_offsets // 2) + [2.0] * (pc.n_offsets % 2), device=DEV))
        pc.triplane.planes.mul_(30.0)
        F, Ko = pc.feat_dim, pc.n_offsets       # the scale heads positive by bias, the scaling mean head near the scalings, as a trained context's
        for lo, hi, gain, bias in ((F, 2 * F, 0.1, 1.0), (2 * F, 2 * F + 6, 0.001, 0.011), (2 * F + 6, 2 * F + 12, 0.01, 0.05),
                                   (2 * F + 12 + 3 * Ko, 2 * F + 12 + 6 * Ko, 0.1, 0.3)):
            pc.mlp_triplane[2].weight[lo:hi].mul_(gain); pc.mlp_triplane[2].bias[lo:hi].fill_(bias)
    for t in (pc._anchor_feat, pc._offset, pc._scaling, pc._mask):
        t.requires_grad_(True)
    pc.library_plane = pc.triplane
    if tri == "torch":      # a plain torch module in the tri-plane's place: the drop-in calls it as the reference does and concatenates
        pc.triplane = PlaneRef(pc.library_plane.planes.detach(), pc.library_plane.radii, copy.deepcopy(pc.library_plane.autoencoder)).to(DEV)
    if mlp == "context":
        pc.mlp_triplane = ContextMLP.from_sequential(pc.mlp_triplane)
    pc.entropy_gaussian = entropy_models.Entropy_gaussian(Q=1)
    return pc


def _cam(pc):
    return types.SimpleNamespace(camera_center=pc.get_anchor.detach().mean(dim=0) + torch.tensor([0.0, 0.0, -2.0], device=DEV))


def _loss(res, R):
    return sum((o * r.to(o)).sum() for o, r in zip(res[:6], R)) + res[7] + (res[11] if res[11] is not None else 0)


@pytest.mark.parametrize("mlp", ["sequential", "context"])
@pytest.mark.parametrize("tri", ["library", "torch"])
@pytest.mark.parametrize("step", [12000, 20000])
def test_gradients_match_float64(step, tri, mlp, monkeypatch):
    """loss = sum(outputs * fixed weights) + bit_per_param + lae: the drop-in's gradients of anchor, feat, offsets, scaling, mask, planes and
    every Linear against the float64 restatement, within 4 x the float32 torch restatement's own error on the same GPU; the repeat form
    (step 12000: the anchor is coordinate and tail at once) and pc.knnanchor (step 20000)"""
    from gauspcc_amd import tcgs_renderer
    from gauspcc_amd.triplane import Triplane

    pc = _seeded_model(300, tri, mlp)
    assert isinstance(pc.triplane, Triplane) == (tri == "library")
    cam = _cam(pc)
    leaves = {"anchor": pc._anchor_leaf, "_anchor_feat": pc._anchor_feat, "_offset": pc._offset, "_scaling": pc._scaling, "_mask": pc._mask,
              "triplane.planes": pc.triplane.planes}
    for name, m in (("tri_mlp", pc.mlp_triplane), ("opacity", pc.mlp_opacity), ("cov", pc.mlp_cov), ("color", pc.mlp_color)):
        for k, p in m.named_parameters():
            leaves[f"{name}.{k}"] = p
    rec = _Recorder()

    def device_run():
        for p in leaves.values():
            p.grad = None
        rec.rewind()
        return _replayed(rec, lambda: tcgs_renderer.generate_neural_gaussians(cam, pc, None, is_training=True, step=step), monkeypatch)

    torch.manual_seed(step)
    res = device_run()
    assert (res[11] is not None) == (step > 15000) and pc.hooks == []
    gen = torch.Generator(device=DEV).manual_seed(11)
    R = [torch.randn(o.shape, device=DEV, generator=gen) for o in res[:6]]
    _loss(res, R).backward()
    got = {k: p.grad.detach().clone() for k, p in leaves.items()}
    res2 = device_run()
    _loss(res2, R).backward()
    assert all(torch.equal(a, b) for a, b in zip(res[:11], res2[:11]))                 # two runs are bit-identical
    if tri == "library":      # (torch's grid_sample adds its plane gradient with float atomics: the stand-in's own gradients vary from run to run)
        assert all(torch.equal(got[k], p.grad) for k, p in leaves.items())
    for k, v in got.items():
        assert torch.count_nonzero(v) > 0, f"no gradient reaches {k}"
    ref = {}
    for dtype in (torch.float64, torch.float32):
        plane = PlaneRef(pc.library_plane.planes.detach().to(dtype), pc.library_plane.radii, copy.deepcopy(pc.library_plane.autoencoder).to(dtype)).to(DEV)
        plain = torch.nn.Sequential(*[copy.deepcopy(m) for m in pc.mlp_triplane]).to(device=DEV, dtype=dtype)      # torch's own Linear - ReLU - Linear
        sh = ShadowModel(pc, dtype, triplane=plane, tri_mlp=plain)
        rec.rewind()
        out = _replayed(rec, lambda: tcgs_branch_ref(cam, sh, None, step), monkeypatch)
        assert torch.equal(out[6], res[6])
        _loss(out, R).backward()
        ref[dtype] = {k: p.grad for k, p in sh.trainable().items()}
    assert set(ref[torch.float64]) == set(got), set(ref[torch.float64]) ^ set(got)
    bad = []
    for k, want in ref[torch.float64].items():
        e_dev, e_t32 = _worst(got[k], want), _worst(ref[torch.float32][k], want)
        print(f"step {step} {tri} {mlp} {k}: e_dev {e_dev:.3e} e_t32 {e_t32:.3e} (largest |gradient| {float(want.abs().max()):.3e})")
        if not e_dev <= 4 * e_t32:
            bad.append((k, e_dev, e_t32))
    assert not bad, bad


def test_two_seeded_runs_are_bitwise_equal_and_draw_as_the_restatement():
    """no hooks replaced: under one torch.manual_seed two runs agree bit for bit, and the float32 restatement draws the same numbers"""
    from gauspcc_amd.tcgs_renderer import generate_neural_gaussians

    pc = _seeded_model(300, "library", "sequential")
    cam = _cam(pc)
    for step in (5000, 20000):
        runs = []
        for _ in range(2):
            torch.manual_seed(step + 20)
            with torch.no_grad():
                runs.append(generate_neural_gaussians(cam, pc, None, is_training=True, step=step))
        after = torch.rand(1, device=DEV)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(*runs))
        torch.manual_seed(step + 20)
        with torch.no_grad():
            want = tcgs_branch_ref(cam, pc, None, step)
        assert torch.equal(after, torch.rand(1, device=DEV))         # both programs drew as many numbers
        _check(runs[0], want, True, step > 10000)


def test_hooks_fire_in_the_recorded_order(arrays):
    from gauspcc_amd.tcgs_renderer import generate_neural_gaussians

    pc, cam, _ = _device_model(arrays)
    torch.manual_seed(0)
    with torch.no_grad():
        for step in (9999, 10000, 10001, 14999, 15000, 15001):
            generate_neural_gaussians(cam, pc, None, is_training=True, step=step)
        generate_neural_gaussians(cam, pc, None, is_training=False, step=10000)
        generate_neural_gaussians(cam, pc, None, is_training=False, step=15000)
    assert pc.hooks == ["updatebbox", ("init_knn_indice", 4)]
    # steps up to 15000 sample the anchor itself (the stand-in sees K equal rows), later ones pc.knnanchor
    assert [c for c in pc.triplane.calls if c[0]] == [(True, s) for s in (10001, 14999, 15000, 15001)]


def test_edges(arrays):
    from gauspcc_amd.tcgs_renderer import generate_neural_gaussians

    pc, cam, vis = _device_model(arrays)
    n = pc.get_anchor.shape[0]
    # pc.knnanchor with another row count than the gathered anchors: the reference fails in torch.cat
    with pytest.raises(ValueError, match=f"knnanchor has {n} rows, the gathered anchors {int(vis.sum())}"):
        generate_neural_gaussians(cam, pc, vis, is_training=True, step=20000)
    # an empty visible set
    none = torch.zeros(n, dtype=torch.bool, device=DEV)
    for decoded in (False, True):
        pc.decoded_version = decoded
        out = generate_neural_gaussians(cam, pc, none, is_training=False)
        assert len(out) == 6 and [tuple(o.shape) for o in out[:5]] == [(0, 3), (0, 3), (0, 1), (0, 3), (0, 4)] and out[5] == 0
    pc.decoded_version = False
    # visible_mask=None is every anchor in evaluation too (un-decoded: the context and the quantisation run on all of them)
    a = generate_neural_gaussians(cam, pc, None, is_training=False)
    b = generate_neural_gaussians(cam, pc, torch.ones(n, dtype=torch.bool, device=DEV), is_training=False)
    assert a[0].shape[0] > 0 and all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))
    # a context of another width is refused
    pc.get_tri_mlp = lambda rows: rows.new_zeros(rows.shape[0], 170)
    with pytest.raises(ValueError, match="get_tri_mlp"):
        generate_neural_gaussians(cam, pc, None, is_training=True, step=12000)
    torch.cuda.synchronize()


# ---- estimate_final_bits ----------------------------------------------------------------------------------------------------------------

def test_estimate_final_bits_matches_the_restatement(capsys):
    from gauspcc_amd import tcgs_codec

    pc = _seeded_model(300, "library", "sequential", seed=8)
    assert pc.triplane.autoencoder.encoder is not None
    log = tcgs_codec.estimate_final_bits(pc)
    assert pc.triplane.autoencoder.encoder is None                   # the reference's side effect
    printed = capsys.readouterr().out.strip().splitlines()[-1].split()
    assert len(printed) == 6
    kept = int(pc.get_mask_anchor.sum())
    assert pc.knn_indices.shape == (kept, 4) and pc.knnanchor.shape == (kept, 4, 3) and int(printed[0]) == kept * 3 * 16
    assert torch.equal(pc.knn_indices[:, 0], torch.arange(kept, device=DEV))
    sh = ShadowModel(pc, torch.float64, triplane=PlaneRef(pc.library_plane.planes.detach().double(), pc.library_plane.radii).to(DEV),
                     tri_mlp=torch.nn.Sequential(*[copy.deepcopy(m) for m in pc.mlp_triplane]).to(device=DEV, dtype=torch.float64))
    sh._anchor = pc._anchor.detach().double()
    want = estimate_bits_ref(sh, pc.knn_indices)
    for name, got, w in zip(("feat", "scaling", "offsets"), printed[1:4], want):
        rel = abs(float(got) - w) / abs(w)
        print(f"estimate_final_bits {name}: {float(got):.4f} against {w:.4f}, {rel:.3e} relative")
        assert rel <= 1e-5, (name, got, w)
    assert log.startswith("\nEstimated sizes in MB: anchor ") and ", triplane " in log and ", Total " in log
