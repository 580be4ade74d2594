"""gsarm_rate_forward / gsarm_rate_backward (gauspcc_amd.arm) on the device: the rate of CAT-3DGS's tri-plane latents under its ARM.

Accuracy criterion (that of tests/test_gpu_rate.py and tests/test_gpu_mlp_train.py, no tolerance fixed in advance): for the rate, mu,
scale and every gradient, e_dev = max |device - float64 restatement| (tests/arm_ref.py) must not exceed 4 x e_t32, the same error of a
float32 torch sequence on the same inputs -- the reference's own recorded values for the golden cases, arm_ref.rate_torch on the same
GPU for the rest -- plus a floor of 1e-6 (absolute for rate, mu and scale, of the largest magnitude for a gradient) for quantities the
float32 sequence gets exactly.  Gradients of latents whose probability lies within 0.1 % of the 2^-16 floor may be left out (their
upstream weight is zeroed on both sides), at most 1 % of a case's latents; the golden fixtures have none.  Rates are compared for every
latent.  Measured ratios e_dev / e_t32: profiles/r07_arm_rate.txt."""
import functools
import os

import numpy as np
import pytest
import torch

from gauspcc_amd import arm as A
from tests import arm_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arm_rate.npz")
FACTOR = 4.0
SPEC_TILE, ANY_TILE, GRID = 256, 128, 1024      # latents per workgroup of the two kernels, and the persistent grid's size


@functools.lru_cache(maxsize=None)
def _golden(key):
    return arm_ref.golden_case(np.load(GOLDEN), key)


def _arm(layers, params):
    arm = A.ArmMLP(12, layers)
    arm.load_state_dict({k: torch.as_tensor(p) for k, p in zip(arm.state_dict().keys(), params)})
    return arm.to(DEV)


def _run(levels, arm, w=None, reduce="none", return_params=True):
    """forward + backward on the device; levels: tensors or arrays shaped [1, C, H, W]"""
    leaves = [torch.as_tensor(y).to(DEV).detach().clone().requires_grad_(True) for y in levels]
    for p in arm.parameters():
        p.grad = None
    out = A.arm_rate(leaves, arm, reduce=reduce, return_params=return_params)
    rate, mu, scale = out if return_params else (out, None, None)
    loss = rate.sum() if w is None else (rate * torch.as_tensor(w).to(DEV)).sum()
    loss.backward()
    return {"rate": rate.detach(), "mu": mu, "scale": scale, "g_levels": [y.grad for y in leaves],
            "g_params": [p.grad.clone() for p in arm.parameters()]}


def _torch32(levels, params, w):
    leaves = [torch.as_tensor(y, dtype=torch.float32).to(DEV).requires_grad_(True) for y in levels]
    ps = [torch.as_tensor(p, dtype=torch.float32).to(DEV).requires_grad_(True) for p in params]
    rate, mu, scale = arm_ref.rate_torch(leaves, ps)
    (rate * torch.as_tensor(w, dtype=torch.float32).to(DEV)).sum().backward()
    return {"rate": rate.detach(), "mu": mu.detach(), "scale": scale.detach(), "g_levels": [y.grad for y in leaves], "g_params": [p.grad for p in ps]}


def _np(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _criterion(tag, dev, t32, want, relative):
    want = _np(want)
    e_dev, e_t32 = float(np.abs(_np(dev).reshape(want.shape) - want).max()), float(np.abs(_np(t32).reshape(want.shape) - want).max())
    floor = 1e-6 * (max(float(np.abs(want).max()), 1e-30) if relative else 1.0)
    print(f"{tag}: e_dev {e_dev:.3e}  e_t32 {e_t32:.3e}  ratio {e_dev / e_t32 if e_t32 else float('inf') if e_dev else 0.0:.2f}")
    return e_dev <= FACTOR * e_t32 + floor, (tag, e_dev, e_t32)


def _compare(tag, dev, t32, f64, g64_levels, g64_params):
    """every quantity by the criterion; all the figures are printed before the first failure is raised"""
    checks = []
    for name in ("rate", "mu", "scale"):
        flat = torch.cat([m.reshape(-1) for m in dev[name]]) if isinstance(dev[name], (list, tuple)) else dev[name]
        checks.append(_criterion(f"{tag} {name}", flat, t32[name], f64[name], False))
    for i, want in enumerate(g64_levels):
        checks.append(_criterion(f"{tag} g_level{i}", dev["g_levels"][i], t32["g_levels"][i], want, True))
    for j, want in enumerate(g64_params):
        checks.append(_criterion(f"{tag} g_param{j}", dev["g_params"][j], t32["g_params"][j], want, True))
    for ok, what in checks:
        assert ok, what


def _leave_out(f64, w):
    """zero the upstream weight of latents within 0.1 % of the floor: at most 1 % of the case"""
    near = arm_ref.near_floor(f64["p0"], 1e-3)
    assert near.sum() <= 0.01 * near.size, (int(near.sum()), near.size)
    return np.where(near, 0.0, w).astype(np.float32)


@pytest.mark.parametrize("key", arm_ref.CASES)
def test_reference_golden(key):
    c = _golden(key)
    f64 = arm_ref.forward64(c["levels"], c["params"])
    assert arm_ref.near_floor(f64["p0"], 1e-3).sum() == 0          # nothing to leave out on these fixtures
    g64_levels, g64_params, _ = arm_ref.grads64(c["levels"], c["params"], c["w"], f64)
    dev = _run(c["levels"], _arm(c["layers"], c["params"]), c["w"])
    assert dev["rate"].shape == (535,) and dev["rate"].dtype == torch.float32
    assert [tuple(m.shape) for m in dev["mu"]] == [y.shape[1:] for y in c["levels"]] == [tuple(s.shape) for s in dev["scale"]]
    for g, y in zip(dev["g_levels"], c["levels"]):
        assert g.shape == y.shape
    _compare(key, dev, {"rate": c["rate"], "mu": c["mu"], "scale": c["scale"], "g_levels": c["g_levels"], "g_params": c["g_params"]}, f64,
             g64_levels, g64_params)
    # the floor set is the reference's, and those rates are exactly 16 bits
    assert torch.equal(dev["rate"].cpu() == 16.0, torch.from_numpy(c["rate"] == 16.0))


def _random_levels(shapes, seed, outliers=True):
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in shapes:
        y = torch.round(torch.randn((1,) + tuple(s), generator=g) * 1.5) + (torch.rand((1,) + tuple(s), generator=g) - 0.5)
        if outliers:
            y.view(-1)[::11] += 40.0                           # on the 2^-16 floor
        out.append(y)
    return out


# planes 1 x 1, 1 x 2, 6 x 1, 3 x 2; C = 1, 2, 3, 72; one below, at and above a workgroup's tile; more tiles than persistent workgroups;
# several levels of different sizes in one call
EDGES = {
    "1x1": [(1, 1, 1)], "1x2": [(1, 1, 2)], "6x1": [(1, 6, 1)], "3x2": [(1, 3, 2)], "c2": [(2, 5, 7)], "c3": [(3, 4, 9)],
    "tile-1": [(1, 15, 17)], "tile": [(1, 16, 16)], "tile+1": [(1, 1, 257)], "half-1": [(1, 1, 127)], "half": [(2, 8, 8)], "half+1": [(1, 3, 43)],
    "c72": [(72, 9, 11)], "levels": [(2, 5, 7), (2, 10, 14), (2, 3, 3), (2, 1, 1)],
    "grid+": [(72, 61, 61)], "grid+half": [(72, 43, 43)],
}
assert 72 * 61 * 61 > GRID * SPEC_TILE > 72 * 60 * 60 and 72 * 43 * 43 > GRID * ANY_TILE


# each kernel has its own shape that outruns its persistent grid
PAIRS = [(e, n) for e in sorted(EDGES) for n in ("round", "wide") if (e, n) not in (("grid+", "wide"), ("grid+half", "round"))]


@pytest.mark.parametrize("edge,net", PAIRS, ids=lambda v: str(v))
def test_edges_against_float64(edge, net):
    c = _golden(net)
    levels = _random_levels(EDGES[edge], seed=len(edge) + 31 * len(EDGES[edge]))
    n = sum(y.numel() for y in levels)
    w = torch.randn(n, generator=torch.Generator().manual_seed(5)).numpy()
    f64 = arm_ref.forward64([y.numpy() for y in levels], c["params"])
    if n >= 100:
        w = _leave_out(f64, w)
    g64_levels, g64_params, _ = arm_ref.grads64(levels, c["params"], w, f64)
    dev = _run(levels, _arm(c["layers"], c["params"]), w)
    t32 = _torch32(levels, c["params"], w)
    _compare(f"{edge}/{net}", dev, t32, f64, g64_levels, g64_params)


def test_non_contiguous_latent_and_single_tensor():
    c = _golden("round")
    arm = _arm(c["layers"], c["params"])
    base = _random_levels([(3, 9, 6)], seed=2)[0].to(DEV)
    y = base.transpose(2, 3)                                  # [1, 3, 6, 9], not contiguous
    assert not y.is_contiguous()
    b = y.contiguous().detach().clone().requires_grad_(True)
    rb = A.arm_rate([b], arm, reduce="none")
    yt = base.detach().clone().requires_grad_(True)
    rc = A.arm_rate(yt.transpose(2, 3), arm, reduce="none")   # the view itself goes in
    assert torch.equal(rc, rb)
    rb.sum().backward()
    rc.sum().backward()
    assert torch.equal(yt.grad.transpose(2, 3), b.grad)
    f64 = arm_ref.forward64([y.cpu().numpy()], c["params"])
    assert np.abs(_np(rc) - f64["rate"]).max() <= 1e-4
    # a [C, H, W] tensor is taken as one level too
    assert torch.equal(A.arm_rate(b[0], arm, reduce="none"), rb)


def test_channel_isolation_and_causality_bitwise():
    c = _golden("round")
    arm = _arm(c["layers"], c["params"])
    C, H, W = 3, 8, 9
    y = _random_levels([(C, H, W)], seed=4, outliers=False)[0].to(DEV)
    with torch.no_grad():
        base = A.arm_rate(y, arm, reduce="none").view(C, H, W)
        for ch in range(C):
            z = y.clone()
            z[0, ch] = z[0, ch] * 1.7 + 3.0
            r = A.arm_rate(z, arm, reduce="none").view(C, H, W)
            others = [k for k in range(C) if k != ch]
            assert torch.equal(r[others], base[others])
            assert not torch.equal(r[ch], base[ch])
        for (ch, h, w) in [(1, 3, 4), (0, 0, 0), (2, H - 1, W - 1), (1, 0, W - 1), (0, H - 2, 1)]:
            z = y.clone()
            z[0, ch, h, w] += 0.37
            r = A.arm_rate(z, arm, reduce="none").view(C, H, W)
            later = torch.zeros(C, H, W, dtype=torch.bool, device=DEV)
            later[ch, h, w] = True
            for hh in range(h, min(h + 3, H)):
                for ww in range(max(w - 2, 0), min(w + 3, W)):
                    if hh > h or ww > w:
                        later[ch, hh, ww] = True
            assert torch.equal(r[~later], base[~later])
            assert r[ch, h, w] != base[ch, h, w]
            assert (r[later] != base[later]).sum() >= later.sum() - 1   # every later latent reads it (one may round to the same rate)


def test_single_latent_gradient_support():
    c = _golden("round")
    arm = _arm(c["layers"], c["params"])
    shape = (2, 6, 7)
    levels = _random_levels([shape], seed=6, outliers=False)
    for (ch, h, w) in [(1, 3, 4), (0, 0, 0), (1, 5, 6), (0, 1, 0)]:
        wts = np.zeros(shape, dtype=np.float32)
        wts[ch, h, w] = 1.0
        g = _run(levels, arm, wts.reshape(-1))["g_levels"][0][0]
        support = torch.zeros(shape, dtype=torch.bool, device=DEV)
        support[ch, h, w] = True
        for pos in arm_ref.context_positions(shape, ch, h, w):
            support[pos] = True
        assert (g[~support] == 0).all()
        assert (g[support] != 0).all(), (ch, h, w)


@pytest.mark.parametrize("key", ["round", "kinks"])
def test_floor_latents_contribute_exactly_zero(key):
    c = _golden(key)
    arm = _arm(c["layers"], c["params"])
    base = _run(c["levels"], arm, c["w"])
    floored = np.flatnonzero(c["rate"] == 16.0)
    assert len(floored) >= 30 and torch.equal(torch.from_numpy(floored).to(DEV), torch.nonzero(base["rate"] == 16.0).view(-1))
    for i in floored:
        w = c["w"].copy()
        w[i] = 0.0
        other = _run(c["levels"], arm, w)
        for a, b in zip(base["g_levels"] + base["g_params"], other["g_levels"] + other["g_params"]):
            assert torch.equal(a, b), int(i)
    # and a case of floored latents alone has no gradient at all
    w = np.where(c["rate"] == 16.0, c["w"], 0.0).astype(np.float32)
    for g in (lambda r: r["g_levels"] + r["g_params"])(_run(c["levels"], arm, w)):
        assert (g == 0).all()


def test_clamped_log_scale_has_zero_gradient():
    c = _golden("kinks")
    arm = _arm(c["layers"], c["params"])
    f64 = arm_ref.forward64(c["levels"], c["params"])
    off_floor = f64["p0"] >= 2 * arm_ref.P_FLOOR
    below, above = f64["ls"] < arm_ref.LS_MIN, f64["ls"] > arm_ref.LS_MAX
    assert (below & off_floor).sum() >= 10 and (above & off_floor).sum() >= 5
    for clamped in (below, above):
        w = np.where(clamped & off_floor, c["w"], 0.0).astype(np.float32)
        g = _run(c["levels"], arm, w)["g_params"]
        # the output layer's second row is log_scale's: nothing reaches it
        assert (g[-2][1] == 0).all() and g[-1][1] == 0
        if clamped is below:        # mu's row does get a gradient (at the scale of 1e-3 above the clamp exp(-|x - mu| / s) underflows)
            assert (g[-2][0] != 0).any() and g[-1][0] != 0
    # inside the clamp the same row does get one
    inside = ~below & ~above & off_floor
    g = _run(c["levels"], arm, np.where(inside, c["w"], 0.0).astype(np.float32))["g_params"]
    assert g[-1][1] != 0


def test_reductions_modes_and_repeatability():
    c = _golden("noise")
    arm = _arm(c["layers"], c["params"])
    levels = c["levels"] + [y.numpy() for y in _random_levels([(5, 40, 41)], seed=8)]     # more than one workgroup
    runs = [_run(levels, arm, None, reduce="sum", return_params=False) for _ in range(2)]
    none = [_run(levels, arm, None, reduce="none") for _ in range(2)]
    for r in (runs, none):
        assert torch.equal(r[0]["rate"], r[1]["rate"])
        for a, b in zip(r[0]["g_levels"] + r[0]["g_params"], r[1]["g_levels"] + r[1]["g_params"]):
            assert torch.equal(a, b)
    for name in ("mu", "scale"):
        for a, b in zip(none[0][name], none[1][name]):
            assert torch.equal(a, b)
    total = runs[0]["rate"]
    assert total.shape == () and total.dtype == torch.float32
    # the sum is the per-latent rates added in double in a fixed order and rounded once
    want = none[0]["rate"].double().sum()
    assert abs(float(total) - float(want)) <= float(torch.finfo(torch.float32).eps) * float(want)
    # a scalar upstream gradient of 1 and a vector of ones are the same backward
    for a, b in zip(runs[0]["g_levels"] + runs[0]["g_params"], none[0]["g_levels"] + none[0]["g_params"]):
        assert torch.equal(a, b)
    # across streams
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        again = _run(levels, arm, None, reduce="sum", return_params=False)
    torch.cuda.synchronize()
    assert torch.equal(again["rate"], total)
    for a, b in zip(again["g_levels"] + again["g_params"], runs[0]["g_levels"] + runs[0]["g_params"]):
        assert torch.equal(a, b)


def test_no_grad_saves_nothing_and_partial_gradients():
    c = _golden("round")
    arm = _arm(c["layers"], c["params"])
    leaves = [torch.as_tensor(y).to(DEV).requires_grad_(True) for y in c["levels"]]
    with torch.no_grad():
        total, mu, scale = A.arm_rate(leaves, arm, return_params=True)
    assert total.grad_fn is None and not total.requires_grad and not mu[0].requires_grad
    full = _run(c["levels"], arm, c["w"])
    # only the latents, only the parameters, only one level
    for p in arm.parameters():
        p.requires_grad_(False)
    only_y = [torch.as_tensor(y).to(DEV).requires_grad_(True) for y in c["levels"]]
    (A.arm_rate(only_y, arm, reduce="none") * torch.as_tensor(c["w"]).to(DEV)).sum().backward()
    for a, b in zip(only_y, full["g_levels"]):
        assert torch.equal(a.grad, b)
    for p in arm.parameters():
        p.requires_grad_(True)
        p.grad = None
    plain = [torch.as_tensor(y).to(DEV) for y in c["levels"]]
    plain[1].requires_grad_(True)
    out, mu, scale = A.arm_rate(plain, arm, reduce="none", return_params=True)
    assert not mu[0].requires_grad and not scale[0].requires_grad
    (out * torch.as_tensor(c["w"]).to(DEV)).sum().backward()
    assert torch.equal(plain[1].grad, full["g_levels"][1]) and plain[0].grad is None
    for p, g in zip(arm.parameters(), full["g_params"]):
        assert torch.equal(p.grad, g)


def test_no_host_sync():
    c = _golden("noise")
    arm = _arm(c["layers"], c["params"])
    wide = _golden("wide")
    arm_w = _arm(wide["layers"], wide["params"])
    levels = [torch.as_tensor(y).to(DEV) for y in c["levels"]]
    w = torch.as_tensor(c["w"]).to(DEV)
    A.arm_rate(levels, arm)                                    # warm: the library's context is created once
    leaves = [y.clone().requires_grad_(True) for y in levels]
    leaves_w = [y.clone().requires_grad_(True) for y in levels]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(8, device=DEV).nonzero()                # the mode is live on this build
        total = A.arm_rate(leaves, arm)
        total.backward()
        rate, mu, scale = A.arm_rate(leaves_w, arm_w, reduce="none", return_params=True)
        (rate * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert leaves[0].grad is not None and leaves_w[1].grad is not None and arm_w.mlp[0].w.grad is not None


def test_errors():
    c = _golden("round")
    arm = _arm(c["layers"], c["params"])
    y = torch.zeros(1, 2, 4, 5, device=DEV)
    with pytest.raises(TypeError):
        A.arm_rate(y.double(), arm)
    with pytest.raises(RuntimeError):
        A.arm_rate(y.cpu(), arm)
    with pytest.raises(ValueError):
        A.arm_rate(y, arm, reduce="mean")
    with pytest.raises(ValueError):
        A.arm_rate(y[0, 0], arm)                               # [H, W]
    with pytest.raises(ValueError):
        A.arm_rate(torch.zeros(2, 2, 4, 5, device=DEV), arm)   # a batch
    for input_ft, layers in [(12, []), (12, [16] * 9), (12, [33]), (24, [16, 16])]:
        with pytest.raises(ValueError):
            A.arm_rate(y, A.ArmMLP(input_ft, layers).to(DEV))
    with pytest.raises(NotImplementedError):
        A.ArmMLP(12, [16, 16], fpfm=8)
    arm.FPFM = 8
    with pytest.raises(NotImplementedError):
        A.arm_rate(y, arm)
    arm.FPFM = 0
    with pytest.raises(TypeError):
        A.arm_rate(y, torch.nn.Linear(12, 2).to(DEV))
    # the smallest and the largest networks the generic kernel takes
    for layers in ([1], [32] * 8):
        net = A.ArmMLP(12, layers).to(DEV)
        yy = y.clone().requires_grad_(True)
        A.arm_rate(yy, net).backward()
        assert torch.isfinite(yy.grad).all() and all(torch.isfinite(p.grad).all() for p in net.parameters())


def test_it_trains():
    """Adam on the ARM's parameters: the total bits of the `round` latents go down (the float32 torch formula on a CPU, from three seeds of
    the same initialisation, reaches 0.88 to 0.89 of the first step's bits in these 60 steps; the latents on the floor cannot move)."""
    torch.manual_seed(0)
    c = _golden("round")
    arm = A.ArmMLP(12, c["layers"]).to(DEV)
    levels = [torch.as_tensor(y).to(DEV) for y in c["levels"]]
    opt = torch.optim.Adam(arm.parameters(), lr=0.01)
    bits = []
    for _ in range(60):
        total = A.arm_rate(levels, arm)
        opt.zero_grad()
        total.backward()
        opt.step()
        bits.append(float(total.detach()))
    assert bits[-1] < 0.95 * bits[0], bits[::10]
