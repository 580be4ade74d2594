"""Inputs of the CAT-3DGS training-branch pin, shared by the generator (tests/golden/make_cat_train_golden.py, which feeds them to the
reference's own gaussian_renderer) and the tests (tests/test_cat_train_ref_cpu.py, tests/test_gpu_cat_train.py).  Everything is drawn from
gauspcc_amd.synth.CounterRNG, so the same bytes come out on every machine; the fixture stores inputs_sha256 of what `inputs()` returns,
weights and recorded draws included, so drift in a builder is caught.

Two models.  "main": 120 anchors of which about 80 % are visible, feat_dim 50, 10 offsets, feat groups [12, 12, 13, 13], the channel-context
MLPs for scaling and offsets on.  "small": 40 anchors, groups [25, 25], both flags off.  `feature_net` is a stand-in: sin(anchor @ A + b)
through Linear(16, 100) - ReLU - Linear(100, 175), plus the scalar feat_rate = rate + 1e-3 * sum of the sin features; it runs in any dtype
and draws nothing.  A row of its output is CAT-3DGS's [scales | means | mean_scaling | scale_scaling | mean_offsets | scale_offsets | 3 adj].
The channel-context MLPs are Linear(dep, 100) - ReLU - Linear(100, 2 ch) with small last layers.  get_mask / get_mask_anchor are methods
that take `weighted_mask` (here a {0, 1} tensor that switches offsets off); anchor 3 is fully masked and is among the chosen; under the
weighted mask anchor 7 is too.  The opacity MLP's last bias is +-1.5 over small weights, so that no candidate's opacity comes near the keep
test's zero (the generator asserts the margin on what the reference computed).

Validation quantises with Q = Q0 (1.1 + tanh(adj)): the builder evaluates its own stand-in context in float64 and float32 and re-draws
every attribute element with |frac(x / Q) - 0.5| below max(1e-3, 10 x the float32-vs-float64 difference in x / Q) (make_attr_pins.py's
rule), so no element can round differently in the two precisions and none is excluded from a comparison (`rounding_violations`).

Recorded draws per run, in the branch's order (`draws(a, tag)`): feat / scaling / offsets noise of the visible anchors, then the rand_like
over the VISIBLE anchors (16 entries at 0.01, the rest >= 0.06).  Steps <= 3000 draw nothing, steps in (3000, 10000] the first three.
"""
import types

import numpy as np

from tests import branch_common
from tests.attr_pin_cases import NG_TOL, _sequential, sha256_of   # noqa: F401  (re-exported for the generator and the tests)
from tests.hacpp_train_cases import _Streams

CTX_DIM, HIDDEN = 16, 100
Q0 = (1.0, 0.001, 0.2)
BASE = 1.1
MODELS = dict(main=dict(N=120, F=50, K=10, groups=(12, 12, 13, 13), on=True, seed=31),
              small=dict(N=40, F=50, K=10, groups=(25, 25), on=False, seed=32))
# (tag, model, is_training, step, weighted mask, decoded)
RUNS = (("train2000", "main", True, 2000, False, False), ("train5000", "main", True, 5000, False, False),
        ("train10000", "main", True, 10000, False, False), ("train12000", "main", True, 12000, False, False),
        ("train-1", "main", True, -1, False, False), ("train12000_wmask", "main", True, 12000, True, False),
        ("small12000", "small", True, 12000, False, False),
        ("val5000", "main", False, 5000, False, False), ("val12000", "main", False, 12000, False, False),
        ("val-1", "main", False, -1, False, False), ("decoded", "main", False, 0, False, True))
TRAIN_STEPS, VAL_STEPS = (2000, 5000, 10000, 12000, -1), (5000, 12000, -1)
N_CHOSEN = 16
RATE_RTOL = 1e-5
OPACITY_MARGIN = 1e-4
OUTPUTS = ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity")
RATES = ("bit_per_param", "bit_per_feats_param", "bit_per_scaling_param", "bit_per_offsets_param", "feat_rate")
OUT_TOL = dict(NG_TOL, neural_opacity=2e-5)


def run(tag):
    return next(r for r in RUNS if r[0] == tag)


def width(F, K):
    return 2 * F + 12 + 6 * K + 3


def rate_branch(step):
    return step > 10000 or step == -1


def _ctx_np(a, p, dtype):
    """the stand-in feature_net's context in numpy, in `dtype`"""
    t = lambda k: a[p + k].astype(dtype)      # noqa: E731
    f = np.sin(t("anchor") @ t("interp_A") + t("interp_b"))
    return np.maximum(f @ t("fnet_w1").T + t("fnet_b1"), 0) @ t("fnet_w2").T + t("fnet_b2")


def _ratios(a, p):
    """per attribute: (x / Q in float64, |its float32 value - it|), from the builder's own context"""
    out = []
    adj64, adj32 = _ctx_np(a, p, np.float64)[:, -3:], _ctx_np(a, p, np.float32)[:, -3:]
    for j, key in enumerate(("feat", "scaling", "offset")):
        x = a[p + key].reshape(a[p + key].shape[0], -1)
        q64 = Q0[j] * (BASE + np.tanh(adj64[:, j:j + 1]))
        q32 = np.float32(Q0[j]) * (np.float32(BASE) + np.tanh(adj32[:, j:j + 1]))
        r64 = x.astype(np.float64) / q64
        out.append((r64, np.abs((x / q32).astype(np.float64) - r64)))
    return out


def _borderline(a, p):
    return [np.abs(r - np.floor(r) - 0.5) < np.maximum(1e-3, 10 * d) for r, d in _ratios(a, p)]


def rounding_violations(a):
    """attribute elements that could round differently in float32 and float64: the cap is zero"""
    return sum(int(b.sum()) for name in MODELS for b in _borderline(a, name + "/"))


def inputs():
    """{name: numpy array}: per model (prefix 'main/', 'small/') the tensors and weights (float32), the visible mask (bool), the weighted mask,
    the camera centre; per run its recorded draws ('draw/<tag>/<i>')"""
    a = {}
    for name, cfg in MODELS.items():
        s, p = _Streams(cfg["seed"]), name + "/"
        N, F, K = cfg["N"], cfg["F"], cfg["K"]
        W = width(F, K)
        a[p + "cam"] = np.array([0.3, -4.0, 1.1], np.float32)
        a[p + "anchor"] = s.uniform((N, 3), -2, 2).astype(np.float32)
        a[p + "mask"] = (s.uniform((N, K, 1)) > 0.35).astype(np.float32)
        a[p + "mask"][3] = 0.0
        a[p + "mask"][5, 0] = 1.0
        w = (s.uniform((N, K, 1)) > 0.25).astype(np.float32)
        w[7] = 0.0
        a[p + "wmask"] = w
        vis = s.uniform((N,)) > 0.2
        vis[1], vis[2], vis[3], vis[5], vis[7] = False, True, True, True, True
        a[p + "vis"] = vis
        for mlp, cin, cout in (("opacity", F + 4, K), ("cov", F + 4, 7 * K), ("color", F + 4, 3 * K)):
            a[p + f"{mlp}_w1"], a[p + f"{mlp}_b1"], a[p + f"{mlp}_w2"], a[p + f"{mlp}_b2"] = s.weights((F, cin), 16), s.weights(F, 16), s.weights((cout, F), 16), s.weights(cout, 16)
        a[p + "opacity_w2"] = (a[p + "opacity_w2"] / np.float32(8)).astype(np.float32)
        a[p + "opacity_b2"] = np.array([1.5 if k % 3 == 0 else -1.5 for k in range(K)], np.float32)      # a third of the candidates kept: a small fixture
        a[p + "interp_A"], a[p + "interp_b"] = s.weights((3, CTX_DIM), 4), s.weights(CTX_DIM, 4)
        a[p + "fnet_w1"], a[p + "fnet_b1"] = s.weights((HIDDEN, CTX_DIM), 16), s.weights(HIDDEN, 16)
        a[p + "fnet_w2"], a[p + "fnet_b2"] = s.weights((W, HIDDEN), 32), s.weights(W, 16)
        a[p + "fnet_rate"] = np.array([0.37], np.float32)
        # scale heads around 0.5 .. 2 x the step, as a trained context model's: positive by bias; the scaling mean head near the scalings
        for lo, hi, bias in ((0, F, 1.0), (2 * F, 2 * F + 6, 0.08), (2 * F + 6, 2 * F + 12, 0.05), (2 * F + 12 + 3 * K, 2 * F + 12 + 6 * K, 0.3)):
            a[p + "fnet_w2"][lo:hi] *= np.float32(bias / 8)
            a[p + "fnet_b2"][lo:hi] = np.float32(bias)
        dep, stages = 0, []
        for i, ch in enumerate(cfg["groups"]):
            if i:
                stages.append((f"chcm{i - 1}", dep, ch, 0.2))
            dep += ch
        if cfg["on"]:
            stages += [("chcm_scaling", F, 6, 0.005), ("chcm_offsets", F, 3 * K, 0.03)]
        for mlp, din, ch, gain in stages:
            a[p + f"{mlp}_w1"], a[p + f"{mlp}_b1"] = s.weights((2 * F, din), 32), s.weights(2 * F, 16)
            a[p + f"{mlp}_w2"], a[p + f"{mlp}_b2"] = s.weights((2 * ch, 2 * F), 32) * np.float32(gain), s.weights(2 * ch, 16) * np.float32(gain)
        fresh = lambda: (s.normal((N, F), 0.8).astype(np.float32), np.exp(s.normal((N, 6), 0.4) - 2.5).astype(np.float32),   # noqa: E731
                         s.normal((N, K, 3), 0.3).astype(np.float32))
        a[p + "feat"], a[p + "scaling"], a[p + "offset"] = fresh()
        for _ in range(200):
            bad = _borderline(a, p)
            if not any(b.any() for b in bad):
                break
            for key, b, new in zip(("feat", "scaling", "offset"), bad, fresh()):
                b = b.reshape(a[p + key].shape)
                a[p + key][b] = new[b]
        else:
            raise AssertionError(f"{name}: could not clear the borderline roundings")
    for tag, name, train, step, _, _ in RUNS:
        if train:
            cfg = MODELS[name]
            s = _Streams(cfg["seed"] * 1000 + abs(step) % 997 + len(tag))
            for i, d in enumerate(_draws(s, a[name + "/vis"], cfg, step)):
                a[f"draw/{tag}/{i}"] = d
    return a


def _draws(s, vis, cfg, step):
    if 0 <= step <= 3000:
        return []
    F, K, nvis = cfg["F"], cfg["K"], int(vis.sum())
    u = lambda *shape: s.uniform(shape, -0.5, 0.5).astype(np.float32)   # noqa: E731
    out = [u(nvis, F), u(nvis, 6), u(nvis, K, 3)]
    if rate_branch(step):
        r = np.minimum((0.06 + 0.94 * s.uniform((nvis,))).astype(np.float32), np.float32(0.99999994))      # values of [0, 1), as rand_like's
        rows = np.cumsum(vis) - 1                      # anchor -> visible row
        chosen = [int(rows[i]) for i in (3, 5, 7)] + list(range(10, 10 + 2 * (N_CHOSEN - 3), 2))
        r[np.array(chosen) % nvis] = np.float32(0.01)
        out.append(r)
    return out


def draws(a, tag):
    out, i = [], 0
    while f"draw/{tag}/{i}" in a:
        out.append(a[f"draw/{tag}/{i}"])
        i += 1
    return out


def Replay(a, tag, torch):
    """branch_common.Replay on the recorded draws of a run"""
    return branch_common.Replay(draws(a, tag), torch)


def expected_draws(step, training=True):
    return 0 if not training or 0 <= step <= 3000 else 4 if rate_branch(step) else 3


def model(a, name, torch, device="cpu", dtype=None, decoded=False):
    """(pc, cam, visible_mask, weighted_mask): a SimpleNamespace with everything CAT-3DGS's generate_neural_gaussians touches, minus the
    rate module pc.entropy_gaussian, which the caller attaches: the reference's, the library's or none (the restatement has its own)."""
    dtype = dtype or torch.float32
    nn = torch.nn
    cfg, p = MODELS[name], name + "/"
    F, K = cfg["F"], cfg["K"]
    sub = {k[len(p):]: v for k, v in a.items() if k.startswith(p)}
    t = lambda x: torch.tensor(np.asarray(x)).to(device=device, dtype=dtype)   # noqa: E731
    pc = types.SimpleNamespace(feat_dim=F, n_offsets=K, decoded_version=bool(decoded), use_feat_bank=False, bound_updates=0,
                               chcm_slices_list=list(cfg["groups"]), chcm_for_scaling=cfg["on"], chcm_for_offsets=cfg["on"])
    pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc._mask01 = t(sub["anchor"]), t(sub["feat"]), t(sub["offset"]), t(sub["scaling"]), t(sub["mask"])

    def get_mask(weighted_mask=None):
        return pc._mask01 if weighted_mask is None or pc.decoded_version else pc._mask01 * weighted_mask

    def get_mask_anchor(weighted_mask=None):
        with torch.no_grad():
            return torch.sum(get_mask(weighted_mask), dim=1)[:, 0] > 0

    pc.get_mask, pc.get_mask_anchor = get_mask, get_mask_anchor
    pc.rotation_activation = torch.nn.functional.normalize
    pc.get_opacity_mlp = _sequential(torch, sub, "opacity", nn.Tanh(), device, dtype)
    pc.get_cov_mlp = _sequential(torch, sub, "cov", None, device, dtype)
    pc.get_color_mlp = _sequential(torch, sub, "color", nn.Sigmoid(), device, dtype)

    class FeatureNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("A", t(sub["interp_A"]))
            self.register_buffer("b", t(sub["interp_b"]))
            self.net = _sequential(torch, sub, "fnet", None, device, dtype)
            self.rate = nn.Parameter(t(sub["fnet_rate"]).reshape(()))
            self.calls = []

        def forward(self, anchor, itr=-1):
            self.calls.append(itr)
            f = torch.sin(anchor @ self.A + self.b)
            return self.net(f), self.rate + 1e-3 * f.sum()

    pc.feature_net = FeatureNet()
    pc.get_chcm_mlp_list = nn.ModuleList([_sequential(torch, sub, f"chcm{i}", None, device, dtype) for i in range(len(cfg["groups"]) - 1)])
    pc.get_chcm_mlp_scaling = _sequential(torch, sub, "chcm_scaling", None, device, dtype) if cfg["on"] else None
    pc.get_chcm_mlp_offsets = _sequential(torch, sub, "chcm_offsets", None, device, dtype) if cfg["on"] else None

    def update_anchor_bound():
        pc.bound_updates += 1
    pc.update_anchor_bound = update_anchor_bound
    cam = types.SimpleNamespace(camera_center=t(sub["cam"]))
    return pc, cam, torch.tensor(np.asarray(sub["vis"]), device=device), t(sub["wmask"])


# ---- tests/golden/cat_train.npz (tests/golden/make_cat_train_golden.py) ---------------------------------------------------------------

def stored(g, tag):
    """(outputs {name: array}, keep mask or None, {name: tolerance}) of a run"""
    pre = tag + "/"
    table = g[pre + "out"]
    outs, at = {}, 0
    for k, w in zip(OUTPUTS[:5], (3, 3, 1, 3, 4)):
        outs[k] = table[:, at:at + w]
        at += w
    keep = None
    if pre + "keep" in g:
        outs["neural_opacity"] = g[pre + "neural_opacity"]
        keep = np.unpackbits(g[pre + "keep"])[:int(g[pre + "keep_len"])].astype(bool)
    tol = dict(zip((str(n) for n in g[pre + "names"]), g[pre + "tol"]))
    outs.update(zip((str(n) for n in g[pre + "rate_names"]), g[pre + "rates"]))
    return outs, keep, tol


def compare(res, g, tag):
    """asserts a 12-tuple (training) or a 7-tuple against the stored outputs of a run within the stored tolerances; prints every figure first"""
    _, _, train, step, _, _ = run(tag)
    outs, keep, tol = stored(g, tag)
    assert len(res) == (12 if train else 7)
    if train:
        assert np.array_equal(res[6].cpu().numpy(), keep)
    for k, v in zip(OUTPUTS[:6 if train else 5], res):
        v = v.detach().double().cpu().numpy()
        assert v.shape == outs[k].shape, (k, v.shape, outs[k].shape)
        err = float(np.abs(v - outs[k]).max())
        print(f"{tag} {k}: {err:.3e} (tolerance {tol[k]:.3e})")
        assert err <= tol[k], (tag, k, err, tol[k])
    rates = dict(zip(RATES, res[7:])) if train else dict(feat_rate=res[6])
    for k, v in rates.items():
        if k not in outs:
            assert v is None or (k == "feat_rate" and not isinstance(v, type(res[0])) and v == 0), (tag, k, v)
            continue
        rel = abs(float(v) - float(outs[k])) / abs(float(outs[k]))
        print(f"{tag} {k}: {rel:.3e} relative (tolerance {tol[k]:.3e})")
        assert rel <= tol[k] + 2.0 ** -23, (tag, k, rel, tol[k])      # the stored value is a float32
