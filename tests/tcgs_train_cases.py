"""Inputs of the TC-GS training-branch pin, shared by the generator (tests/golden/make_tcgs_train_golden.py, which feeds them to the
reference's own gaussian_renderer) and the tests (tests/test_tcgs_train_ref_cpu.py, tests/test_gpu_tcgs_train.py).  Everything is drawn from
gauspcc_amd.synth.CounterRNG, so the same bytes come out on every machine; the fixture stores inputs_sha256 of what `inputs()` returns,
weights and recorded draws included, so drift in a builder is caught.

One model: 120 anchors of which about 80 % are visible, feat_dim 50, 10 offsets, K = 4 neighbours.  `triplane` is a stand-in (StandInPlane):
sin(knnanchor.reshape(N, 12) @ A + b), 16 features, in any dtype, drawing nothing; it returns (features, None, None) in training up to step
15000 and past that (features, planes[:, :1], 0.5 planes + 0.1) -- a reconstruction whose L1 distance to `planes` is not zero -- and the
features alone in evaluation.  `mlp_triplane` is Linear(16 + 3, 100) - ReLU - Linear(100, 175); a row of its output is TC-GS's [mean | scale |
mean_scaling | scale_scaling | mean_offsets | scale_offsets | 3 adj].  get_mask and get_mask_anchor are properties, the latter a bool (N,);
anchors 3 and 40 are fully masked and anchor 3 is among the chosen.  knnanchor[i] holds anchors i, i + 7, i + 14, i + 21 (mod N): distinct
neighbours.  The opacity MLP's last bias is +-1.5 over small weights, so that no candidate's opacity comes near the keep test's zero (the
generator asserts the margin on what the reference computed).

Validation quantises with Q = Q0 (1 + tanh(adj)), Q0 = (1, 0.001, 0.3): the builder evaluates its own stand-in context in float64 and float32
and re-draws every attribute element with |frac(x / Q) - 0.5| below max(1e-3, 10 x the float32-vs-float64 difference in x / Q)
(cat_train_cases.py's rule), so no element can round differently in the two precisions and none is excluded (`rounding_violations`).

Recorded draws per run, in the branch's order (`draws(a, tag)`): feat / scaling / offsets noise of the gathered anchors, then the rand_like
over them (8 entries at 0.01, 8 at 0.10, the rest >= 0.2).  Steps <= 3000 draw nothing, steps in (3000, 10000] the first three.
"""
import types

import numpy as np

from tests import branch_common
from tests.attr_pin_cases import NG_TOL, _sequential, sha256_of   # noqa: F401  (re-exported for the generator and the tests)
from tests.hacpp_train_cases import _Streams

N, F, K_OFF, KNN, TRI_DIM, HIDDEN = 120, 50, 10, 4, 16, 100
PLANE_SHAPE = (3, 4, 4, 4)
Q0 = (1.0, 0.001, 0.3)
SEED = 51
# (tag, is_training, step, with the visible mask, decoded)
RUNS = (("train2000", True, 2000, False, False), ("train5000", True, 5000, False, False), ("train10000", True, 10000, False, False),
        ("train12000", True, 12000, False, False), ("train15000", True, 15000, False, False), ("train20000", True, 20000, False, False),
        ("train12000_vis", True, 12000, True, False), ("val", False, 0, True, False), ("decoded", False, 0, True, True))
TRAIN_STEPS = (2000, 5000, 10000, 12000, 15000, 20000)
MUTATIONS = ("q_offsets02", "threshold005", "no_mask_anchor", "drop_offset_mask", "repeat_form", "no_rate_factor")
RATE_RTOL = 1e-5
OPACITY_MARGIN = 1e-4
OUTPUTS = ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity")
RATES = ("bit_per_param", "bit_per_feat_param", "bit_per_scaling_param", "bit_per_offsets_param", "lae")
OUT_TOL = dict(NG_TOL, neural_opacity=2e-5)
WIDTH = 2 * F + 12 + 6 * K_OFF + 3


def run(tag):
    return next(r for r in RUNS if r[0] == tag)


def _ctx_np(a, dtype):
    """the stand-in context of every anchor in the repeat form, in numpy, in `dtype`"""
    t = lambda k: a[k].astype(dtype)      # noqa: E731
    anchor = t("anchor")
    f = np.sin(np.tile(anchor, (1, KNN)) @ t("tri_A") + t("tri_b"))
    rows = np.concatenate([f, anchor], axis=1)
    return np.maximum(rows @ t("tri_w1").T + t("tri_b1"), 0) @ t("tri_w2").T + t("tri_b2")


def _ratios(a):
    out = []
    adj64, adj32 = _ctx_np(a, np.float64)[:, -3:], _ctx_np(a, np.float32)[:, -3:]
    for j, key in enumerate(("feat", "scaling", "offset")):
        x = a[key].reshape(a[key].shape[0], -1)
        q64 = Q0[j] * (1 + np.tanh(adj64[:, j:j + 1]))
        q32 = np.float32(Q0[j]) * (np.float32(1) + np.tanh(adj32[:, j:j + 1]))
        r64 = x.astype(np.float64) / q64
        out.append((r64, np.abs((x / q32).astype(np.float64) - r64)))
    return out


def _borderline(a):
    return [np.abs(r - np.floor(r) - 0.5) < np.maximum(1e-3, 10 * d) for r, d in _ratios(a)]


def rounding_violations(a):
    """attribute elements that could round differently in float32 and float64: the cap is zero"""
    return sum(int(b.sum()) for b in _borderline(a))


def inputs():
    """{name: numpy array}: the tensors and weights (float32), the visible mask (bool), the camera centre; per run its recorded draws
    ('draw/<tag>/<i>')"""
    a = {}
    s = _Streams(SEED)
    a["cam"] = np.array([0.3, -4.0, 1.1], np.float32)
    a["anchor"] = s.uniform((N, 3), -2, 2).astype(np.float32)
    a["bound_max"], a["bound_min"] = np.array([2.5, 2.4, 2.6], np.float32), np.array([-2.4, -2.6, -2.5], np.float32)
    a["mask"] = (s.uniform((N, K_OFF, 1)) > 0.35).astype(np.float32)
    a["mask"][3] = 0.0
    a["mask"][40] = 0.0
    a["mask"][5, 0] = 1.0
    vis = s.uniform((N,)) > 0.2
    vis[1], vis[2], vis[3], vis[5], vis[40] = False, True, True, True, True
    a["vis"] = vis
    for mlp, cin, cout in (("opacity", F + 4, K_OFF), ("cov", F + 4, 7 * K_OFF), ("color", F + 4, 3 * K_OFF)):
        a[f"{mlp}_w1"], a[f"{mlp}_b1"], a[f"{mlp}_w2"], a[f"{mlp}_b2"] = s.weights((F, cin), 16), s.weights(F, 16), s.weights((cout, F), 16), s.weights(cout, 16)
    a["opacity_w2"] = (a["opacity_w2"] / np.float32(8)).astype(np.float32)
    a["opacity_b2"] = np.array([1.5 if k % 3 == 0 else -1.5 for k in range(K_OFF)], np.float32)
    a["tri_A"], a["tri_b"] = s.weights((3 * KNN, TRI_DIM), 8), s.weights(TRI_DIM, 4)
    a["tri_planes"] = (s.uniform(PLANE_SHAPE, -1, 1) * 0.5).astype(np.float32)
    a["tri_w1"], a["tri_b1"] = s.weights((HIDDEN, TRI_DIM + 3), 16), s.weights(HIDDEN, 16)
    a["tri_w2"], a["tri_b2"] = s.weights((WIDTH, HIDDEN), 32), s.weights(WIDTH, 16)
    # scale heads around 0.5 .. 2 x the step, as a trained context model's: positive by bias; the scaling mean head near the scalings
    for lo, hi, bias in ((F, 2 * F, 1.0), (2 * F, 2 * F + 6, 0.08), (2 * F + 6, 2 * F + 12, 0.05), (2 * F + 12 + 3 * K_OFF, 2 * F + 12 + 6 * K_OFF, 0.3)):
        a["tri_w2"][lo:hi] *= np.float32(bias / 8)
        a["tri_b2"][lo:hi] = np.float32(bias)
    fresh = lambda: (s.normal((N, F), 0.8).astype(np.float32), np.exp(s.normal((N, 6), 0.4) - 2.5).astype(np.float32),   # noqa: E731
                     s.normal((N, K_OFF, 3), 0.3).astype(np.float32))
    a["feat"], a["scaling"], a["offset"] = fresh()
    for _ in range(200):
        bad = _borderline(a)
        if not any(b.any() for b in bad):
            break
        for key, b, new in zip(("feat", "scaling", "offset"), bad, fresh()):
            b = b.reshape(a[key].shape)
            a[key][b] = new[b]
    else:
        raise AssertionError("could not clear the borderline roundings")
    for tag, train, step, with_vis, _ in RUNS:
        if train:
            s = _Streams(SEED * 1000 + step % 997 + len(tag))
            for i, d in enumerate(_draws(s, vis if with_vis else np.ones(N, bool), step)):
                a[f"draw/{tag}/{i}"] = d
    return a


def _draws(s, vis, step):
    if step <= 3000:
        return []
    n = int(vis.sum())
    u = lambda *shape: s.uniform(shape, -0.5, 0.5).astype(np.float32)   # noqa: E731
    out = [u(n, F), u(n, 6), u(n, K_OFF, 3)]
    if step > 10000:
        r = np.minimum((0.2 + 0.8 * s.uniform((n,))).astype(np.float32), np.float32(0.99999994))      # values of [0, 1), as rand_like's
        rows = np.cumsum(vis) - 1                      # anchor -> gathered row
        low = [int(rows[i]) for i in (3, 5)] + list(range(10, 22, 2))
        mid = [int(rows[40])] + list(range(31, 45, 2))
        r[np.array(mid) % n] = np.float32(0.10)
        r[np.array(low) % n] = np.float32(0.01)
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
    return 0 if not training or step <= 3000 else 4 if step > 10000 else 3


def expected_hooks(step, training=True):
    """the model's step hooks a run fires, in order"""
    return [] if not training else ["updatebbox"] if step == 10000 else [("init_knn_indice", KNN)] if step == 15000 else []


def stand_in_plane(torch, A, b, planes):
    """The stand-in for utils/triplane.py's Triplane: a plain torch module with its call signature and return convention."""
    nn = torch.nn

    class StandInPlane(nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("A", A)
            self.register_buffer("b", b)
            self.planes = nn.Parameter(planes.clone())
            self.autoencoder = types.SimpleNamespace(encoder=object())
            self.calls = []

        def forward(self, knnanchor, max_coords, min_coords, is_training=0, step=0):
            assert knnanchor.dim() == 3 and knnanchor.shape[1:] == (KNN, 3) and max_coords.shape == (3,) and min_coords.shape == (3,)
            self.calls.append((bool(is_training), step))
            f = torch.sin(knnanchor.reshape(knnanchor.shape[0], -1) @ self.A + self.b)
            if is_training and step > 15000:
                return f, self.planes[:, :1], self.planes * 0.5 + 0.1
            if is_training:
                return f, None, None
            return f

    return StandInPlane()


def model(a, torch, device="cpu", dtype=None, decoded=False):
    """(pc, cam, visible_mask): an object with everything TC-GS's generate_neural_gaussians touches, minus the rate module
    pc.entropy_gaussian, which the caller attaches: the reference's, the library's or none (the restatement has its own)."""
    dtype = dtype or torch.float32
    nn = torch.nn
    t = lambda x: torch.tensor(np.asarray(x)).to(device=device, dtype=dtype)   # noqa: E731

    class Model:
        @property
        def get_mask(self):
            return self._mask01

        @property
        def get_mask_anchor(self):
            with torch.no_grad():
                return torch.sum(self._mask01, dim=1)[:, 0] > 0

        def updatebbox(self):
            self.hooks.append("updatebbox")

        def init_knn_indice(self, k):
            self.hooks.append(("init_knn_indice", k))

    pc = Model()
    pc.feat_dim, pc.n_offsets, pc.decoded_version, pc.use_feat_bank, pc.appearance_dim = F, K_OFF, bool(decoded), False, 0
    pc.add_color_dist = pc.add_cov_dist = pc.add_opacity_dist = True
    pc.hooks = []
    pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc._mask01 = t(a["anchor"]), t(a["feat"]), t(a["offset"]), t(a["scaling"]), t(a["mask"])
    pc._anchor = pc.get_anchor
    pc.x_bound_max, pc.x_bound_min = t(a["bound_max"]), t(a["bound_min"])
    idx = (np.arange(N)[:, None] + 7 * np.arange(KNN)[None, :]) % N
    pc.knnanchor = pc.get_anchor[torch.tensor(idx, device=device)]
    pc.rotation_activation = torch.nn.functional.normalize
    pc.get_opacity_mlp = _sequential(torch, a, "opacity", nn.Tanh(), device, dtype)
    pc.get_cov_mlp = _sequential(torch, a, "cov", None, device, dtype)
    pc.get_color_mlp = _sequential(torch, a, "color", nn.Sigmoid(), device, dtype)
    pc.get_tri_mlp = _sequential(torch, a, "tri", None, device, dtype)
    pc.triplane = stand_in_plane(torch, t(a["tri_A"]), t(a["tri_b"]), t(a["tri_planes"])).to(device)
    cam = types.SimpleNamespace(camera_center=t(a["cam"]), uid=0)
    return pc, cam, torch.tensor(np.asarray(a["vis"]), device=device)


# ---- tests/golden/tcgs_train.npz (tests/golden/make_tcgs_train_golden.py) -------------------------------------------------------------

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
    """asserts a 12-tuple (training) or a 6-tuple against the stored outputs of a run within the stored tolerances; prints every figure first"""
    _, train, step, _, _ = run(tag)
    outs, keep, tol = stored(g, tag)
    assert len(res) == (12 if train else 6)
    if train:
        assert np.array_equal(res[6].cpu().numpy(), keep)
    for k, v in zip(OUTPUTS[:6 if train else 5], res):
        v = v.detach().double().cpu().numpy()
        assert v.shape == outs[k].shape, (k, v.shape, outs[k].shape)
        err = float(np.abs(v - outs[k]).max())
        print(f"{tag} {k}: {err:.3e} (tolerance {tol[k]:.3e})")
        assert err <= tol[k], (tag, k, err, tol[k])
    for k, v in (zip(RATES, res[7:]) if train else ()):
        if k not in outs:
            assert v is None, (tag, k, v)
            continue
        rel = abs(float(v) - float(outs[k])) / abs(float(outs[k]))
        print(f"{tag} {k}: {rel:.3e} relative (tolerance {tol[k]:.3e})")
        assert rel <= tol[k] + 2.0 ** -23, (tag, k, rel, tol[k])      # the stored value is a float32
