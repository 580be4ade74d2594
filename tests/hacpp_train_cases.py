"""Inputs of the HAC++ training-branch pin, shared by the generator (tests/golden/make_hacpp_train_golden.py, which feeds them to the
reference's own gaussian_renderer) and the tests (tests/test_hacpp_train_ref_cpu.py, tests/test_gpu_hacpp_train.py).  Everything is drawn
from gauspcc_amd.synth.CounterRNG, so the same bytes come out on every machine; the fixture stores inputs_sha256 of what `inputs()` returns,
weights and recorded draws included, so drift in a builder is caught.

The model is HAC++-shaped: feat_dim 50, 10 offsets, 120 anchors of which about 80 % are visible; `mlp_grid` is Linear(16, 100) - ReLU -
Linear(100, 225); the channel-context MLP has Channel_CTX_fea's five MLP_d{c}: Linear(150 + 10 c, 40) - LeakyReLU - Linear(40, 30).
calc_interp_feat is a stand-in, sin(anchor @ A + b): a smooth function of the positions that needs no hash grid and runs in any dtype.
The opacity MLP's last bias is +-1.5 over small weights, so that no candidate's opacity comes near the keep test's zero (the generator asserts
the margin on what the reference computed).  Anchor 3 is fully masked (mask_anchor == 0) and is among the chosen.

Recorded draws, per step, in the branch's order (`draws(step)`): feat / scaling / offsets noise of the visible anchors, the rand_like over
all anchors (20 entries at 0.01, the rest >= 0.06: 20 chosen anchors), feat / scaling / offsets noise of the chosen.  Steps <= 3000 draw
nothing, steps in (3000, 10000] the first three.
"""
import types

import numpy as np

from gauspcc_amd.synth import CounterRNG
from tests import branch_common
from tests.attr_pin_cases import NG_TOL, _sequential, sha256_of   # noqa: F401  (NG_TOL: re-exported for the generator and the tests)

F, K, N, CTX_DIM, HIDDEN = 50, 10, 120, 16, 100
WIDTH = 3 * F + 12 + 6 * K + 3            # 225
STEPS = (2000, 5000, 10000, 12000)
N_CHOSEN = 20
RATE_RTOL = 1e-5                          # tests/test_gpu_ng_train.py::test_generate_training_matches_reference_branch
OPACITY_MARGIN = 1e-4                     # the same test's margin
OUTPUTS = ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity")
RATES = ("bit_per_param", "bit_per_feat_param", "bit_per_scaling_param", "bit_per_offsets_param")
OUT_TOL = dict(NG_TOL, neural_opacity=2e-5)
SEED = 20


class _Streams:
    def __init__(self, seed):
        self.rng, self.next = CounterRNG(seed), 1

    def uniform(self, shape, lo=0.0, hi=1.0):
        self.next += 1
        return (self.rng.uniform(self.next, int(np.prod(shape))) * (hi - lo) + lo).reshape(shape)

    def normal(self, shape, scale=1.0):
        self.next += 3          # CounterRNG.normal reads the streams 2 s + 1 and 2 s + 2
        return (self.rng.normal(self.next * 64, int(np.prod(shape))) * scale).reshape(shape)

    def weights(self, shape, unit):
        """multiples of 1 / unit in [-8 / unit, 8 / unit]"""
        return (np.floor(self.uniform(shape) * 17) - 8).astype(np.float32) / np.float32(unit)


def inputs():
    """{name: numpy array}: model tensors and weights (float32), the visible mask (bool), the camera centre"""
    s = _Streams(SEED)
    a = dict(cam=np.array([0.3, -4.0, 1.1], np.float32))
    a["anchor"] = s.uniform((N, 3), -2, 2).astype(np.float32)
    a["feat"] = s.normal((N, F), 0.8).astype(np.float32)
    a["offset"] = s.normal((N, K, 3), 0.3).astype(np.float32)
    a["scaling"] = np.exp(s.normal((N, 6), 0.4) - 2.5).astype(np.float32)
    a["mask"] = (s.uniform((N, K, 1)) > 0.35).astype(np.float32)
    a["mask"][3] = 0.0
    vis = s.uniform((N,)) > 0.2
    vis[1], vis[2], vis[3] = False, True, True
    a["vis"] = vis
    for name, cin, cout in (("opacity", F + 4, K), ("cov", F + 4, 7 * K), ("color", F + 4, 3 * K)):
        a[f"{name}_w1"], a[f"{name}_b1"], a[f"{name}_w2"], a[f"{name}_b2"] = s.weights((F, cin), 16), s.weights(F, 16), s.weights((cout, F), 16), s.weights(cout, 16)
    a["opacity_w2"] = (a["opacity_w2"] / np.float32(8)).astype(np.float32)
    a["opacity_b2"] = np.array([1.5, -1.5] * (K // 2), np.float32)
    a["interp_A"], a["interp_b"] = s.weights((3, CTX_DIM), 4), s.weights(CTX_DIM, 4)
    a["grid_w1"], a["grid_b1"] = s.weights((HIDDEN, CTX_DIM), 16), s.weights(HIDDEN, 16)
    a["grid_w2"], a["grid_b2"] = s.weights((WIDTH, HIDDEN), 32), s.weights(WIDTH, 16)
    # the two scale heads end up around 0.5 .. 2 x the step, as a trained context model's do: softplus-free, so keep them positive by bias
    # (and the scaling mean head near the scalings themselves: their step is 1e-3)
    for lo, hi, bias in ((F, 2 * F, 1.0), (3 * F, 3 * F + 6, 0.08), (3 * F + 6, 3 * F + 12, 0.05), (3 * F + 12 + 3 * K, 3 * F + 12 + 6 * K, 0.3)):
        a["grid_w2"][lo:hi] *= np.float32(bias / 8)
        a["grid_b2"][lo:hi] = np.float32(bias)
    for c in range(5):
        a[f"deform{c}_w1"], a[f"deform{c}_b1"] = s.weights((40, 3 * F + 10 * c), 32), s.weights(40, 16)
        a[f"deform{c}_w2"], a[f"deform{c}_b2"] = s.weights((30, 40), 32), s.weights(30, 16)
        a[f"deform{c}_b2"][10:20] += np.float32(1.0)          # the second component's scales: positive
    for step in STEPS:
        for i, d in enumerate(_draws(s, int(vis.sum()), step)):
            a[f"draw_{step}_{i}"] = d
    return a


def _draws(s, nvis, step):
    if step <= 3000:
        return []
    u = lambda *shape: s.uniform(shape, -0.5, 0.5).astype(np.float32)   # noqa: E731
    out = [u(nvis, F), u(nvis, 6), u(nvis, K, 3)]
    if step > 10000:
        r = np.minimum((0.06 + 0.94 * s.uniform((N,))).astype(np.float32), np.float32(0.99999994))      # values of [0, 1), as rand_like's
        r[[3] + list(range(7, 7 + 6 * (N_CHOSEN - 1), 6))] = np.float32(0.01)
        out += [r, u(N_CHOSEN, F), u(N_CHOSEN, 6), u(N_CHOSEN, K, 3)]
    return out


def draws(a, step):
    """the recorded draws of a step, in the branch's order"""
    out, i = [], 0
    while f"draw_{step}_{i}" in a:
        out.append(a[f"draw_{step}_{i}"])
        i += 1
    return out


def Replay(a, step, torch):
    """branch_common.Replay on the recorded draws of a run"""
    return branch_common.Replay(draws(a, step), torch)


def model(a, torch, device="cpu", dtype=None):
    """(pc, cam, visible_mask): a SimpleNamespace with everything HAC++'s generate_neural_gaussians touches in training mode, minus the two
    rate modules (pc.EG_mix_prob_2, pc.entropy_gaussian), which the caller attaches: the reference's, the library's or a restatement."""
    dtype = dtype or torch.float32
    nn = torch.nn
    t = lambda x: torch.tensor(np.asarray(x)).to(device=device, dtype=dtype)   # noqa: E731
    pc = types.SimpleNamespace(feat_dim=F, n_offsets=K, decoded_version=False, use_feat_bank=False, bound_updates=0)
    pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc.get_mask = t(a["anchor"]), t(a["feat"]), t(a["offset"]), t(a["scaling"]), t(a["mask"])
    pc.get_mask_anchor = (pc.get_mask.sum(dim=1) > 0).to(dtype)            # (N, 1)
    pc.rotation_activation = torch.nn.functional.normalize
    pc.get_opacity_mlp = _sequential(torch, a, "opacity", nn.Tanh(), device, dtype)
    pc.get_cov_mlp = _sequential(torch, a, "cov", None, device, dtype)
    pc.get_color_mlp = _sequential(torch, a, "color", nn.Sigmoid(), device, dtype)
    pc.get_grid_mlp = _sequential(torch, a, "grid", None, device, dtype)
    A, b = t(a["interp_A"]), t(a["interp_b"])
    pc.calc_interp_feat = lambda x: torch.sin(x @ A + b)

    class ChannelCtx(nn.Module):
        def __init__(self):
            super().__init__()
            for c in range(5):
                seq = nn.Sequential(nn.Linear(3 * F + 10 * c, 40), nn.LeakyReLU(inplace=True), nn.Linear(40, 30))
                with torch.no_grad():
                    for lin, tag in ((seq[0], "1"), (seq[2], "2")):
                        lin.weight.copy_(torch.tensor(a[f"deform{c}_w{tag}"])); lin.bias.copy_(torch.tensor(a[f"deform{c}_b{tag}"]))
                setattr(self, f"MLP_d{c}", seq)

        def forward(self, fea_q, mean_scale, to_dec=-1):
            d = torch.split(fea_q, [10] * 5, dim=-1)
            outs = [torch.chunk(getattr(self, f"MLP_d{c}")(torch.cat(list(d[:c]) + [mean_scale], dim=-1)), chunks=3, dim=-1) for c in range(5)]
            return tuple(torch.cat([o[i] for o in outs], dim=-1) for i in range(3))

    pc.get_deform_mlp = ChannelCtx().to(device=device, dtype=dtype)

    def update_anchor_bound():
        pc.bound_updates += 1
    pc.update_anchor_bound = update_anchor_bound
    cam = types.SimpleNamespace(camera_center=t(a["cam"]))
    return pc, cam, torch.tensor(np.asarray(a["vis"]), device=device)


# ---- tests/golden/hacpp_train.npz (tests/golden/make_hacpp_train_golden.py) -----------------------------------------------------------

def stored(g, step):
    """(outputs {name: array}, keep mask, {name: tolerance}) of a step"""
    pre = f"step{step}/"
    table = g[pre + "out"]
    outs, at = {}, 0
    for k, w in zip(OUTPUTS[:5], (3, 3, 1, 3, 4)):
        outs[k] = table[:, at:at + w]
        at += w
    outs["neural_opacity"] = g[pre + "neural_opacity"]
    keep = np.unpackbits(g[pre + "keep"])[:int(g[pre + "keep_len"])].astype(bool)
    tol = dict(zip((str(n) for n in g[pre + "names"]), g[pre + "tol"]))
    if pre + "rates" in g:
        outs.update(zip(RATES, g[pre + "rates"]))
    return outs, keep, tol


def compare(res, g, step):
    """asserts an 11-tuple against the stored outputs of a step within the stored tolerances; prints every figure first"""
    outs, keep, tol = stored(g, step)
    assert len(res) == 11
    assert np.array_equal(res[6].cpu().numpy(), keep)
    for k, v in zip(OUTPUTS, res[:6]):
        v = v.detach().double().cpu().numpy()
        assert v.shape == outs[k].shape, k
        err = float(np.abs(v - outs[k]).max())
        print(f"step {step} {k}: {err:.3e} (tolerance {tol[k]:.3e})")
        assert err <= tol[k], (step, k, err, tol[k])
    for k, v in zip(RATES, res[7:]):
        if step <= 10000:
            assert v is None and k not in outs
            continue
        rel = abs(float(v) - float(outs[k])) / abs(float(outs[k]))
        print(f"step {step} {k}: {rel:.3e} relative (tolerance {tol[k]:.3e})")
        assert rel <= tol[k] + 2.0 ** -23, (step, k, rel, tol[k])      # the stored value is a float32
