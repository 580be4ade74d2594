"""tests/tcgs_branch_ref.py, the restatement the GPU tests measure gauspcc_amd.tcgs_renderer against, reproduces what the reference's own
TC-GS/gaussian_renderer/__init__.py computed (tests/golden/tcgs_train.npz, written by tests/golden/make_tcgs_train_golden.py): float64 on
the CPU, the recorded draws replayed through the renderer's two hooks.  Also here, without a device: the restatement's mutations move its
outputs as the reference's did, the restated sampler (PlaneRef) is the stand-in-free statement of the tri-plane's contract, and the new
entry points, signatures and constants."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import tcgs_train_cases as tc
from tests.tcgs_branch_ref import estimate_bits_ref, tcgs_branch_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcgs_train.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def arrays():
    return tc.inputs()


def _run(arrays, tag, monkeypatch, dtype=torch.float64, mutate=None):
    from gauspcc_amd import tcgs_renderer

    _, train, step, with_vis, decoded = tc.run(tag)
    pc, cam, vis = tc.model(arrays, torch, "cpu", dtype, decoded=decoded)
    replay = tc.Replay(arrays, tag, torch)
    monkeypatch.setattr(tcgs_renderer, "_uniform_like", replay.uniform_like)
    monkeypatch.setattr(tcgs_renderer, "_rand_like", replay.rand_like)
    with torch.no_grad():
        res = tcgs_branch_ref(cam, pc, vis if with_vis else None, step, is_training=train, mutate=mutate)
    assert not replay.queue and replay.served == tc.expected_draws(step, train)
    assert pc.hooks == tc.expected_hooks(step, train)
    return res


def test_inputs_unchanged(golden, arrays):
    assert str(golden["inputs_sha256"]) == tc.sha256_of(arrays)
    assert tuple(str(t) for t in golden["runs"]) == tuple(r[0] for r in tc.RUNS)
    assert {r[2] for r in tc.RUNS if r[1] and not r[3]} == set(tc.TRAIN_STEPS)
    assert tc.rounding_violations(arrays) == 0
    r = arrays["draw/train20000/3"]
    masked = arrays["mask"].sum(axis=(1, 2)) == 0
    assert (r <= 0.05).sum() >= 6 and ((r > 0.05) & (r <= 0.15)).sum() >= 6 and ((r <= 0.15) & masked).any()     # a fully masked anchor among the chosen
    idx = (np.arange(tc.N)[:, None] + 7 * np.arange(tc.KNN)[None, :]) % tc.N
    assert all(len(set(row)) == tc.KNN for row in idx)                                                            # distinct neighbours


@pytest.mark.parametrize("tag", [r[0] for r in tc.RUNS])
def test_restatement_reproduces_the_reference(golden, arrays, tag, monkeypatch):
    tc.compare(_run(arrays, tag, monkeypatch), golden, tag)


@pytest.mark.parametrize("mutate", tc.MUTATIONS)
def test_restatement_mutations_move_as_the_references_did(golden, arrays, mutate, monkeypatch):
    """each of the generator's mutations, restated, leaves the stored outputs by >= 100 x the tolerance: the restatement has the same parts"""
    tag = "train20000"
    assert float(golden[f"{tag}/mutation_{mutate}"]) >= 100
    res = _run(arrays, tag, monkeypatch, mutate=mutate)
    outs, keep, tol = tc.stored(golden, tag)
    worst = 0.0
    if np.array_equal(res[6].numpy(), keep):
        for k, v in zip(tc.OUTPUTS, res[:6]):
            worst = max(worst, float(np.abs(v.numpy() - outs[k]).max()) / tol[k])
        for k, v in zip(tc.RATES, res[7:]):
            worst = max(worst, abs(float(v) - float(outs[k])) / (tol[k] * abs(float(outs[k]))))
    else:
        worst = np.inf
    assert worst >= 100, (mutate, worst)


def test_fixture_records_its_own_checks(golden):
    for tag, train, step, _, _ in tc.RUNS:
        if train:
            assert float(golden[f"{tag}/opacity_margin"]) >= tc.OPACITY_MARGIN
        names = [str(n) for n in golden[f"{tag}/names"]]
        for n, d, t in zip(names, golden[f"{tag}/f32_vs_f64"], golden[f"{tag}/tol"]):
            assert t == max(tc.OUT_TOL.get(n, tc.RATE_RTOL), 4 * d), (tag, n)
        rates = [str(n) for n in golden[f"{tag}/rate_names"]]
        assert rates == (list(tc.RATES) if train and step > 15000 else list(tc.RATES[:4]) if train and step > 10000 else [])


def test_estimate_restatement_runs_on_the_stand_in(arrays):
    """estimate_bits_ref on the CPU model: finite, positive, and the masked anchors are left out (their neighbours' rows are not read)"""
    pc, _, _ = tc.model(arrays, torch, "cpu", torch.float64)
    kept = int(pc.get_mask_anchor.sum())
    assert kept == tc.N - 2
    idx = (torch.arange(kept)[:, None] + 7 * torch.arange(tc.KNN)[None, :]) % kept
    bits = estimate_bits_ref(pc, idx)
    assert all(np.isfinite(b) and b > 0 for b in bits)


def test_plane_ref_is_the_samplers_contract():
    """PlaneRef against a direct evaluation of include/gauspcc.h's formulas at one in-range sample (float64)"""
    from tests.tcgs_branch_ref import PlaneRef

    g = torch.Generator().manual_seed(3)
    planes = torch.randn(3, 2, 8, 8, generator=g, dtype=torch.float64)
    ref = PlaneRef(planes, radii=5.0)
    mx, mn = torch.tensor([2.0, 2.2, 2.4], dtype=torch.float64), torch.tensor([-2.1, -2.3, -2.5], dtype=torch.float64)
    c = torch.tensor([[[0.31, 0.52, 0.43]]], dtype=torch.float64)
    out = ref(c, mx, mn).detach().view(3, 2)
    proj = ((0, 1), (0, 2), (2, 0))
    comp = ((1, 2), (0, 2), (0, 1))
    for p in range(3):
        i, j = proj[p]
        mag = min(min(float(mx[i] ** 2 + mx[j] ** 2), float(mn[i] ** 2 + mn[j] ** 2)), 2.5 ** 2) ** 0.5
        x = [6 * (2 * float(c[0, 0, d]) / mag * 2 - 1) for d in comp[p]]
        m = max(x[0] ** 2 + x[1] ** 2, float(np.finfo(np.float32).eps))
        s = 1.0 if m <= 1 else (2 * m ** 0.5 - 1) / m
        ix, iy = ((s * x[0] / 2 + 1) * 8 - 1) / 2, ((s * x[1] / 2 + 1) * 8 - 1) / 2
        x0, y0 = int(np.floor(ix)), int(np.floor(iy))
        want = torch.zeros(2, dtype=torch.float64)
        for yy, wy in ((y0, y0 + 1 - iy), (y0 + 1, iy - y0)):
            for xx, wx in ((x0, x0 + 1 - ix), (x0 + 1, ix - x0)):
                if 0 <= xx < 8 and 0 <= yy < 8:
                    want += planes[p, :, yy, xx] * wx * wy
        assert torch.allclose(out[p], want, atol=1e-12), (p, out[p], want)


def test_new_entry_points_and_signatures():
    from gauspcc_amd import _lib, tcgs_codec, tcgs_renderer, triplane
    from gauspcc_amd.neural_gaussians import quantise_steps

    assert {"gsge_plane_rows_forward", "gsge_plane_rows_backward", "gsnn_quantise", "gsnn_mean"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.gsge_plane_rows_forward and L.gsge_plane_rows_backward and L.gsnn_quantise and L.gsnn_mean
    assert list(inspect.signature(quantise_steps).parameters) == ["xs", "q0s", "adj", "cols", "base", "means"]
    assert list(inspect.signature(triplane.triplane_rows).parameters) == ["planes", "coordinates", "tail", "max_coords", "min_coords", "radii", "repeat"]
    assert list(inspect.signature(triplane.Triplane.context_rows).parameters) == ["self", "sample_coordinates", "tail", "max_coords", "min_coords", "is_training",
                                                                                 "step", "repeat"]
    sig = inspect.signature(tcgs_renderer.generate_neural_gaussians)
    assert [(k, p.default) for k, p in sig.parameters.items()][2:] == [("visible_mask", None), ("is_training", False), ("step", 0)]
    assert (tcgs_renderer.Q_FEAT, tcgs_renderer.Q_SCALING, tcgs_renderer.Q_OFFSETS, tcgs_renderer.K) == (1, 0.001, 0.3, 4)
    assert list(inspect.signature(tcgs_codec.estimate_final_bits).parameters) == ["self"]


def test_argument_checks_need_no_device():
    from gauspcc_amd.neural_gaussians import quantise_steps
    from gauspcc_amd.triplane import triplane_rows

    x = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        quantise_steps([x], [1.0], None)
    with pytest.raises(ValueError):
        quantise_steps([x], [1.0], torch.zeros(4, 1))          # CPU tensors
    with pytest.raises((TypeError, RuntimeError)):
        triplane_rows(torch.zeros(3, 2, 4, 4), torch.zeros(4, 3), x, torch.ones(3), -torch.ones(3), 1.0, repeat=4)
