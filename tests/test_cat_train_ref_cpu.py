"""tests/cat_branch_ref.py, the restatement the GPU tests measure gauspcc_amd.cat_renderer against, reproduces what the reference's own
CAT-3DGS/gaussian_renderer/__init__.py computed (tests/golden/cat_train.npz, written by tests/golden/make_cat_train_golden.py): float64 on
the CPU, the recorded draws replayed through the renderer's two hooks.  Also here, without a device: the restatement's mutations move its
outputs as the reference's did, the stage table the drop-in uses is the restatement's, and chain_rate's argument checks."""
import os

import numpy as np
import pytest
import torch

from tests import cat_train_cases as cc
from tests.cat_branch_ref import cat_branch_ref, stages_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cat_train.npz")
MUTATIONS = ("hac_order", "base1", "drop_residual", "drop_offset_mask", "no_mask_anchor")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def arrays():
    return cc.inputs()


def _run(arrays, tag, monkeypatch, dtype=torch.float64, mutate=None):
    from gauspcc_amd import cat_renderer

    _, name, train, step, wm, decoded = cc.run(tag)
    pc, cam, vis, wmask = cc.model(arrays, name, torch, "cpu", dtype, decoded=decoded)
    replay = cc.Replay(arrays, tag, torch)
    monkeypatch.setattr(cat_renderer, "_uniform_like", replay.uniform_like)
    monkeypatch.setattr(cat_renderer, "_rand_like", replay.rand_like)
    with torch.no_grad():
        res = cat_branch_ref(cam, pc, vis, step, is_training=train, mask=wmask if wm else None, mutate=mutate)
    assert not replay.queue and replay.served == cc.expected_draws(step, train)
    assert pc.bound_updates == (1 if train and step == 10000 else 0)
    return res


def test_inputs_unchanged(golden, arrays):
    assert str(golden["inputs_sha256"]) == cc.sha256_of(arrays)
    assert tuple(str(t) for t in golden["runs"]) == tuple(r[0] for r in cc.RUNS)
    assert {r[3] for r in cc.RUNS if r[2] and r[1] == "main"} == set(cc.TRAIN_STEPS) and {r[3] for r in cc.RUNS if not r[2] and not r[5]} == set(cc.VAL_STEPS)
    assert cc.rounding_violations(arrays) == 0
    vis = arrays["main/vis"]
    chosen = arrays["draw/train12000/3"] <= 0.05
    masked = arrays["main/mask"][vis].sum(axis=(1, 2)) == 0
    assert chosen.sum() >= 12 and (chosen & masked).any()          # a fully masked anchor among the chosen


@pytest.mark.parametrize("tag", [r[0] for r in cc.RUNS])
def test_restatement_reproduces_the_reference(golden, arrays, tag, monkeypatch):
    cc.compare(_run(arrays, tag, monkeypatch), golden, tag)


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_restatement_mutations_move_as_the_references_did(golden, arrays, mutate, monkeypatch):
    """each of the generator's mutations, restated, leaves the stored outputs by >= 100 x the tolerance: the restatement has the same parts"""
    tag = "train12000"
    assert float(golden[f"{tag}/mutation_{mutate}"]) >= 100
    res = _run(arrays, tag, monkeypatch, mutate=mutate)
    outs, keep, tol = cc.stored(golden, tag)
    worst = 0.0
    if np.array_equal(res[6].numpy(), keep):
        for k, v in zip(cc.OUTPUTS, res[:6]):
            worst = max(worst, float(np.abs(v.numpy() - outs[k]).max()) / tol[k])
        for k, v in zip(cc.RATES, res[7:]):
            worst = max(worst, abs(float(v) - float(outs[k])) / (tol[k] * abs(float(outs[k]))))
    else:
        worst = np.inf
    assert worst >= 100, (mutate, worst)


def test_fixture_records_its_own_checks(golden):
    for tag, _, train, step, _, _ in cc.RUNS:
        if train:
            assert float(golden[f"{tag}/opacity_margin"]) >= cc.OPACITY_MARGIN
        names = [str(n) for n in golden[f"{tag}/names"]]
        for n, d, t in zip(names, golden[f"{tag}/f32_vs_f64"], golden[f"{tag}/tol"]):
            assert t == max(cc.OUT_TOL.get(n, cc.RATE_RTOL), 4 * d), (tag, n)
        rates = [str(n) for n in golden[f"{tag}/rate_names"]]
        assert rates == (list(cc.RATES) if train and cc.rate_branch(step) else ["feat_rate"] if not train and tag.startswith("val") and step != 5000 else [])


@pytest.mark.parametrize("name", list(cc.MODELS))
def test_stage_table_is_the_restatements(arrays, name):
    """cat_codec.stage_table -- the one statement of the row layout the drop-in reads -- against the layout written out from the reference"""
    from gauspcc_amd.cat_renderer import _stages

    pc, _, _, _ = cc.model(arrays, name, torch)
    got = [(s["attr"], s["out_col"], s["ch"], s["mean_col"], s["scale_col"], s["dep_ch"], s["mlp"]) for s in _stages(pc)]
    want = stages_of(pc)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:6] == w[:6] and g[6] is w[6], (g, w)
    F = pc.feat_dim
    assert all(s[4] < F <= s[3] for s in want if s[0] == "feat")       # scales come first


def test_quant_noise_signature_keeps_its_default():
    import inspect

    from gauspcc_amd.neural_gaussians import quant_noise

    sig = inspect.signature(quant_noise)
    assert list(sig.parameters) == ["xs", "us", "q0s", "adj", "cols", "base"] and sig.parameters["base"].default == 1.0
    from gauspcc_amd import cat_renderer
    sig = inspect.signature(cat_renderer.generate_neural_gaussians)
    assert [(k, p.default) for k, p in sig.parameters.items()][2:] == [("visible_mask", None), ("is_training", False), ("step", 0), ("mask", None)]
