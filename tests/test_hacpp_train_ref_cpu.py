"""tests/hacpp_branch_ref.py, the restatement the GPU tests measure gauspcc_amd.hac_plus_renderer against, reproduces what the reference's
own HAC-plus/gaussian_renderer/__init__.py computed in training mode (tests/golden/hacpp_train.npz, written by
tests/golden/make_hacpp_train_golden.py): float64 on the CPU, the recorded draws replayed through the renderer's two hooks."""
import os

import numpy as np
import pytest
import torch

from tests import hacpp_train_cases as hc
from tests.hacpp_branch_ref import hacpp_branch_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hacpp_train.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def arrays():
    return hc.inputs()


def test_inputs_unchanged(golden, arrays):
    assert str(golden["inputs_sha256"]) == hc.sha256_of(arrays)
    assert tuple(golden["steps"]) == hc.STEPS
    chosen = arrays["draw_12000_3"] <= 0.05
    assert chosen.sum() >= 16 and (arrays["mask"][chosen].sum(axis=(1, 2)) == 0).any()


@pytest.mark.parametrize("step", hc.STEPS)
def test_restatement_reproduces_the_reference(golden, arrays, step, monkeypatch):
    from gauspcc_amd import hac_plus_renderer

    pc, cam, vis = hc.model(arrays, torch, "cpu", torch.float64)
    replay = hc.Replay(arrays, step, torch)
    monkeypatch.setattr(hac_plus_renderer, "_uniform_like", replay.uniform_like)
    monkeypatch.setattr(hac_plus_renderer, "_rand_like", replay.rand_like)
    with torch.no_grad():
        res = hacpp_branch_ref(cam, pc, vis, step)
    assert not replay.queue and replay.served == (0 if step <= 3000 else 3 if step <= 10000 else 7)
    assert pc.bound_updates == (1 if step == 10000 else 0)
    hc.compare(res, golden, step)


def test_fixture_records_its_own_checks(golden):
    for step in hc.STEPS:
        assert float(golden[f"step{step}/opacity_margin"]) >= hc.OPACITY_MARGIN
        names = [str(n) for n in golden[f"step{step}/names"]]
        for n, d, t in zip(names, golden[f"step{step}/f32_vs_f64"], golden[f"step{step}/tol"]):
            floor = hc.OUT_TOL.get(n, hc.RATE_RTOL)
            assert t == max(floor, 4 * d), (step, n)
    for m in ("swap_draws", "drop_mask_anchor", "nine_way"):
        assert float(golden[f"step12000/mutation_{m}"]) >= 100
