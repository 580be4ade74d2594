"""tests/arm_ref.py (the project's float64 restatement of CAT-3DGS's tri-plane ARM rate term) against the values recorded from the
reference's own scene/arm.py (tests/golden/arm_rate.npz, written by tests/golden/make_arm_golden.py); the conditions the fixture was
built to have; and gauspcc_amd.arm.ArmMLP's state-dict compatibility with the reference's scripted module.

"To float32 rounding": the recorded values are float32 results of the same formulas, so their distance from float64 is compared with
that of this project's float32 torch sequence (arm_ref.rate_torch) on the same inputs: at most 4 times its largest error per quantity,
plus 1e-6 of the quantity's scale for quantities the float32 sequence happens to get exactly."""
import os

import numpy as np
import pytest
import torch

from tests import arm_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arm_rate.npz")
SHAPES = [(1, 3, 5, 7), (1, 3, 10, 14), (1, 2, 1, 2), (1, 1, 6, 1)]


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: arm_ref.golden_case(z, k) for k in arm_ref.CASES}


def _torch32(c):
    levels = [torch.from_numpy(y).clone().requires_grad_(True) for y in c["levels"]]
    params = [torch.from_numpy(p).clone().requires_grad_(True) for p in c["params"]]
    rate, mu, scale = arm_ref.rate_torch(levels, params)
    (rate * torch.from_numpy(c["w"])).sum().backward()
    return rate.detach().numpy(), mu.detach().numpy(), scale.detach().numpy(), [y.grad.numpy() for y in levels], [p.grad.numpy() for p in params]


@pytest.mark.parametrize("key", arm_ref.CASES)
def test_restatement_reproduces_the_reference(golden, key):
    c = golden[key]
    assert [tuple(y.shape) for y in c["levels"]] == SHAPES and c["rate"].shape == (535,)
    f = arm_ref.forward64(c["levels"], c["params"])
    gl, gp, _ = arm_ref.grads64(c["levels"], c["params"], c["w"], f)
    rate32, mu32, s32, gl32, gp32 = _torch32(c)

    def close(name, gold, ref, own32):
        ref = np.asarray(ref).reshape(gold.shape)
        err, own = np.abs(gold - ref).max(), np.abs(own32.reshape(gold.shape) - ref).max()
        assert err <= 4 * own + 1e-6 * max(np.abs(ref).max(), 1e-30), (key, name, err, own)

    close("rate", c["rate"], f["rate"], rate32)
    close("mu", c["mu"], f["mu"], mu32)
    close("scale", c["scale"], f["scale"], s32)
    for i in range(len(gl)):
        close(f"g_level{i}", c["g_levels"][i], gl[i], gl32[i])
    for j in range(len(gp)):
        close(f"g_{c['keys'][j]}", c["g_params"][j], gp[j], gp32[j])
    # the floor set is the same in float32 and float64
    on64 = f["p0"] < arm_ref.P_FLOOR
    assert np.array_equal(c["rate"] == 16.0, on64)


def test_fixture_conditions(golden):
    for key in ("round", "noise"):
        f = arm_ref.forward64(golden[key]["levels"], golden[key]["params"])
        share = float(np.mean(f["p0"] < arm_ref.P_FLOOR))
        assert 0.05 <= share <= 0.25, (key, share)
        assert not ((f["ls"] < arm_ref.LS_MIN) | (f["ls"] > arm_ref.LS_MAX)).any()
        assert arm_ref.near_floor(f["p0"], 1e-3).sum() <= 0.01 * f["p0"].size
    assert np.array_equal(golden["round"]["levels"][1], np.round(golden["round"]["levels"][1]))
    assert not np.array_equal(golden["noise"]["levels"][1], np.round(golden["noise"]["levels"][1]))
    k = golden["kinks"]
    f = arm_ref.forward64(k["levels"], k["params"])
    below, above = f["ls"] < arm_ref.LS_MIN, f["ls"] > arm_ref.LS_MAX
    assert below.sum() >= 10 and above.sum() >= 10
    # by the reference's own output: the scale sits on exp(5) and on exp(-0.5 * 13.8155) exactly there
    assert np.array_equal(k["scale"] == k["scale"].max(), below) and np.array_equal(k["scale"] == k["scale"].min(), above)
    inside = ~below & ~above & (f["p0"] >= arm_ref.P_FLOOR)
    assert inside.sum() >= 100
    assert golden["wide"]["layers"] == [24, 24, 8]


def test_layout_is_the_5x5_causal_half():
    y = np.arange(3 * 10 * 14, dtype=np.float64).reshape(3, 10, 14)
    ctx = arm_ref.contexts64(y).reshape(3, 10, 14, 12)
    assert np.array_equal(ctx[1, 3, 4], np.concatenate([y[1, 1:3, 2:7].reshape(-1), y[1, 3, 2:4]]))
    assert np.array_equal(ctx[2, 0, 0], np.zeros(12))                     # nothing from channel 1
    t = arm_ref.contexts_torch(torch.from_numpy(y)[None]).numpy()
    assert np.array_equal(t, ctx.reshape(-1, 12))


@pytest.mark.parametrize("key", ["round", "wide"])
def test_armmlp_loads_the_reference_state_dict(golden, key):
    from gauspcc_amd.arm import ArmMLP

    c = golden[key]
    arm = ArmMLP(12, c["layers"])
    assert list(arm.state_dict().keys()) == c["keys"]
    zero = [k for k, v in arm.state_dict().items() if float(v.abs().max()) == 0.0]
    res = [f"mlp.{2 * l}.w" for l, (a, b) in enumerate(zip([12] + c["layers"][:-1], c["layers"])) if a == b]
    assert sorted(zero) == sorted(res + [k for k in c["keys"] if k.endswith(".b")])
    arm.load_state_dict({k: torch.from_numpy(p) for k, p in zip(c["keys"], c["params"])}, strict=True)
    # its forward is the torch formula: the recorded mu of the first level's first latents
    ctx = arm_ref.contexts_torch(torch.from_numpy(c["levels"][0]))
    with torch.no_grad():
        raw = arm(ctx)
    assert raw.shape == (105, 2)
    assert np.allclose(raw[:, 0].numpy(), c["mu"][:105], rtol=1e-5, atol=1e-6)
    with pytest.raises(NotImplementedError):
        ArmMLP(12, c["layers"], fpfm=8)
    with pytest.raises(NotImplementedError):
        arm.set_quant(8)


def test_library_exports_the_arm_entry_points():
    import ctypes
    import re

    from gauspcc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gauspcc.h")).read()
    declared = sorted(set(re.findall(r"GPCC_API\s+[\w\s\*]*?\b(gsarm_\w+)\s*\(", header)))
    assert declared == sorted(_lib.EXPORTS_ARM) and len(declared) == 2
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(so, name), name
