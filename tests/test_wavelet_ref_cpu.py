"""tests/wavelet_ref.py on the CPU: the float64 restatement (quads) and the float32 conv2d program agree with what the reference's own
wavelet_loss recorded (tests/golden/wavelet.npz), the two forms of the transform agree with each other, the stand-in inverts itself,
and pick_seed keeps every difference coefficient of the GPU tests' shapes away from zero."""
import os

import numpy as np
import pytest
import torch

from tests import wavelet_ref as wr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavelet.npz")
SHAPES = [(3, 24, 32), (3, 13, 18), (3, 37, 41)]
STEPS = [0, 12000, 25000, 25001, 30000]
GPU_SHAPES = [(3, 1, 1), (3, 2, 3), (3, 5, 6), (3, 13, 18), (3, 24, 32), (3, 37, 41), (1, 9, 7)]   # tests/test_gpu_wavelet.py


def _case(g, shape, step):
    name = "x".join(map(str, shape))
    return torch.tensor(g[f"{name}_img1"]), torch.tensor(g[f"{name}_img2"]), f"{name}_s{step}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_and_program_match_the_fixture(shape):
    g = np.load(GOLDEN)
    for step in STEPS:
        x, y, k = _case(g, shape, step)
        ref = float(g[f"{k}_value"])
        # float64 on the quads: the reference's own float64 run to rounding
        v64, d1, d2 = wr.grads(lambda a, b: wr.wavelet_loss64(a, b, step)[0], x, y, torch.float64)
        assert abs(float(v64) - ref) <= 1e-12 * abs(ref)
        for d, name in ((d1, "grad1"), (d2, "grad2")):
            want = g[f"{k}_{name}"]
            assert np.abs(d.numpy() - want).max() <= 1e-12 * np.abs(want).max(), (k, name)
        # the float32 program: what the reference's float32 run gave
        v32, h1, h2 = wr.grads(lambda a, b: wr.wavelet_loss(a, b, step), x, y, torch.float32)
        assert abs(float(v32) - float(g[f"{k}_value32"])) <= 2e-7 * abs(ref)
        for h, name, e in ((h1, "grad1", g[f"{k}_grad32_err"][0]), (h2, "grad2", g[f"{k}_grad32_err"][1])):
            want = g[f"{k}_{name}"]
            assert np.abs(h.double().numpy() - want).max() <= e + 1e-7 * np.abs(want).max(), (k, name)


def test_fixture_inputs_are_the_helper_images():
    g = np.load(GOLDEN)
    for shape in SHAPES:
        name = "x".join(map(str, shape))
        x, y = wr.make_images(shape, int(g[f"{name}_seed"]))
        assert np.array_equal(x.numpy(), g[f"{name}_img1"]) and np.array_equal(y.numpy(), g[f"{name}_img2"])
        assert wr.min_abs_coef(x, y) >= wr.MIN_COEF


@pytest.mark.parametrize("shape", [(1, 3, 24, 32), (1, 3, 13, 18), (2, 3, 9, 7), (1, 3, 1, 1), (1, 3, 5, 6), (1, 1, 2, 3), (1, 3, 37, 41)],
                         ids=lambda s: "x".join(map(str, s)))
def test_quads_equal_the_conv_program(shape):
    x = torch.rand(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    for J in (1, 2, 3):
        ll, yh = wr.dwt_conv(x, J)
        ll2, yh2 = wr.dwt_quads(x, J)
        assert ll.shape == ll2.shape and float((ll - ll2).abs().max()) <= 1e-14
        H, W = shape[-2:]
        for a, b in zip(yh, yh2):
            H, W = (H + 1) // 2, (W + 1) // 2
            assert a.shape == b.shape == shape[:2] + (3, H, W) and float((a - b).abs().max()) <= 1e-14
        back = wr.DWTInverse()((ll, yh))
        assert back.shape[-2:] == (2 * yh[0].shape[-2], 2 * yh[0].shape[-1])
        assert float((back[..., : shape[-2], : shape[-1]] - x).abs().max()) <= 1e-14
        assert float((wr.idwt_quads(ll2, yh2) - back).abs().max()) <= 1e-14


def test_band_zero_is_high_along_the_height():
    x = torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    x[..., 0::2, :] = 1.0                              # rows alternate: high along the height only
    _, yh = wr.dwt_conv(x, 1)
    assert float(yh[0][0, 0, 0].min()) == pytest.approx(1.0) and float(yh[0][0, 0, 1:].abs().max()) <= 1e-15
    _, yh = wr.dwt_conv(x.transpose(-1, -2).contiguous(), 1)
    assert float(yh[0][0, 0, 1].min()) == pytest.approx(1.0) and float(yh[0][0, 0, [0, 2]].abs().max()) <= 1e-15


def test_pick_seed_meets_its_bound():
    for shape in GPU_SHAPES + [(2, 3, 13, 18), (1, 3, 37, 41)]:
        seed = wr.pick_seed(shape)
        assert 0 <= seed < 16
        assert wr.min_abs_coef(*wr.make_images(shape, seed)) >= wr.MIN_COEF
    assert wr.pick_seed((3, 24, 32)) == 1          # seed 0 has a coefficient of 2e-6
    x, y = wr.make_images((3, 24, 32), 0)
    assert wr.min_abs_coef(x, y) < wr.MIN_COEF and wr.unsafe_pixels(x, y).any() and wr.unsafe_pixels(x, y).shape == x.shape
    assert not wr.unsafe_pixels(*wr.make_images((3, 24, 32), 1)).any()


def test_weights_follow_the_branch():
    assert wr.band_weights(0) == [1.0] + [0.0] * 6
    assert wr.band_weights(25000)[0] == 1.0 - 25000 / 30000 and wr.band_weights(25001)[0] == 0.0
    assert wr.band_weights(30000)[1:4] == [0.0, 0.0, 0.0] and wr.band_weights(30000)[4:] == [0.4, 0.3, 0.3]
