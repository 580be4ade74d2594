"""CPU side of the GausPcgc training path: the float64 restatement (tests/pcgc_ref.py) against the oracle, gradcheck, the module's
upstream key set, the trainer's flags and patch split."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from gauspcc_amd.model import tensor_table
from gauspcc_amd.synth import synthetic_cloud, synthetic_state_dict
from oracle import oracle as orc

from . import pcgc_ref as ref
from .test_model_loader import UPSTREAM_KEYS


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("res_relu", [False, True])
def test_ref_conv_matches_the_oracle(k, res_relu):
    rng = np.random.default_rng(k)
    pts = np.unique(rng.integers(-12, 12, size=(600, 3)), axis=0).astype(np.int32)
    pts = pts[orc.raster_order(pts)]
    x = rng.standard_normal((pts.shape[0], 32)).astype(np.float32)
    w = (rng.standard_normal((k ** 3, 32, 32)) * 0.1).astype(np.float32)
    r = rng.standard_normal(x.shape).astype(np.float32) if res_relu else None
    want = orc.conv(x, orc.nbr(pts, k), w, r, res_relu)
    got = ref.conv(torch.tensor(x, dtype=torch.float64), ref.neighbours(pts, k), torch.tensor(w, dtype=torch.float64),
                   None if r is None else torch.tensor(r, dtype=torch.float64), res_relu).numpy()
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("k", [3, 5])
def test_ref_total_bits_matches_the_oracle_encoder(k):
    pts = synthetic_cloud(3000, seed=5)
    sd = synthetic_state_dict(32, k, seed=3)
    orc.encode(orc.Model(tensor_table(sd, 32, k), 32, k), pts, chunk_log2=11)
    want = orc.ideal_bits()
    got = float(ref.total_bits(ref.params(sd), pts, k))
    assert abs(got - want) <= 1e-5 * want


def test_ref_gradcheck_on_a_tiny_cloud():
    rng = np.random.default_rng(2)
    pts = np.unique(rng.integers(0, 24, size=(300, 3)), axis=0)
    levels = ref.build_levels(pts)
    (pc, po), (cc, co) = levels[-2], levels[-1]
    nb = ref.neighbours(cc, 3)
    x = torch.randn(cc.shape[0], 4, dtype=torch.float64, requires_grad=True)
    w = (0.3 * torch.randn(27, 4, 4, dtype=torch.float64)).requires_grad_(True)
    r = torch.randn(cc.shape[0], 4, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b, c: ref.conv(a, nb, b, c, True), (x, w, r))


def test_network_has_the_upstream_key_set_and_round_trips():
    from gauspcc_amd.pcgc_net import Network

    for k in (3, 5):
        net = Network(32, k)
        sd = net.state_dict()
        assert sorted(sd) == sorted(UPSTREAM_KEYS)
        want = synthetic_state_dict(32, k)
        assert all(tuple(sd[key].shape) == want[key].shape for key in want)
        assert torch.equal(sd["fog.conv.kernel"], torch.ones(8, 1, 1))
        assert len(list(net.parameters())) == 39
        net.load_state_dict(want)
        got = tensor_table(net.state_dict(), 32, k)
        assert all(np.array_equal(a, b) for a, b in zip(got, tensor_table(want, 32, k)))
    with pytest.raises(ValueError):
        Network(16, 5)


def test_trainer_help_carries_the_upstream_flags():
    out = subprocess.run([sys.executable, "-m", "gauspcc_amd.cli.train", "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--training_data", "--val_data", "--model_save_folder", "--channels", "--kernel_size", "--learning_rate", "--lr_decay",
                 "--lr_decay_steps", "--max_steps", "--val_interval", "--log_interval", "--is_data_pre_quantized", "--batch_size"):
        assert flag in out


def test_patch_split_partitions_the_cloud_deterministically():
    from gauspcc_amd.cli.train import split_patches

    pts = synthetic_cloud(20000, seed=9)
    parts = split_patches(pts, 3000)
    assert all(p.shape[0] <= 3000 for p in parts) and len(parts) >= 7
    u = np.concatenate(parts)
    assert u.shape == pts.shape
    assert np.array_equal(np.unique(u, axis=0), np.unique(pts, axis=0))
    again = split_patches(pts, 3000)
    assert all(np.array_equal(a, b) for a, b in zip(parts, again))
