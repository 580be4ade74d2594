"""Host-side pieces of gauspcc_amd.anchor_codec (no GPU): the slice geometry the four conduct_encoding / conduct_decoding drop-ins share, and
the recognition of the context MLPs that go through the device kernel."""
import os

import pytest
import torch

from gauspcc_amd import anchor_codec

K = 10
N_CASES = {"0": lambda mb: 0, "1": lambda mb: 1, "mb-1": lambda mb: mb - 1, "mb": lambda mb: mb, "mb+1": lambda mb: mb + 1, "2mb+37": lambda mb: 2 * mb + 37}


def test_file_names():
    assert anchor_codec.slice_file_names("/x/y", "feat2", 3) == [os.path.join("/x/y", f"feat2_{s}.b") for s in range(3)]
    assert anchor_codec.slice_file_names("d", "offsets", 0) == []


@pytest.mark.parametrize("max_batch", [500, 1000, 3000])
@pytest.mark.parametrize("case", list(N_CASES))
def test_slice_and_offset_bounds(case, max_batch):
    N = N_CASES[case](max_batch)
    b = anchor_codec.slice_bounds(N, max_batch)
    steps = -(-N // max_batch)
    assert len(b) == steps + 1 and b[0] == 0 and b[-1] == N
    assert all(0 < y - x <= max_batch for x, y in zip(b, b[1:])) and all(y - x == max_batch for x, y in zip(b[:-1], b[1:-1]))
    assert anchor_codec.n_slices(N, max_batch) == steps
    g = torch.Generator().manual_seed(N)
    mask = torch.rand(N, 3 * K, generator=g) < 0.4
    ob = anchor_codec.offset_bounds(mask.reshape(-1), N, b)
    assert ob == [int(mask[:x].sum()) for x in b]


def test_offsets_mask():
    g = torch.Generator().manual_seed(1)
    m = (torch.rand(7, K, 1, generator=g) < 0.5).float()
    flat = anchor_codec.offsets_mask(m)
    assert flat.dtype == torch.bool and flat.shape == (7 * K * 3,)
    assert torch.equal(flat.view(7, K, 3), m.bool().expand(7, K, 3))
    assert anchor_codec.offsets_mask(torch.zeros(0, K, 1)).shape == (0,)


def test_mlp2_parts_and_run_mlp2():
    from gauspcc_amd.mlp import ContextMLP

    nn = torch.nn
    m = nn.Sequential(nn.Linear(5, 7), nn.ReLU(True), nn.Linear(7, 3))
    w1, b1, w2, b2, act, slope = anchor_codec.mlp2_parts(m)
    assert all(a is b for a, b in zip((w1, b1, w2, b2), (m[0].weight, m[0].bias, m[2].weight, m[2].bias))) and (act, slope) == ("relu", 0.0)
    m = nn.Sequential(nn.Linear(5, 7), nn.LeakyReLU(0.2), nn.Linear(7, 3))
    parts = anchor_codec.mlp2_parts(m)
    assert parts[0] is m[0].weight and parts[3] is m[2].bias and parts[4:] == ("leaky_relu", 0.2)
    for cm in (ContextMLP(5, 7, 3), ContextMLP(5, 7, 3, "leaky_relu", 0.05)):
        parts = anchor_codec.mlp2_parts(cm)
        assert parts[0] is cm[0].weight and parts[2] is cm[2].weight
        assert parts[4:] == (("relu", 0.0) if isinstance(cm[1], nn.ReLU) else ("leaky_relu", 0.05))

    class Plain(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = nn.Linear(5, 7), nn.Linear(7, 3)

        def forward(self, x):
            return self.b(torch.relu(self.a(x)))

    others = [nn.Sequential(nn.Linear(5, 7), nn.ReLU(), nn.Linear(7, 7), nn.Linear(7, 3)),      # four modules
              nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3)),
              nn.Sequential(nn.Linear(5, 7, bias=False), nn.ReLU(), nn.Linear(7, 3)),
              nn.Sequential(nn.Linear(5, 7), nn.ReLU(), nn.Linear(7, 3, bias=False)),
              Plain()]
    x = torch.randn(11, 5, generator=torch.Generator().manual_seed(0))
    for o in others:
        assert anchor_codec.mlp2_parts(o) is None
        with torch.no_grad():
            assert torch.equal(anchor_codec.run_mlp2(o, x), o(x))
