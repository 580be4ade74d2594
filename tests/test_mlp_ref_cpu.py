"""tests/mlp_ref.py against torch autograd in float64, the new entry point's declaration and export, and the fixture rule's drop rate."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "%d-%d-%d-%s" % s)
def test_closed_form_equals_autograd_in_float64(shape):
    din, dh, dout, act = shape
    x, dy, w, _ = ref.fixture(din, dh, dout, 77, seed=5)
    leaves = [t.double().requires_grad_(True) for t in (x, *w)]
    y = ref.forward(*leaves, act)
    mod = torch.nn.Sequential(torch.nn.Linear(din, dh), torch.nn.ReLU() if act == "relu" else torch.nn.LeakyReLU(ref.SLOPE), torch.nn.Linear(dh, dout)).double()
    with torch.no_grad():
        for p, v in zip((mod[0].weight, mod[0].bias, mod[2].weight, mod[2].bias), w):
            p.copy_(v)
    assert torch.allclose(y, mod(x.double()), rtol=1e-12, atol=1e-12)
    auto = torch.autograd.grad(y, leaves, dy.double())
    mine = ref.closed_form_grads(*(t.detach() for t in leaves), dy.double(), act)
    for a, m in zip(auto, mine):
        assert a.shape == m.shape and torch.allclose(a, m, rtol=1e-12, atol=1e-12)


def test_kink_gradient_follows_torch():
    h = torch.tensor([0.0, -1.0, 2.0], dtype=torch.float64, requires_grad=True)
    for act, f in (("relu", torch.nn.functional.relu), ("leaky_relu", lambda t: torch.nn.functional.leaky_relu(t, ref.SLOPE))):
        g, = torch.autograd.grad(f(h).sum(), h)
        assert torch.equal(g, ref.act_grad(h.detach(), act))


def test_entry_point_is_declared_and_exported():
    from gauspcc_amd import _lib

    header = open(os.path.join(ROOT, "include", "gauspcc.h")).read()
    assert re.search(r"GPCC_API int gshac_mlp2_backward\(gpcc_ctx \*ctx,", header)
    assert re.search(r"GPCC_API int64_t gshac_mlp2_slab_rows\(", header)
    assert {"gshac_mlp2_backward", "gshac_mlp2_slab_rows"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.gshac_mlp2_backward and L.gshac_mlp2_slab_rows
    assert len(L.gshac_mlp2_backward.argtypes) == 21


def test_slab_size_depends_on_n_and_the_sizes_alone():
    from gauspcc_amd.mlp import slab_rows

    for din, dh, dout, _ in ref.SHAPES:
        S = slab_rows(1, din, dh, dout)
        assert S > 0 and S % 16 == 0
        for n in ref.row_counts(S):
            assert slab_rows(n, din, dh, dout) == S          # the GPU tests' row counts sit in one regime
        big = slab_rows(1_000_000, din, dh, dout)
        assert big % 16 == 0 and 256 <= -(-1_000_000 // big) <= 512
    assert slab_rows(10, 2000, 100, 3) == 0                  # 16 (din + dh) floats above 64 KB: not a size the forward takes


def test_fixture_rule_drops_under_five_percent_of_rows():
    from gauspcc_amd.mlp import slab_rows

    for s, (din, dh, dout, _) in enumerate(ref.SHAPES):
        for n in ref.row_counts(slab_rows(1, din, dh, dout)):
            x, dy, _, dropped = ref.fixture(din, dh, dout, n, seed=10 * s)
            assert x.shape == (n, din) and dy.shape == (n, dout)
            assert dropped < 0.05, (din, dh, dout, n, dropped)
