"""tests/mlp_ref.py against torch autograd in float64, the new entry point's declaration and export, the fixture rule's drop rate, and what
tests/test_gpu_mlp_classes.py takes for granted: the kernel and slab regime each entry of the class-edge tables reaches, the a-priori bound
on torch's own float32 gradients, the guard-band helper."""
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


EDGE_IDS = ["%d-%d-%d" % s for s in ref.BWD_EDGES]


def _f32_module_grads(x, dy, w, act):
    """(dx, dW1, db1, dW2, db2) of torch's float32 nn.Sequential on the CPU"""
    din, dh, dout = x.shape[1], w[0].shape[0], w[2].shape[0]
    mod = torch.nn.Sequential(torch.nn.Linear(din, dh), torch.nn.ReLU() if act == "relu" else torch.nn.LeakyReLU(ref.SLOPE), torch.nn.Linear(dh, dout))
    with torch.no_grad():
        for p, v in zip((mod[0].weight, mod[0].bias, mod[2].weight, mod[2].bias), w):
            p.copy_(v)
    xr = x.clone().requires_grad_(True)
    return torch.autograd.grad(mod(xr), [xr, mod[0].weight, mod[0].bias, mod[2].weight, mod[2].bias], dy)


@pytest.mark.parametrize("i", range(len(ref.BWD_EDGES)), ids=EDGE_IDS)
def test_closed_form_equals_autograd_in_float64_at_the_class_edges(i):
    test_closed_form_equals_autograd_in_float64((*ref.BWD_EDGES[i], ref.edge_act(i)))


def test_class_edge_tables_name_the_kernels_they_say():
    """the dispatch of gshac_mlp2_act, restated: every group of CLASS_EDGES lands in its kernel, and the backward's row counts in their slab regime"""
    from gauspcc_amd.mlp import slab_rows

    def kernel(din, dh, dout):
        if (din, dh, dout) == (96, 100, 175):
            return "exact"
        if din <= 192 and dh <= 40 and dout <= 32:
            return "<192,40,32>"
        if din <= 48 and dh <= 100 and dout <= 240:
            return "<48,100,240>"
        return "wide" if din <= 608 and dh <= 100 and dout <= 176 else "plain"

    assert [kernel(*s) for s in ref.CLASS_EDGES] == ref.EDGE_KERNELS
    assert [kernel(*s) for s in ref.LOOP_SHAPES] == ["<192,40,32>", "<48,100,240>"]
    assert [kernel(*s) for s in ref.BITWISE_EDGES] == ["<48,100,240>", "<192,40,32>", "plain", "<192,40,32>"]
    assert [kernel(*s) for s in ref.GUARDED_EDGES] == ["<48,100,240>", "<192,40,32>", "wide", "plain", "<192,40,32>"]
    assert set(ref.BITWISE_EDGES + ref.GUARDED_EDGES) <= set(ref.BWD_EDGES)
    assert -(-ref.LOOP_ROWS // 16) > 256 * 8                 # more 16-row tiles than 256 workgroups of eight waves take in one trip
    for s in ref.CLASS_EDGES + [(768, 256, 5)]:
        assert 16 * (s[0] + s[1]) * 4 <= 64 * 1024 and slab_rows(1, *s) == 128
        for n in ref.row_counts(128):
            assert slab_rows(n, *s) == 128
    assert [16 * (s[0] + s[1]) * 4 for s in ref.CLASS_EDGES[-4:-1]] == [64 * 1024] * 3
    for s in ref.OVER_THE_LIMIT:
        assert slab_rows(1, *s) == 0 and slab_rows(389, *s) == 0
    for s, n, slab in ref.GROWN_SLAB:
        small = 32768 if kernel(*s) == "plain" else 65536
        assert slab_rows(small, *s) == 128 and slab_rows(small + 1, *s) == 144 and slab_rows(n, *s) == slab and (slab > 128) == (n > small)
    assert [kernel(*s) for s, _, slab in ref.GROWN_SLAB if slab > 128] == ["<192,40,32>", "<48,100,240>", "plain"]


def test_guard_band_helper_sees_a_word_written_on_either_side():
    from tests.gpu_helpers import GUARD_WORDS, guarded, guards_intact

    for shape in ((17, 3), (5,), (2, 3, 1)):
        t = torch.randn(*shape)
        v = guarded(t, device="cpu").requires_grad_(True)
        assert torch.equal(v.detach(), t) and v.is_contiguous() and v.data_ptr() % 16 == 0 and guards_intact(v)
        assert v.storage_offset() * 4 >= 1024 and (v._base.numel() - v.storage_offset() - v.numel()) * 4 >= 1024 and GUARD_WORDS * 4 == 1024
        assert torch.nn.Parameter(v.detach()).data_ptr() == v.data_ptr()
        for at in (0, v.storage_offset() - 1, v.storage_offset() + v.numel(), v._base.numel() - 1):
            saved = v._base[at].clone()
            v._base[at] = 0.0
            assert not guards_intact(v)
            v._base[at] = saved
        assert guards_intact(v)


def test_fixture_rule_drops_under_five_percent_of_rows_at_the_class_edges():
    for i, (din, dh, dout) in enumerate(ref.BWD_EDGES):
        for n in ref.row_counts(128):
            x, dy, _, dropped = ref.fixture(din, dh, dout, n, seed=ref.edge_seed(i))
            assert x.shape == (n, din) and dy.shape == (n, dout)
            assert dropped < 0.05, (din, dh, dout, n, dropped)
    for j, ((din, dh, dout), n, _) in enumerate(ref.GROWN_SLAB):
        assert ref.fixture(din, dh, dout, n, seed=ref.grown_seed(j))[3] < 0.05


@pytest.mark.parametrize("i", range(len(ref.BWD_EDGES) + len(ref.GROWN_SLAB)), ids=EDGE_IDS + ["%d-%d-%d-n%d" % (*s, n) for s, n, _ in ref.GROWN_SLAB])
def test_torch_float32_gradients_satisfy_the_a_priori_bound(i):
    """gamma_bound is what the GPU test holds a gradient of fewer than SMALL elements to: torch's own float32 gradients must pass it in every
    such case (here all five gradients are checked, the small ones and the rest)."""
    j = i - len(ref.BWD_EDGES)
    (din, dh, dout), rows = (ref.BWD_EDGES[i], ref.row_counts(128)) if j < 0 else (ref.GROWN_SLAB[j][0], [ref.GROWN_SLAB[j][1]])
    act, seed = ref.edge_act(i if j < 0 else j), ref.edge_seed(i) if j < 0 else ref.grown_seed(j)
    small_cases = 0
    for n in rows:
        x, dy, w, _ = ref.fixture(din, dh, dout, n, seed=seed)
        a64 = (x.double(), *(t.double() for t in w), dy.double(), act)
        want, bound = ref.closed_form_grads(*a64), ref.gamma_bound(*a64)
        for name, g, t, b in zip(("dx", "dW1", "db1", "dW2", "db2"), _f32_module_grads(x, dy, w, act), want, bound):
            assert g.shape == t.shape == b.shape
            small_cases += g.numel() < ref.SMALL
            assert bool(((g.double() - t).abs() <= b).all()), (n, name, float(((g.double() - t).abs() - b).max()))
    assert small_cases or min(dh, dout) >= ref.SMALL


def test_fixture_rule_drops_under_five_percent_of_rows():
    from gauspcc_amd.mlp import slab_rows

    for s, (din, dh, dout, _) in enumerate(ref.SHAPES):
        for n in ref.row_counts(slab_rows(1, din, dh, dout)):
            x, dy, _, dropped = ref.fixture(din, dh, dout, n, seed=10 * s)
            assert x.shape == (n, din) and dy.shape == (n, dout)
            assert dropped < 0.05, (din, dh, dout, n, dropped)
