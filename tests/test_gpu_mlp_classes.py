"""gshac_mlp2_act / gshac_mlp2_backward at the edges of every compile-time class (tests/mlp_ref.py: CLASS_EDGES and the tables after it): layers
narrower than their class in each size, one step outside every class, the size limit, the second trip of the forward's persistent loop and the
backward's grown slabs.  The criteria are those of tests/test_gpu_mlp_train.py: the forward is the oracle's chain bit for bit; a gradient's
e_dev = max |device - float64| must not exceed 4 x e_t32 of the float32 nn.Sequential on the same GPU.  That maximum is a fair scale only over enough
elements (the smallest gradient held to it there has 30): a gradient of fewer than mlp_ref.SMALL elements is held elementwise to the a-priori bound
mlp_ref.gamma_bound instead, which tests/test_mlp_ref_cpu.py shows torch's own float32 gradients to satisfy in every one of these cases."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as ref  # noqa: E402

from tests.gpu_helpers import guarded, guards_intact  # noqa: E402
from tests.test_gpu_mlp_train import DEV, FACTOR, NAMES, _criterion, _grads, _ours, _torch_module  # noqa: E402

pytestmark = pytest.mark.gpu
ACTS = (("relu", 0.0), ("leaky_relu", ref.SLOPE))


def ident(shape):
    return "%d-%d-%d" % tuple(shape)


def _forward_is_the_oracles(orc, din, dh, dout, rows, seed):
    from gauspcc_amd.mlp import mlp2

    w = ref.weights(din, dh, dout, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(max(rows), din, generator=g)
    wd, xd = [t.to(DEV) for t in w], x.to(DEV)
    for n in rows:
        for act, slope in ACTS:
            want = orc.mlp2(x[:n].numpy(), *(t.numpy() for t in w), slope=slope)
            with torch.no_grad():
                y = mlp2(xd[:n], *wd, act=act, slope=slope)
            assert y.shape == (n, dout) and np.array_equal(y.cpu().numpy(), want), (n, act)


@pytest.mark.parametrize("i", range(len(ref.CLASS_EDGES)), ids=[f"{ident(s)}-{k}" for s, k in zip(ref.CLASS_EDGES, ref.EDGE_KERNELS)])
def test_forward_is_the_oracles_chain_bit_for_bit(i, orc):
    _forward_is_the_oracles(orc, *ref.CLASS_EDGES[i], ref.EDGE_ROWS, seed=ref.edge_seed(i))


@pytest.mark.parametrize("shape", ref.LOOP_SHAPES, ids=ident)
def test_forward_second_trip_of_the_persistent_loop(shape, orc):
    _forward_is_the_oracles(orc, *shape, [ref.LOOP_ROWS], seed=7)


@pytest.mark.parametrize("shape", ref.OVER_THE_LIMIT, ids=ident)
def test_one_step_over_the_size_limit_is_refused(shape):
    from gauspcc_amd import _lib, runtime
    from gauspcc_amd._lib import GpccError
    from gauspcc_amd.mlp import mlp2, slab_rows

    din, dh, dout = shape
    n = 17
    w = [t.to(DEV) for t in ref.weights(din, dh, dout, 3)]
    x = torch.randn(n, din, device=DEV)
    assert slab_rows(n, din, dh, dout) == 0 and slab_rows(n, din - (din > 1), dh - (dh > 1), dout) == 128
    with pytest.raises(GpccError):
        mlp2(x, *w)
    with pytest.raises(GpccError):      # with autograd: refused in the forward, before anything is saved
        mlp2(x.clone().requires_grad_(True), *w)
    dy = torch.randn(n, dout, device=DEV)
    grads = [torch.full_like(t, 7.0) for t in w]
    ws = runtime.Workspace(DEV)
    with pytest.raises(GpccError):
        _lib.check(_lib.lib().gshac_mlp2_backward(runtime.context(DEV), x.data_ptr(), *(t.data_ptr() for t in w), n, din, dh, dout, 0, 0.0, dy.data_ptr(), None,
                                                  *(g.data_ptr() for g in grads), ws.fn(), None, runtime.stream_ptr(DEV)))
    torch.cuda.synchronize()
    assert not ws.buffers and all(bool((g == 7.0).all()) for g in grads)        # nothing was asked for, nothing written


@functools.lru_cache(maxsize=None)
def _case(din, dh, dout, act, n, seed):
    """Inputs, the float64 gradients and the a-priori bounds (computed once, on the CPU), and the float32 nn.Sequential's gradients on the GPU."""
    x, dy, w, _ = ref.fixture(din, dh, dout, n, seed=seed)
    a64 = (x.double(), *(t.double() for t in w), dy.double(), act)
    _, g32 = _grads(_torch_module(din, dh, dout, act, w), x, dy)
    return dict(x=x, dy=dy, w=w, g64=ref.closed_form_grads(*a64), bound=ref.gamma_bound(*a64), g32=[g.cpu() for g in g32])


def _check_gradients(din, dh, dout, act, rows, seed):
    bad = []
    for n in rows:
        d = _case(din, dh, dout, act, n, seed)
        _, g = _grads(_ours(din, dh, dout, act, d["w"]), d["x"], d["dy"])
        for name, dev, t32, want, bound in zip(NAMES, g, d["g32"], d["g64"], d["bound"]):
            assert dev.shape == want.shape
            ok, info = _criterion(f"{din}-{dh}-{dout} n {n} {name}", dev, t32, want)
            if want.numel() < ref.SMALL:
                over = float(((dev.double().cpu() - want).abs() / bound.clamp_min(1e-300)).max())
                print(f"    {want.numel()} elements: |dev - f64| / gamma_bound at most {over:.3e}")
                ok, info = over <= 1.0, info + ("gamma_bound", over)
            if not ok:
                bad.append(info)
    assert not bad, (FACTOR, bad)


@pytest.mark.parametrize("i", range(len(ref.BWD_EDGES)), ids=[ident(s) for s in ref.BWD_EDGES])
def test_gradients_match_float64_restatement(i):
    from gauspcc_amd.mlp import slab_rows

    rows = ref.row_counts(128)
    assert all(slab_rows(n, *ref.BWD_EDGES[i]) == 128 for n in rows)
    _check_gradients(*ref.BWD_EDGES[i], ref.edge_act(i), rows, ref.edge_seed(i))


@pytest.mark.parametrize("j", range(len(ref.GROWN_SLAB)), ids=["%s-n%d-slab%d" % (ident(s), n, slab) for s, n, slab in ref.GROWN_SLAB])
def test_gradients_in_the_grown_slab_regime(j):
    from gauspcc_amd.mlp import slab_rows

    shape, n, slab = ref.GROWN_SLAB[j]
    assert slab_rows(n, *shape) == slab and slab_rows(389, *shape) == 128
    _check_gradients(*shape, ref.edge_act(j), [n], ref.grown_seed(j))


def _bitwise_case(shape):
    i = ref.BWD_EDGES.index(shape)
    act = ref.edge_act(i)
    d = _case(*shape, act, 389, ref.edge_seed(i))
    return d, _ours(*shape, act, d["w"])


@pytest.mark.parametrize("shape", ref.BITWISE_EDGES, ids=ident)
def test_backward_is_bitwise_reproducible_also_on_a_side_stream(shape):
    d, m = _bitwise_case(shape)
    _, g0 = _grads(m, d["x"], d["dy"])
    for _ in range(2):
        _, g = _grads(m, d["x"], d["dy"])
        assert all(torch.equal(a, b) for a, b in zip(g, g0))
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _, g = _grads(m, d["x"], d["dy"])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(g, g0))


@pytest.mark.parametrize("shape", ref.BITWISE_EDGES, ids=ident)
def test_parameter_gradients_do_not_depend_on_dx(shape):
    d, m = _bitwise_case(shape)
    _, g = _grads(m, d["x"], d["dy"])
    _, h = _grads(m, d["x"], d["dy"], with_dx=False)
    assert all(torch.equal(a, b) for a, b in zip(g[1:], h[1:]))


@pytest.mark.parametrize("shape", ref.GUARDED_EDGES, ids=ident)
def test_inputs_inside_guard_bands(shape):
    """x, the four parameters and dy each sit in a NaN-filled buffer: the results are the plain call's bit for bit (no operand came from outside
    its tensor) and the guard words are NaN afterwards (nothing was written there)."""
    from gauspcc_amd.mlp import mlp2

    din, dh, dout = shape
    i = ref.BWD_EDGES.index(shape)
    act, slope = ACTS[i % 2]
    assert act == ref.edge_act(i)
    x, dy, w, _ = ref.fixture(din, dh, dout, 17, seed=ref.edge_seed(i))

    def run(place):
        ts = [place(t.to(DEV)) for t in (x, *w, dy)]
        leaves = [t.requires_grad_(True) for t in ts[:5]]
        y = mlp2(*leaves, act=act, slope=slope)
        with torch.no_grad():
            y_plain = mlp2(*ts[:5], act=act, slope=slope)
        return ts, [y.detach(), y_plain, *torch.autograd.grad(y, leaves, ts[5])]

    _, want = run(lambda t: t.clone())
    ts, got = run(guarded)
    torch.cuda.synchronize()
    assert not any(bool(t.isnan().any()) for t in want)
    for name, a, b in zip(("y", "y without autograd") + NAMES, got, want):
        assert torch.equal(a, b), name
    assert all(guards_intact(t) for t in ts)
