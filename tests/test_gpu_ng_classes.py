"""The neural-Gaussian kernels (csrc/neural_gaussians.hip) at every emission class, wave count and strip count: tests/ng_train_ref.py's NG_EDGES --
n_offsets from 1 to the limit of 64, through every NIT of k_ng_emit, the eight-wave | four-wave edge, the lane kernels and a full strip table of
k_ngb_wgrad -- at 1, 16, 17 and 333 anchors.  The criteria are those of tests/test_gpu_ng_train.py: keep flags equal to the float64 restatement's
and values within 2e-5 (5e-5 for rot); in HAC's order the training forward equal to the inference forward bit for bit; gradients within 5e-5 of
float64 in the norm of each tensor.  tests/test_ng_train_cpu.py checks the conditions on the inputs (anchors left out, candidates kept)."""
import ctypes as C
import types

import pytest
import torch

from tests import ng_train_ref as ref
from tests.gpu_helpers import guarded, guards_intact
from tests.ng_train_ref import ng_train_ref
from tests.test_gpu_ng_train import DEV, _pc, _pc_params, _run, _upstream

pytestmark = pytest.mark.gpu

NAMES = ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity")
TOLS = (2e-5,) * 4 + (5e-5, 2e-5)
GRAD_TOL = 5e-5


def ident(case):
    return "F%d-K%d-%s" % (case[0], case[1], "bank" if case[2] else "nobank")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def _close_to_restatement(out, want, tag):
    for name, a, b, tol in zip(NAMES, out, want, TOLS):
        assert a.shape == b.shape and a.dtype == torch.float32, (tag, name)
        assert not a.isnan().any(), (tag, name)
        assert torch.allclose(a.double(), b, atol=tol, rtol=tol), (tag, name, (a.double() - b).abs().max().item())


def _decoded_model(ts, ps, F, K, bank):
    """a decoded model holding float32 copies of the fixture's tensors, and its camera"""
    pc = _pc(ps, bank)
    pc.decoded_version, pc.feat_dim, pc.n_offsets = True, F, K
    pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc.get_mask = (t.float() for t in ts[:5])
    return pc, types.SimpleNamespace(camera_center=ts[5].float())


def _training_forward_matches(F, K, bank, n):
    for mask_after in (False, True):
        ts, ps, _ = ref.edge_case(n, F, K, bank, mask_after, DEV)
        want = ng_train_ref(*ts, ps, mask_after)
        out, _ = _run(ts, _pc(ps, bank), mask_after)
        tag = (n, mask_after)
        assert out[6].dtype == torch.bool and torch.equal(out[6], want[6]) and out[6].any(), tag
        assert out[5].shape == (n * K, 1), tag
        _close_to_restatement(out[:6], want[:6], tag)


def _training_equals_inference(F, K, bank, n):
    """HAC's order: the <F, false, false> instantiations compute what the training ones do, bit for bit"""
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians, neural_gaussians_train

    ts, ps, _ = ref.edge_case(n, F, K, bank, False, DEV)
    pc, cam = _decoded_model(ts, ps, F, K, bank)
    want = generate_neural_gaussians(cam, pc, None)[:5]
    got = neural_gaussians_train(pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc.get_mask, cam.camera_center, pc)
    assert int(got[6].sum()) == want[0].shape[0] > 0, n
    for name, a, b in zip(NAMES, got[:5], want):
        assert a.shape == b.shape and torch.equal(a, b), (n, name)


@pytest.mark.parametrize("case", ref.NG_EDGES, ids=ident)
def test_training_forward_matches_restatement(case):
    for n in ref.EDGE_ROWS:
        _training_forward_matches(*case, n)


@pytest.mark.parametrize("case", ref.NG_EDGES, ids=ident)
def test_training_forward_equals_inference_forward(case):
    for n in ref.EDGE_ROWS:
        _training_equals_inference(*case, n)


@pytest.mark.parametrize("case", ref.NG_EDGES, ids=ident)
def test_inference_reads_the_visible_rows_only(case):
    """The ROWS instantiations: the model's tensors hold the fixture's anchors at the odd rows and NaN everywhere else, visible_mask names the odd rows."""
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians

    F, K, bank = case
    for n in ref.EDGE_ROWS:
        ts, ps, _ = ref.edge_case(n, F, K, bank, False, DEV)
        want = ng_train_ref(*ts, ps, False)
        pc, cam = _decoded_model(ts, ps, F, K, bank)
        visible = torch.zeros(2 * n + 3, dtype=torch.bool, device=DEV)
        visible[1:2 * n:2] = True
        for name in ("get_anchor", "_anchor_feat", "_offset", "get_scaling", "get_mask"):
            real = getattr(pc, name)
            held = torch.full((2 * n + 3, *real.shape[1:]), float("nan"), device=DEV)
            held[visible] = real
            setattr(pc, name, held)
        out = generate_neural_gaussians(cam, pc, visible)[:5]
        assert out[0].shape[0] == int(want[6].sum()) > 0, n
        _close_to_restatement(out, want[:5], n)


def _gradients(ts, ps, bank, mask_after, repeat=False):
    pc = _pc(ps, bank)
    out, _ = _run(ts, pc, mask_after)
    R = _upstream(out, 11)
    _, got = _run(ts, pc, mask_after, R)
    if repeat:
        for _ in range(2):
            _, again = _run(ts, pc, mask_after, R)
            assert all(torch.equal(a, b) for a, b in zip(got, again))
    ins = [t.clone().requires_grad_(True) for t in ts[:5]]
    pr = [None if p is None else p.clone().requires_grad_(True) for p in ps]
    want = ng_train_ref(*ins, ts[5], pr, mask_after)
    sum((o * r.double()).sum() for o, r in zip(want[:6], R)).backward()
    return got, [t.grad for t in ins] + [p.grad for p in pr if p is not None]


@pytest.mark.parametrize("case", [c for c in ref.NG_EDGES if c[1] in ref.GRAD_K], ids=ident)
def test_gradients_match_float64(case):
    F, K, bank = case
    worst, bad = 0.0, []
    for n in ref.EDGE_ROWS:
        for mask_after in (False, True):
            ts, ps, _ = ref.edge_case(n, F, K, bank, mask_after, DEV)
            got, want = _gradients(ts, ps, bank, mask_after, repeat=case in ref.BITWISE_EDGES and n == 333)
            assert len(got) == len(want) == 5 + (16 if bank else 12)
            for i, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape, i
                rel = ((a.double() - b).norm() / max(b.norm().item(), 1e-30)).item()
                worst = max(worst, rel)
                if not rel < GRAD_TOL:
                    bad.append((n, mask_after, i, rel))
    print(f"{ident(case)}: worst relative gradient error {worst:.3e} (bound {GRAD_TOL:.0e})")
    assert not bad, bad


@pytest.mark.parametrize("case", ref.LOOP_EDGES, ids=ident)
def test_second_trip_of_the_tile_loops(case):
    _training_forward_matches(*case, ref.LOOP_ROWS)
    _training_equals_inference(*case, ref.LOOP_ROWS)


def test_limits_are_refused_by_the_wrapper_and_by_every_entry_point():
    from gauspcc_amd import _lib, runtime
    from gauspcc_amd._lib import GpccError
    from gauspcc_amd.neural_gaussians import neural_gaussians_train

    n = 4
    g = torch.Generator().manual_seed(2)
    cam = torch.tensor([0.3, -4.0, 1.1], device=DEV)
    # (F, K, bank): no offsets, one more than 64, a feature width without kernels, a bank over a width that is no multiple of 4
    for F, K, bank in ((32, 0, False), (32, 65, False), (48, 5, False), (50, 5, True)):
        pc = _pc(ref.random_params(50 if bank else 32, 5, bank, g), bank)
        ins = [torch.zeros(n, 3, device=DEV), torch.zeros(n, F, device=DEV), torch.zeros(n, K, 3, device=DEV), torch.ones(n, 6, device=DEV),
               torch.ones(n, K, 1, device=DEV)]
        with pytest.raises(GpccError):
            neural_gaussians_train(*ins, cam, pc)
        # the C entry points: every pointer names one zeroed buffer larger than any tensor of these sizes; the check comes before any use
        buf = torch.zeros(1 << 18, device=DEV)
        p = buf.data_ptr()
        mlp = (C.c_void_p * 16)(*([p if bank else None] * 4 + [p] * 12))
        L, ctx, st = _lib.lib(), runtime.context(DEV), runtime.stream_ptr(DEV)
        ws = runtime.Workspace(DEV)
        count, pos = C.c_int64(), C.c_void_p()
        with pytest.raises(GpccError):
            _lib.check(L.gsnn_generate(ctx, n, None, F, K, *[p] * 6, mlp, *[p] * 5, C.byref(count), st))
        with pytest.raises(GpccError):
            _lib.check(L.gsnn_forward_train(ctx, n, F, K, *[p] * 6, mlp, 0, *[p] * 7, ws.fn(), None, C.byref(pos), C.byref(count), st))
        with pytest.raises(GpccError):
            _lib.check(L.gsnn_backward(ctx, n, F, K, *[p] * 6, mlp, 0, *[p] * 12, mlp, ws.fn(), None, st))
        torch.cuda.synchronize()
        assert not ws.buffers and count.value == 0 and not pos.value and not buf.any()


@pytest.mark.parametrize("case", ref.GUARDED_EDGES, ids=ident)
def test_inputs_inside_guard_bands(case):
    """The five inputs, the camera centre and every MLP parameter each sit in a NaN-filled buffer: outputs and gradients are the plain call's bit for
    bit (no operand came from outside its tensor) and the guard words are NaN afterwards (nothing was written there)."""
    from gauspcc_amd.neural_gaussians import neural_gaussians_train

    F, K, bank = case
    for mask_after in (False, True):
        ts, ps, _ = ref.edge_case(17, F, K, bank, mask_after, DEV)

        def run(place):
            pc = _pc(ps, bank)
            held = []
            for seq in ([pc.get_featurebank_mlp] if bank else []) + [pc.get_opacity_mlp, pc.get_cov_mlp, pc.get_color_mlp]:
                for lin in (seq[0], seq[2]):
                    held += [place(lin.weight), place(lin.bias)]
                    lin.weight, lin.bias = torch.nn.Parameter(held[-2]), torch.nn.Parameter(held[-1])
                    assert lin.weight.data_ptr() == held[-2].data_ptr() and lin.bias.data_ptr() == held[-1].data_ptr()
            ins = [place(t.float()).requires_grad_(True) for t in ts[:5]]
            cam = place(ts[5].float())
            out = neural_gaussians_train(*ins, cam, pc, mask_after_opacity=mask_after)
            R = _upstream(out, 11)
            sum((o * r).sum() for o, r in zip(out[:6], R)).backward()
            return held + ins + [cam], [o.detach() for o in out] + [t.grad for t in ins] + [p.grad for p in _pc_params(pc, bank)]

        _, want = run(lambda t: t.detach().clone())
        held, got = run(guarded)
        torch.cuda.synchronize()
        assert len(got) == len(want) == 7 + 5 + (16 if bank else 12) and want[6].any()
        assert not any(bool(t.isnan().any()) for t in want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (mask_after, i)
        assert all(guards_intact(t) for t in held), mask_after
