"""CPU checks of tests/ng_train_ref.py, the float64 restatement the GPU tests of the neural-Gaussian training path compare against."""
import pytest
import torch

from tests import ng_train_ref as ref
from tests.ng_train_ref import ng_train_ref, normalize, random_params, ste_masks


def _inputs(n, F, K, bank, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.float64
    anchor = torch.rand(n, 3, generator=g, dtype=d) * 4 - 2
    feat = torch.randn(n, F, generator=g, dtype=d) * 0.8
    off = torch.randn(n, K, 3, generator=g, dtype=d) * 0.3
    sc = torch.exp(torch.randn(n, 6, generator=g, dtype=d) * 0.4 - 2.5)
    masks = ste_masks(n, K, g)
    cam = torch.tensor([0.3, -4.0, 1.1], dtype=d)
    return anchor, feat, off, sc, masks, cam, random_params(F, K, bank, g)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("mask_after", [False, True])
def test_gradcheck(bank, mask_after):
    F, K = 8, 3
    anchor, feat, off, sc, masks, cam, params = _inputs(5, F, K, bank, seed=3 + bank + 2 * mask_after)
    # a mask at exactly 0 is where HAC's keep test flips under a finite difference; gradcheck takes the (b - s) + s values near 1 and 0.5
    masks = torch.where(masks == 0, torch.full_like(masks, 0.5), masks)
    ts = [anchor, feat, off, sc, masks] + [p for p in params if p is not None]
    for t in ts:
        t.requires_grad_(True)
    where = [i for i, p in enumerate(params) if p is not None]

    def fn(a, f, o, s, m, *ps):
        full = [None] * 16
        for i, p in zip(where, ps):
            full[i] = p
        out = ng_train_ref(a, f, o, s, m, cam, full, mask_after)
        return out[:6]

    # keep is piecewise constant: the random inputs stay away from tanh(z) = 0
    assert torch.autograd.gradcheck(fn, ts, eps=1e-6, atol=1e-6, rtol=1e-4)


def test_masks_are_the_straight_through_form():
    m = ste_masks(200, 4, torch.Generator().manual_seed(0))
    assert (m - m.round()).abs().max() < 1e-6 and 0 < m.sum() < m.numel()


def test_rotation_eps_branch():
    q = torch.tensor([[1e-14, 0.0, 0.0, 0.0], [3.0, 0.0, 4.0, 0.0]], dtype=torch.float64, requires_grad=True)
    r = normalize(q)
    assert torch.allclose(r[0], torch.tensor([1e-2, 0, 0, 0], dtype=torch.float64))
    assert torch.allclose(r[1], torch.tensor([0.6, 0, 0.8, 0], dtype=torch.float64))
    g = torch.randn(2, 4, dtype=torch.float64)
    (r * g).sum().backward()
    assert torch.allclose(q.grad[0], g[0] / 1e-12)            # below eps the denominator is a constant
    assert torch.allclose(q.grad[1], (g[1] - r[1] * (r[1] @ g[1])) / 5.0)
    assert torch.equal(normalize(q.detach()), torch.nn.functional.normalize(q.detach(), dim=-1))


def edge_input_failures(F, K, bank, seed=None):
    """the conditions on the inputs of tests/test_gpu_ng_classes.py that case (F, K, bank) misses with `seed` (default: its own)"""
    bad = []
    for n in ref.EDGE_ROWS + ([ref.LOOP_ROWS] if (F, K, bank) in ref.LOOP_EDGES else []):
        for mask_after in (False, True):
            ts, ps, dropped = ref.edge_case(n, F, K, bank, mask_after, "cpu", seed)
            assert [t.shape[0] for t in ts[:5]] == [n] * 5
            kept = ng_train_ref(*ts, ps, mask_after)[6]
            share = float(kept.double().mean())
            if dropped >= 0.05:
                bad.append((n, mask_after, "dropped", dropped))
            if n >= 333 and not 0.1 <= share <= 0.9:
                bad.append((n, mask_after, "kept share", share))
            if not kept.any():
                bad.append((n, mask_after, "nothing kept"))
    return bad


@pytest.mark.parametrize("F,K,bank", ref.NG_EDGES + [c for c in ref.GUARDED_EDGES if c not in ref.NG_EDGES])
def test_edge_inputs_meet_their_conditions(F, K, bank):
    """under 5 % of the anchors left out, 10 % to 90 % of the candidates kept, at least one Gaussian at 1, 16 and 17 anchors"""
    assert not edge_input_failures(F, K, bank)


def test_edge_tables():
    assert len(ref.NG_EDGES) == 25 and len(set(ref.NG_EDGES)) == 25 and set(ref.EDGE_SEED_J) <= set(ref.NG_EDGES)
    assert set(ref.LOOP_EDGES + ref.BITWISE_EDGES) <= set(ref.NG_EDGES) and set(ref.GRAD_K) <= set(ref.EDGE_K)
    assert sorted({(16 * K + 63) // 64 for K in ref.EDGE_K if K <= 16}) == [1, 2, 3, 4]         # every NIT of k_ng_emit
    strips = lambda F, K, bank: 3 + sum(-(-m // 64) for m in (K, 7 * K, 3 * K)) + (2 if bank else 0)   # noqa: E731  (F <= 64: one strip per first layer)
    assert strips(32, 64, True) == 16 and max(strips(*c) for c in ref.NG_EDGES) == 16           # NG_MAX_STRIPS, reached and not passed


def _hand_case():
    """two anchors, K = 2; the opacity head's output bias decides the signs: tanh(z) = +, - for each anchor"""
    F, K = 8, 2
    params = random_params(F, K, False, torch.Generator().manual_seed(1))
    params[6] = torch.zeros_like(params[6])
    params[7] = torch.tensor([2.0, -2.0], dtype=torch.float64)
    n = 2
    anchor = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], dtype=torch.float64)
    feat = torch.zeros(n, F, dtype=torch.float64)
    off = torch.zeros(n, K, 3, dtype=torch.float64)
    sc = torch.ones(n, 6, dtype=torch.float64)
    cam = torch.zeros(3, dtype=torch.float64)
    return anchor, feat, off, sc, cam, params


def test_keep_sets_hand_made():
    anchor, feat, off, sc, cam, params = _hand_case()
    masks = torch.tensor([[[1.0], [1.0]], [[0.0], [1.0]]], dtype=torch.float64)
    out = ng_train_ref(anchor, feat, off, sc, masks, cam, params, mask_after=False)
    assert out[6].tolist() == [True, False, False, False]       # HAC: the masked positive candidate is dropped
    out = ng_train_ref(anchor, feat, off, sc, masks, cam, params, mask_after=True)
    assert out[6].tolist() == [True, False, True, False]        # HAC++: kept on tanh > 0, its opacity and scaling then masked
    assert out[2][1].item() == 0.0 and torch.all(out[3][1] == 0.0)
    assert out[5].shape == (4, 1)
    masks = torch.zeros(2, 2, 1, dtype=torch.float64)
    assert ng_train_ref(anchor, feat, off, sc, masks, cam, params)[6].sum().item() == 0    # every anchor fully masked: nothing kept
