"""The float64 restatement of the entropy rate models and their analytic gradients (tests/rate_ref.py), checked on the CPU before any
GPU test relies on them: against gradcheck away from the kinks, against autograd of the same formula in float64, and against the
reference's own float32 values and autograd gradients (tests/golden/rate.npz)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import rate_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rate.npz")


class _Rate64(torch.autograd.Function):
    """rate64 forward, grads64 backward: what gradcheck differentiates numerically"""
    @staticmethod
    def forward(ctx, k, q_kind, x, Q, *ops):
        means, scales, probs = list(ops[:k]), list(ops[k:2 * k]), list(ops[2 * k:]) or None
        ctx.k, ctx.args = k, (x, means, scales, probs, Q)
        return rate_ref.rate64(x, means, scales, probs, Q)[0]

    @staticmethod
    def backward(ctx, g):
        x, means, scales, probs, Q = ctx.args
        d = rate_ref.grads64(g, x, means, scales, probs, Q)
        return (None, None, d["x"], d["Q"], *d["mean"], *d["scale"], *d["prob"])


@pytest.mark.parametrize("k,q_kind", [(1, "row"), (1, "full"), (1, "one"), (2, "row"), (3, "full")])
def test_analytic_gradients_gradcheck(k, q_kind):
    x, means, scales, probs, Q = rate_ref.make_case(5, 4, k=k, seed=10 + k, q_kind="full" if q_kind == "one" else q_kind)
    if q_kind == "one":
        Q = torch.tensor(0.8)
    x = means[0] + scales[0] * torch.randn(x.shape, generator=torch.Generator().manual_seed(k))   # near the first mean: L well above 1e-6
    _, L = rate_ref.rate64(x, means, scales, probs, Q)
    assert float(L.min()) > 1e-4   # away from the 1e-6 floor; x inside the window (Q ~ 1: +-15000); scales far above 1e-9
    leaves = [t.double().requires_grad_(True) for t in [x, Q] + means + scales + (probs or [])]
    assert torch.autograd.gradcheck(lambda *a: _Rate64.apply(k, q_kind, *a), leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("k,lkl,floor", [(1, False, None), (2, False, None), (3, True, None), (1, False, 1e-9)])
def test_analytic_equals_autograd_float64(k, lkl, floor):
    x, means, scales, probs, Q = rate_ref.make_case(40, 7, k=k, seed=k, q_kind="row", saturate=True)
    Q = Q * torch.where(torch.arange(40) % 3 == 0, 1e-3, 1.0).view(40, 1)   # windows that cut into the data
    Q[::7] = 1e-12
    scales[0].view(-1)[::13] = 1e-12
    leaves = [t.double().requires_grad_(True) for t in [x, Q] + means + scales + (probs or [])]
    xd, Qd = leaves[0], leaves[1]
    md, sd, pd = leaves[2:2 + k], leaves[2 + k:2 + 2 * k], leaves[2 + 2 * k:] or None
    out = rate_ref.rate_torch(xd, md, sd, pd, Qd, x_mean=xd.mean().detach() + 3.0, q_floor=floor, return_lkl=lkl)
    g = torch.randn(out.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    (out * g).sum().backward()
    ref, _ = rate_ref.rate64(xd, md, sd, pd, Qd, xd.mean() + 3.0, floor, lkl)
    assert torch.allclose(out.detach(), ref, rtol=0, atol=1e-8)   # the two groupings of (v - m) / (s sqrt 2) near the floor
    d = rate_ref.grads64(g, xd, md, sd, pd, Qd, xd.mean() + 3.0, floor, lkl)
    pairs = [(d["x"], xd), (d["Q"], Qd)] + list(zip(d["mean"] + d["scale"] + d["prob"], md + sd + (pd or [])))
    for a, leaf in pairs:
        scale = float(leaf.grad.abs().max()) + 1e-30
        assert torch.allclose(a, leaf.grad, rtol=0, atol=1e-8 * scale)
    assert (d["x"] == 0).any() and (d["Q"] == 0).any()   # the window and the Q floor did cut


def golden_tolerance(c, L, d_el, near):
    """Per-element bound on the reference's float32 gradient error: the likelihood's error (L_MARGIN) relative to L, scaled by the
    gradient, plus a floor; near a kink either side is right, so the whole value.  Reduced operands sum their elements' bounds."""
    tol = (rate_ref.rel_error32(c, L) + 1e-4) * d_el.abs() + 1e-5 * float(d_el.abs().max())
    return torch.where(near, tol + 2 * d_el.abs(), tol)


def _pairs(d, c):
    out = [("x", d["x"], c["g_x"])]
    for name, dk, ck in (("mean", "mean", "g_mean"), ("scale", "scale", "g_scale"), ("prob", "prob", "g_prob")):
        out += [(f"{name}{i}", a, r) for i, (a, r) in enumerate(zip(d[dk] or [], c[ck] or []))]
    if d["Q"] is not None:
        out.append(("Q", d["Q"], c["g_Q"]))
    return out


@pytest.mark.parametrize("key", sorted(rate_ref.GOLDEN_CASES))
def test_restatement_matches_reference_golden(key):
    c = rate_ref.golden_case(np.load(GOLDEN), key)
    args = lambda c: (c["x"], c["means"], c["scales"], c["probs"], c["Q"], c["x_mean"], c["q_floor"], c["lkl"])   # noqa: E731
    out, L = rate_ref.rate64(*args(c))
    near = rate_ref.near_kinks(c)
    away = ~near
    # outputs: bits error = likelihood error / (L ln 2); the likelihood's own error is absolute
    rel = rate_ref.rel_error32(c, L)
    tol_out = (rel * torch.clamp(L, min=rate_ref.LOW) if c["lkl"] else rel / math.log(2)) + 1e-6
    assert ((out - c["out"].double()).abs() <= tol_out)[away].all(), key
    # the elements on the 1e-6 floor are the reference's, except within the stated margin of it
    floor_bits = float(c["out"].max()) if not c["lkl"] else 1e-6
    floor_ref = (c["out"].double() - (np.float32(1e-6) if c["lkl"] else floor_bits)).abs() <= (0 if c["lkl"] else 1e-5)
    assert (c["lkl"] or abs(floor_bits - (-math.log2(1e-6))) < 1e-5) and floor_ref.any()
    assert torch.equal((L < rate_ref.LOW)[away], floor_ref[away]), key
    d = rate_ref.grads64(c["w"], *args(c))
    d_el = rate_ref.grads64(c["w"], *args(rate_ref.expanded(c)))
    for (name, a, ref), (_, a_el, _) in zip(_pairs(d, c), _pairs(d_el, c)):
        tol = golden_tolerance(c, L, a_el, near).sum_to_size(ref.shape)
        err = (a - ref.double()).abs()
        assert (err <= tol).all(), (key, name, float((err - tol).max()))
        if a.shape == L.shape:   # on the floor (away from its margin) the gradient is exactly 0, in both
            on = ~rate_ref.near_kinks(c, flat=False) & (L < rate_ref.LOW)
            assert on.any() and (a[on] == 0).all() and (ref[on] == 0).all(), (key, name)


def test_golden_covers_the_kinks():
    g = np.load(GOLDEN)
    c = rate_ref.golden_case(g, "cat_floor")
    assert (c["Q"] < 1e-9).any() and (c["g_Q"][c["Q"] < 1e-9] == 0).all()
    for key in rate_ref.GOLDEN_CASES:
        c = rate_ref.golden_case(g, key)
        assert (c["scales"][0] < 1e-9).any() and (c["g_scale"][0][c["scales"][0] < 1e-9] == 0).all(), key
        q = torch.as_tensor(c["Q"], dtype=torch.float64)
        if c["q_floor"] is not None:
            q = torch.clamp(q, min=c["q_floor"])
        xm = c["x"].double().mean() if c["x_mean"] is None else c["x_mean"].double()
        outside = (c["x"].double() - xm).abs() > 15000 * q
        assert outside.any() and (c["g_x"][outside] == 0).all(), key
