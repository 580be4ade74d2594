"""Restatements of the entropy rate models (utils/entropy_models.py: Entropy_gaussian, the mixtures, Low_bound) for the tests of
gauspcc_amd.entropy_models:

  rate64 / grads64   the formula and its analytic gradients in float64 (the yardstick the device is measured against)
  rate_torch         the same formula as a plain torch program, differentiated by autograd; in float32 it is the reference's own
                     arithmetic (used to calibrate tolerances), in float64 a cross-check of grads64
  RefEntropy*        torch modules that behave as the reference's do, including torch.distributions.Normal's argument validation and a
                     Low_bound backward that round-trips the likelihood and its gradient through host memory (timing baseline)

The model, per element: Q = max(Q, q_floor) when given; x' = clamp(x, x_mean - 15000 Q, x_mean + 15000 Q) with detached bounds;
s_i = max(scale_i, 1e-9); Phi_i(v) = 0.5 (1 + erf((v - mean_i) / (s_i sqrt 2))); L = sum_i prob_i |Phi_i(x' + Q/2) - Phi_i(x' - Q/2)|
(prob = 1 for one component); out = max(L, 1e-6) with return_lkl, else -log2 of it.
"""
import math

import numpy as np
import torch

LOW = 1e-6
SCALE_FLOOR = 1e-9


def _as(v, like):
    return v.to(like) if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=like.dtype, device=like.device)


def _window(x, Q, x_mean, q_floor):
    q = _as(Q, x)
    if q_floor is not None:
        q = torch.clamp(q, min=q_floor)
    xm = x.mean() if x_mean is None else _as(x_mean, x)
    lo, hi = (xm - 15000 * q).detach(), (xm + 15000 * q).detach()
    return q, lo, hi


def rate_torch(x, means, scales, probs=None, Q=1, x_mean=None, q_floor=None, return_lkl=False):
    """The formula as a torch program in x's dtype; autograd gives the reference's gradients (Low_bound: passes iff L >= 1e-6)."""
    q, lo, hi = _window(x, Q, x_mean, q_floor)
    xc = torch.clamp(x, min=lo, max=hi)
    L = None
    for i in range(len(means)):
        s = torch.clamp(scales[i], min=SCALE_FLOOR)
        cdf = lambda v: 0.5 * (1 + torch.erf((v - means[i]) * s.reciprocal() / math.sqrt(2)))   # noqa: E731
        t = torch.abs(cdf(xc + 0.5 * q) - cdf(xc - 0.5 * q))
        if probs is not None:
            t = probs[i] * t
        L = t if L is None else L + t
    Lb = _LowBound.apply(L)
    return Lb if return_lkl else -torch.log2(Lb)


class _LowBound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.clamp(x, min=LOW)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g * (x >= LOW).to(g.dtype)


def _f64(t):
    return t.detach().double() if isinstance(t, torch.Tensor) else torch.tensor(float(t), dtype=torch.float64)


def rate64(x, means, scales, probs=None, Q=1, x_mean=None, q_floor=None, return_lkl=False):
    """Forward in float64 on the CPU (inputs are widened from whatever they are); returns out and the likelihood L before the bound."""
    x = _f64(x).cpu()
    q = _f64(Q).cpu()
    if q_floor is not None:
        q = torch.clamp(q, min=q_floor)
    xm = x.mean() if x_mean is None else _f64(x_mean).cpu()
    xc = torch.minimum(torch.maximum(x, xm - 15000 * q), xm + 15000 * q)
    L = torch.zeros_like(x)
    for i in range(len(means)):
        m, s = _f64(means[i]).cpu(), torch.clamp(_f64(scales[i]).cpu(), min=SCALE_FLOOR)
        u = 0.5 * (1 + torch.erf((xc + q / 2 - m) / (s * math.sqrt(2))))
        lo = 0.5 * (1 + torch.erf((xc - q / 2 - m) / (s * math.sqrt(2))))
        p = 1.0 if probs is None else _f64(probs[i]).cpu()
        L = L + p * torch.abs(u - lo)
    Lb = torch.clamp(L, min=LOW)
    return (Lb if return_lkl else -torch.log2(Lb)), L


def grads64(g, x, means, scales, probs=None, Q=1, x_mean=None, q_floor=None, return_lkl=False):
    """Analytic gradients of sum(g * out) in float64: dict with 'x', 'mean', 'scale', 'prob' (lists) and 'Q', each shaped as the input
    (broadcast operands summed back); 'Q' is None for a number Q."""
    g = _f64(g).cpu()
    x64 = _f64(x).cpu()
    q_in = _f64(Q).cpu()
    q = torch.clamp(q_in, min=q_floor) if q_floor is not None else q_in
    xm = x64.mean() if x_mean is None else _f64(x_mean).cpu()
    lo_b, hi_b = xm - 15000 * q, xm + 15000 * q
    xc = torch.minimum(torch.maximum(x64, lo_b), hi_b)
    k = len(means)
    comps = []
    L = torch.zeros_like(x64)
    for i in range(k):
        m, s_raw = _f64(means[i]).cpu(), _f64(scales[i]).cpu()
        s = torch.clamp(s_raw, min=SCALE_FLOOR)
        du, dl = xc + q / 2 - m, xc - q / 2 - m
        u = 0.5 * (1 + torch.erf(du / (s * math.sqrt(2))))
        lo = 0.5 * (1 + torch.erf(dl / (s * math.sqrt(2))))
        p = torch.ones((), dtype=torch.float64) if probs is None else _f64(probs[i]).cpu()
        Li = torch.abs(u - lo)
        L = L + p * Li
        comps.append((m, s_raw, s, du, dl, u, lo, p, Li))
    Lb = torch.clamp(L, min=LOW)
    gL = g if return_lkl else -g / (Lb * math.log(2))
    gL = torch.where(L >= LOW, gL, torch.zeros_like(gL))
    gx = torch.zeros_like(x64)
    gq = torch.zeros_like(x64)
    out = {"mean": [], "scale": [], "prob": []}
    for i, (m, s_raw, s, du, dl, u, lo, p, Li) in enumerate(comps):
        a = gL * p * torch.sign(u - lo)
        pdf_u = torch.exp(-(du / s) ** 2 / 2) / (s * math.sqrt(2 * math.pi))
        pdf_l = torch.exp(-(dl / s) ** 2 / 2) / (s * math.sqrt(2 * math.pi))
        gx = gx + a * (pdf_u - pdf_l)
        gq = gq + a * (pdf_u + pdf_l) / 2
        out["mean"].append(_sum_to(-a * (pdf_u - pdf_l), means[i]))
        gs = -a * (pdf_u * du - pdf_l * dl) / s
        gs = torch.where(s_raw.expand_as(gs) >= SCALE_FLOOR, gs, torch.zeros_like(gs))
        out["scale"].append(_sum_to(gs, scales[i]))
        if probs is not None:
            out["prob"].append(_sum_to(gL * Li, probs[i]))
    out["x"] = torch.where((x64 >= lo_b) & (x64 <= hi_b), gx, torch.zeros_like(gx))
    if isinstance(Q, torch.Tensor):
        if q_floor is not None:
            gq = torch.where(q_in.expand_as(gq) >= q_floor, gq, torch.zeros_like(gq))
        out["Q"] = _sum_to(gq, Q)
    else:
        out["Q"] = None
    return out


def _sum_to(t, like):
    shape = like.shape if isinstance(like, torch.Tensor) else ()
    return t.sum_to_size(shape) if tuple(shape) != tuple(t.shape) else t


# ---- the reference's behaviour, for timing: Normal's validation and Low_bound's host round trip -------------------------------------

class _HostLowBound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.clamp(x, min=LOW)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        kept = g.clone()
        kept[x < LOW] = 0
        mask = np.logical_or(x.cpu().numpy() >= LOW, g.cpu().numpy() < 0.0)
        return kept * torch.from_numpy(mask.astype(np.float32)).to(g.device)


def _ref_bits(x, comps, Q, x_mean, lkl, mixture):
    if x_mean is None:
        x_mean = x.mean().detach() if mixture else x.mean()
    xc = torch.clamp(x, min=(x_mean - 15000 * Q).detach(), max=(x_mean + 15000 * Q).detach())
    L = None
    for mean, scale, prob in comps:
        d = torch.distributions.normal.Normal(mean, torch.clamp(scale, min=SCALE_FLOOR))
        t = torch.abs(d.cdf(xc + 0.5 * Q) - d.cdf(xc - 0.5 * Q))
        t = t if prob is None else prob * t
        L = t if L is None else L + t
    L = _HostLowBound.apply(L)
    if lkl:
        return L
    if mixture:
        L = _HostLowBound.apply(L)
    return -torch.log2(L)


class RefEntropy_gaussian(torch.nn.Module):
    def __init__(self, Q=1):
        super().__init__()
        self.Q = Q

    def forward(self, x, mean, scale, Q=None, x_mean=None):
        return _ref_bits(x, [(mean, scale, None)], self.Q if Q is None else Q, x_mean, False, False)


class RefEntropy_gaussian_mix_prob_2(torch.nn.Module):
    def __init__(self, Q=1):
        super().__init__()
        self.Q = Q

    def forward(self, x, mean1, mean2, scale1, scale2, probs1, probs2, Q=None, x_mean=None, return_lkl=False):
        return _ref_bits(x, [(mean1, scale1, probs1), (mean2, scale2, probs2)], self.Q if Q is None else Q, x_mean, return_lkl, True)


def make_case(n, c, k=1, seed=0, q_kind="row", device="cpu", saturate=False):
    """HAC-like inputs: quantised-looking x near the means, scales around 0.1-2, softmaxed probs; Q per row (n, 1), full, or a number.
    saturate adds a few elements far in the tails (on the 1e-6 floor) and outside the clamp window."""
    gen = torch.Generator().manual_seed(seed)
    mean = [torch.randn(n, c, generator=gen) * 2 for _ in range(k)]
    scale = [torch.exp(torch.randn(n, c, generator=gen) * 0.7 - 0.7) for _ in range(k)]
    x = torch.round(mean[0] + torch.randn(n, c, generator=gen) * 1.5)
    probs = None
    if k > 1:
        probs = list(torch.softmax(torch.randn(k, n, c, generator=gen), dim=0))
    if q_kind == "row":
        Q = 0.5 + torch.rand(n, 1, generator=gen)
    elif q_kind == "full":
        Q = 0.5 + torch.rand(n, c, generator=gen)
    else:
        Q = 1.0
    if saturate and n * c >= 8:
        flat = x.view(-1)
        flat[::7] += 40.0     # far tails: likelihood on the 1e-6 floor
    to = lambda t: t.to(device)   # noqa: E731
    return (to(x), [to(m) for m in mean], [to(s) for s in scale], None if probs is None else [to(p) for p in probs],
            to(Q) if isinstance(Q, torch.Tensor) else Q)


# ---- tests/golden/rate.npz (tests/golden/make_rate_golden.py) --------------------------------------------------------------------------

GOLDEN_CASES = {   # key: (k, module, return_lkl, q_floor)
    "k1_row": (1, "Entropy_gaussian", False, None), "k1_full": (1, "Entropy_gaussian", False, None),
    "k1_num": (1, "Entropy_gaussian", False, None), "k1_zero_d": (1, "Entropy_gaussian", False, None),
    "k1_clamp": (1, "Entropy_gaussian_clamp", False, None), "k2": (2, "Entropy_gaussian_mix_prob_2", False, None),
    "k3": (3, "Entropy_gaussian_mix_prob_3", False, None), "k2_lkl": (2, "Entropy_gaussian_mix_prob_2", True, None),
    "cat_floor": (1, "Entropy_gaussian", False, 1e-9),
}


def golden_case(g, key):
    """One recorded case as float32 CPU tensors: dict with x, means, scales, probs (None for k = 1), Q (tensor or number), x_mean (tensor
    or None), q_floor, lkl, module, w (upstream weights), out and the gradients g_x, g_mean, g_scale, g_prob, g_Q."""
    k, module, lkl, q_floor = GOLDEN_CASES[key]
    t = lambda name: torch.from_numpy(np.array(g[f"{key}_{name}"]))   # noqa: E731
    c = {"k": k, "module": module, "lkl": lkl, "q_floor": q_floor, "x": t("x"), "w": t("w"), "out": t("out"), "g_x": t("gx"),
         "means": [t(f"mean{j}") for j in range(k)], "scales": [t(f"scale{j}") for j in range(k)],
         "g_mean": [t(f"gmean{j}") for j in range(k)], "g_scale": [t(f"gscale{j}") for j in range(k)],
         "probs": [t(f"prob{j}") for j in range(k)] if k > 1 else None, "g_prob": [t(f"gprob{j}") for j in range(k)] if k > 1 else None}
    c["Q"], c["g_Q"] = (t("Q"), t("gQ")) if f"{key}_Q" in g else (float(g[f"{key}_Qnum"]), None)
    c["x_mean"] = t("xmean") if f"{key}_xmean" in g else None
    return c


L_MARGIN = 8 * 2.0 ** -24   # a float32 likelihood is good to a few ulps of 1 (the 1 + erf form cancels where the CDFs saturate)


def rel_error32(c, L):
    """Per element, a bound on the relative error of a float32 evaluation of L: L_MARGIN absolute, plus the rounding of the bin's edges
    x' +- Q/2 - mean, relative to the bin's width Q (HAC's scaling bins are 1e-3 wide around values of order 1)."""
    q = _f64(c["Q"]).abs()
    if c["q_floor"] is not None:
        q = torch.clamp(q, min=c["q_floor"])
    mag = c["x"].double().abs() + max(float(_f64(m).abs().max()) for m in c["means"]) + q
    return L_MARGIN / torch.clamp(L, min=LOW) + 2.0 ** -23 * mag / q


def near_kinks(c, rel=1e-3, flat=True):
    """Elements within a margin of a kink of the formula, where float32 and float64 may fall on different sides: the 1e-6 floor
    (|L - 1e-6| <= L_MARGIN + rel 1e-6), the clamp window's edges (relative margin) and, with flat, a component whose own likelihood is
    within L_MARGIN of 0 (float32 may round it to 0, where |.| has gradient 0); tests compare exactly only away from them."""
    _, L = rate64(c["x"], c["means"], c["scales"], c["probs"], c["Q"], c["x_mean"], c["q_floor"], c["lkl"])
    x = c["x"].double()
    q = _f64(c["Q"])
    if c["q_floor"] is not None:
        q = torch.clamp(q, min=c["q_floor"])
    xm = x.mean() if c["x_mean"] is None else _f64(c["x_mean"])
    hw = (15000 * q).expand_as(x)
    edge = torch.minimum((x - (xm - hw)).abs(), (x - (xm + hw)).abs()) <= rel * hw.abs() + 1e-6
    comp = torch.zeros_like(L, dtype=torch.bool)
    if flat:
        for m, s in zip(c["means"], c["scales"]):
            comp |= rate64(c["x"], [m], [s], None, c["Q"], c["x_mean"], c["q_floor"], True)[1] <= L_MARGIN
    return ((L - LOW).abs() <= L_MARGIN + rel * LOW) | edge | comp


def expanded(c):
    """The case with every operand (and a tensor Q) expanded to x's shape: grads64 of it gives per-element gradients."""
    full = lambda t: t.expand(c["x"].shape).clone() if isinstance(t, torch.Tensor) else t   # noqa: E731
    return dict(c, means=[full(t) for t in c["means"]], scales=[full(t) for t in c["scales"]],
                probs=None if c["probs"] is None else [full(t) for t in c["probs"]], Q=full(c["Q"]))
