"""The rate terms of the 3DGS compressors' training loss on the device (gsac_rate_forward / gsac_rate_backward): a drop-in for
utils/entropy_models.py (HAC, HAC++, CAT-3DGS) and TC-GS's utils/entropy.py:

    from utils.entropy_models import Entropy_gaussian   ->   from gauspcc_amd.entropy_models import Entropy_gaussian

`Entropy_gaussian`, `Entropy_gaussian_clamp`, `Entropy_gaussian_mix_prob_2` and `Entropy_gaussian_mix_prob_3` keep the reference's
`forward` signatures, defaults and float32 values (use_clamp = True, the frameworks' setting): bits = -log2(max(L, 1e-6)) of the Gaussian
(mixture) likelihood L of the bin [x - Q/2, x + Q/2], with x clamped to x_mean +- 15000 Q.  Each call is one autograd Function: one fused
kernel forward, one backward (plus a small fixed-order reduction when a one-value operand wants a gradient), no host synchronisation --
`x_mean` defaults to `x.mean()` computed by torch on the device.  Gradients reach x, every mean, scale and prob and a tensor Q; per-row
(n, 1) and one-value operands have their gradients summed in a fixed order in the library: bitwise reproducible.  CAT-3DGS floors Q at
1e-9 before use: `Entropy_gaussian(q_floor=1e-9)`.

Differences from the reference: non-finite mean or scale is not rejected (torch.distributions.Normal's argument validation is two host
syncs per call, exactly what this module removes); inputs must be float32 (TypeError otherwise) CUDA tensors (RuntimeError for CPU
tensors: there is no CPU path); operands must broadcast to x's shape.
"""
import ctypes
import numbers

import torch
import torch.nn as nn

from . import _lib, runtime
from .runtime import ptr, ptrs

FULL, ROW, ONE, HOST = 0, 1, 2, 3


def _check_tensor(t, name, who):
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a CUDA tensor (got {t.device}); gauspcc_amd has no CPU path")


class _Operand:
    """One of mean_i, scale_i, prob_i or Q as the kernels read it: its kind, the flat float32 device tensor (None for a host Q), and how
    its gradient goes back to the caller's shape."""
    __slots__ = ("kind", "data", "shape", "expanded", "host", "needs_grad")

    def __init__(self, v, name, x, n, c, who, allow_host=False):
        self.expanded, self.host, self.needs_grad = False, None, False
        if isinstance(v, numbers.Real) and not isinstance(v, bool):
            if allow_host:
                self.kind, self.data, self.shape, self.host = HOST, None, (), float(v)
                return
            v = torch.full((), float(v), dtype=torch.float32, device=x.device)
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch.Tensor or a number, got {type(v).__name__}")
        _check_tensor(v, name, who)
        if v.device != x.device:
            raise ValueError(f"{who}: {name} on {v.device}, x on {x.device}")
        self.shape, self.needs_grad = v.shape, v.requires_grad
        d = v.detach()
        if d.numel() == 1 and d.dim() <= x.dim():
            self.kind, self.data = ONE, d.reshape(1)
        elif x.dim() == 2 and tuple(d.shape) == (n, c):
            self.kind, self.data = FULL, d.contiguous()
        elif x.dim() == 2 and tuple(d.shape) == (n, 1):
            self.kind, self.data = ROW, d.reshape(n).contiguous()
        else:   # any other broadcastable shape: expanded here, its gradient summed back by sum_to_size
            try:
                e = d.expand(x.shape)
            except RuntimeError:
                raise ValueError(f"{who}: {name} of shape {tuple(d.shape)} does not broadcast to x's {tuple(x.shape)}") from None
            self.kind, self.data, self.expanded = FULL, e.reshape(n, c).contiguous(), True

    def grad_buffer(self, n, c):
        size = {FULL: (n, c), ROW: (n,), ONE: (1,)}[self.kind]
        return torch.empty(size, dtype=torch.float32, device=self.data.device)

    def to_caller(self, g, xshape):
        if self.expanded:
            return g.view(xshape).sum_to_size(self.shape)
        return g.view(self.shape)


class _Plan:
    """What one call of the fused rate term reads: k components, x as (n, c), its operands, Q and the options."""
    def __init__(self, k, x, n, c, ops, q, q_floor, lkl):
        self.k, self.xshape, self.n, self.c, self.ops, self.q = k, x.shape, n, c, ops, q
        self.q_floor, self.lkl = q_floor, bool(lkl)

    def args(self, x2, xm):
        k, ops, q = self.k, self.ops, self.q
        means, scales, probs = ops[:k], ops[k:2 * k], ops[2 * k:]
        kinds = [o.kind for o in means] + [o.kind for o in scales] + ([o.kind for o in probs] if k > 1 else [ONE] * k)
        return (k, self.n, self.c, x2.data_ptr(), xm.data_ptr(), ptrs([o.data for o in means]), ptrs([o.data for o in scales]),
                ptrs([o.data for o in probs]) if k > 1 else None, (ctypes.c_int * (3 * k))(*kinds),
                None if q.kind == HOST else q.data.data_ptr(), q.kind, 0.0 if q.host is None else q.host,
                0.0 if self.q_floor is None else float(self.q_floor), int(self.lkl))


def _forward(plan, x2, xm):
    out = torch.empty((plan.n, plan.c), dtype=torch.float32, device=x2.device)
    if plan.n:
        dev = x2.device
        _lib.check(_lib.lib().gsac_rate_forward(runtime.context(dev), *plan.args(x2, xm), out.data_ptr(), runtime.stream_ptr(dev)))
    return out.view(plan.xshape)


class _Rate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, x, xm, q_src, *op_srcs):
        x2 = x.detach().reshape(plan.n, plan.c).contiguous()
        ctx.plan = plan
        ctx.save_for_backward(x2, xm)
        return _forward(plan, x2, xm)

    @staticmethod
    def backward(ctx, grad):
        plan = ctx.plan
        x2, xm = ctx.saved_tensors
        n, c, k, q, ops = plan.n, plan.c, plan.k, plan.q, plan.ops
        dev = x2.device
        need = ctx.needs_input_grad
        gx = torch.empty((n, c), dtype=torch.float32, device=dev) if need[1] else None
        gq = q.grad_buffer(n, c) if need[3] else None
        gops = [o.grad_buffer(n, c) if need[4 + i] else None for i, o in enumerate(ops)]
        if n == 0:   # nothing to launch: empty gradients, and zero for the one-value operands (empty sums)
            gq = None if gq is None else gq.zero_()
            gops = [None if g is None else g.zero_() for g in gops]
        elif gx is not None or gq is not None or any(g is not None for g in gops):
            g = grad.detach().reshape(n, c).contiguous()
            _lib.check(_lib.lib().gsac_rate_backward(runtime.context(dev), *plan.args(x2, xm), g.data_ptr(), ptr(gx), ptrs(gops[:k]),
                                                     ptrs(gops[k:2 * k]), ptrs(gops[2 * k:]) if k > 1 else None, ptr(gq),
                                                     runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
        back = lambda g, o: None if g is None else o.to_caller(g, plan.xshape)   # noqa: E731
        return (None, None if gx is None else gx.view(plan.xshape), None, back(gq, q)) + tuple(back(g, o) for g, o in zip(gops, ops))


def rate(x, means, scales, probs=None, Q=1, x_mean=None, q_floor=None, return_lkl=False, who="rate"):
    """The fused rate term, shaped as x: -log2(max(L, 1e-6)) (or max(L, 1e-6) with return_lkl) of x under the k = len(means) component
    Gaussian model; probs is None for k = 1.  The Entropy_* modules below are this with the reference's signatures."""
    k = len(means)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{who}: x must be a torch.Tensor, got {type(x).__name__}")
    _check_tensor(x, "x", who)
    c = max(x.shape[-1], 1) if x.dim() >= 1 else 1
    n = x.numel() // c
    if q_floor is not None and isinstance(Q, numbers.Real):
        Q = max(float(Q), float(q_floor))
    names = [f"mean{i + 1}" for i in range(k)] + [f"scale{i + 1}" for i in range(k)] + ([f"probs{i + 1}" for i in range(k)] if k > 1 else [])
    vals = list(means) + list(scales) + (list(probs) if k > 1 else [])
    ops = [_Operand(v, nm, x, n, c, who) for v, nm in zip(vals, names)]
    q = _Operand(Q, "Q", x, n, c, who, allow_host=True)
    if x_mean is None:
        xm = x.detach().mean().reshape(1)
    elif isinstance(x_mean, torch.Tensor):
        if x_mean.numel() != 1:
            raise ValueError(f"{who}: x_mean must hold one value, got shape {tuple(x_mean.shape)}")
        if not x_mean.is_cuda:
            raise RuntimeError(f"{who}: x_mean must be a CUDA tensor (got {x_mean.device}); gauspcc_amd has no CPU path")
        xm = x_mean.detach().reshape(1).to(device=x.device, dtype=torch.float32)
    else:
        xm = torch.full((1,), float(x_mean), dtype=torch.float32, device=x.device)
    plan = _Plan(k, x, n, c, ops, q, q_floor, return_lkl)
    if torch.is_grad_enabled() and (x.requires_grad or q.needs_grad or any(o.needs_grad for o in ops)):
        # autograd sees the caller's tensors (numbers become the device values the kernels read); the kernels read the flat copies
        srcs = [v if isinstance(v, torch.Tensor) else o.data for v, o in zip(vals, ops)]
        return _Rate.apply(plan, x, xm, Q if q.needs_grad else None, *srcs)
    return _forward(plan, x.detach().reshape(n, c).contiguous(), xm)


class Low_bound(torch.autograd.Function):
    """max(x, 1e-6), the gradient passed iff x >= 1e-6 (the reference's extra pass-through where g < 0 multiplies a gradient that is
    already zero there, so it changes nothing); no host copy."""
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.clamp(x, min=1e-6)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return torch.where(x >= 1e-6, g, torch.zeros((), dtype=g.dtype, device=g.device))


class Entropy_gaussian(nn.Module):
    def __init__(self, Q=1, q_floor=None):
        super().__init__()
        self.Q = Q
        self.q_floor = q_floor

    def forward(self, x, mean, scale, Q=None, x_mean=None):
        if Q is None:
            Q = self.Q
        return rate(x, [mean], [scale], None, Q, x_mean, self.q_floor, who="Entropy_gaussian")


class Entropy_gaussian_clamp(nn.Module):
    def __init__(self, Q=1):
        super().__init__()
        self.Q = Q

    def forward(self, x, mean, scale, Q=None):
        if Q is None:
            Q = self.Q
        return rate(x, [mean], [scale], None, Q, None, who="Entropy_gaussian_clamp")


class Entropy_gaussian_mix_prob_2(nn.Module):
    def __init__(self, Q=1):
        super().__init__()
        self.Q = Q

    def forward(self, x, mean1, mean2, scale1, scale2, probs1, probs2, Q=None, x_mean=None, return_lkl=False):
        if Q is None:
            Q = self.Q
        return rate(x, [mean1, mean2], [scale1, scale2], [probs1, probs2], Q, x_mean, return_lkl=return_lkl, who="Entropy_gaussian_mix_prob_2")


class Entropy_gaussian_mix_prob_3(nn.Module):
    def __init__(self, Q=1):
        super().__init__()
        self.Q = Q

    def forward(self, x, mean1, mean2, mean3, scale1, scale2, scale3, probs1, probs2, probs3, Q=None, x_mean=None, return_lkl=False):
        if Q is None:
            Q = self.Q
        return rate(x, [mean1, mean2, mean3], [scale1, scale2, scale3], [probs1, probs2, probs3], Q, x_mean, return_lkl=return_lkl,
                    who="Entropy_gaussian_mix_prob_3")
