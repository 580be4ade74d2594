"""The two-layer context MLPs of HAC / HAC++ / TC-GS as trainable modules on the device (gshac_mlp2_act / gshac_mlp2_backward): drop-ins for

    self.mlp_grid = nn.Sequential(nn.Linear(..), nn.ReLU(True), nn.Linear(..))   ->   ContextMLP(din, dh, dout)
                                                (HAC/scene/gaussian_model.py:258-262, HAC-plus/scene/gaussian_model.py:370-374)
    Channel_CTX_fea, Channel_CTX_fea_tiny       ->   from gauspcc_amd.mlp import Channel_CTX_fea, Channel_CTX_fea_tiny
                                                (HAC-plus/scene/gaussian_model.py:117-220, built at :377-380)

The forward is the codecs': `mlp2_forward`, the bit-specified chain (bias, then fmaf over k ascending) that the conduct_encoding / conduct_decoding
drop-ins evaluate when they encode and decode (anchor_codec.run_mlp2), so the rate model is trained on exactly the means, scales and step sizes
the coder will compute.  Nothing is saved for the backward except the inputs: it recomputes the hidden layer with the same chain.  Weight and bias
gradients are summed in a fixed order (no atomics): bitwise reproducible from run to run and across streams.

`ContextMLP` IS an nn.Sequential(Linear, ReLU | LeakyReLU, Linear): state-dict keys 0.weight, 0.bias, 2.weight, 2.bias, code that walks
it for nn.Linear and the codecs' own recognition of the pattern keep working.  Only float32 CUDA input takes the fused path; anything
else (float64, CPU, autocast to another dtype) goes through Sequential.forward.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, runtime
from .runtime import ptr

_ACTS = {"relu": 0, "leaky_relu": 1}


def slab_rows(n, din, dh, dout):
    """Rows per slab of the backward's fixed-order parameter-gradient sums for n rows of a din-dh-dout layer (a function of these alone)."""
    return int(_lib.lib().gshac_mlp2_slab_rows(int(n), int(din), int(dh), int(dout)))


def mlp2_forward(x, w1, b1, w2, b2, act="relu", slope=0.0):
    """W2 act(W1 x + b1) + b2 without autograd, x (n, din) -> (n, dout): the ONE call of gshac_mlp2_act from Python -- the codecs' context MLPs
    (anchor_codec.run_mlp2, hac_codec.mlp2, hac_plus_codec.mlp2_act) and `mlp2` below end here.  Any float dtype and strides."""
    x, w1, b1, w2, b2 = (t.detach().contiguous().float() for t in (x, w1, b1, w2, b2))
    n, din = x.shape
    dh, dout = w1.shape[0], w2.shape[0]
    y = torch.empty(n, dout, device=x.device, dtype=torch.float32)
    if n == 0:          # nothing to launch (and an empty tensor has no address to pass)
        return y
    _lib.check(_lib.lib().gshac_mlp2_act(runtime.context(x.device), ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), n, din, dh, dout, _ACTS[act], float(slope),
                                         ptr(y), runtime.stream_ptr(x.device)))
    return y


class _MLP2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act, slope):
        t = tuple(v.detach().contiguous() for v in (x, w1, b1, w2, b2))
        ctx.save_for_backward(*t)
        ctx.act = (_ACTS[act], slope)
        return mlp2_forward(*t, act, slope)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        x, w1, b1, w2, b2 = ctx.saved_tensors
        act, slope = ctx.act
        n, din = x.shape
        dh, dout = w1.shape[0], w2.shape[0]
        dy = grad.to(torch.float32).contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw1, db1, dw2, db2 = (torch.empty_like(v) for v in (w1, b1, w2, b2))
        _lib.check(_lib.lib().gshac_mlp2_backward(runtime.context(x.device), ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), n, din, dh, dout, act, slope,
                                                  ptr(dy), ptr(dx), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), runtime.Workspace(x.device).fn(), None,
                                                  runtime.stream_ptr(x.device)))
        need = ctx.needs_input_grad
        return dx, *(g if need[i + 1] else None for i, g in enumerate((dw1, db1, dw2, db2))), None, None


def mlp2(x, w1, b1, w2, b2, act="relu", slope=0.01):
    """W2 act(W1 x + b1) + b2 over the last dimension of x (any leading shape, any strides), float32 CUDA tensors; w1 (dh, din), w2 (dout, dh)
    as nn.Linear stores them.  act 'relu' or 'leaky_relu' (with `slope`).  Differentiable in all five tensors."""
    if act not in _ACTS:
        raise ValueError(f"mlp2: act must be 'relu' or 'leaky_relu', got {act!r}")
    for t, name in ((x, "x"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
            raise TypeError(f"mlp2: {name} must be a float32 CUDA tensor")
        if t.device != x.device:
            raise ValueError(f"mlp2: {name} on {t.device}, x on {x.device}")
    if w1.dim() != 2 or w2.dim() != 2 or x.dim() < 1 or x.shape[-1] != w1.shape[1] or w2.shape[1] != w1.shape[0] or b1.shape != w1.shape[:1] \
            or b2.shape != w2.shape[:1]:
        raise ValueError(f"mlp2: shapes x {tuple(x.shape)}, w1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, w2 {tuple(w2.shape)}, b2 {tuple(b2.shape)}")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, w1, b1, w2, b2)):
        y = _MLP2.apply(x2, w1, b1, w2, b2, act, float(slope))
    else:
        y = mlp2_forward(x2, w1, b1, w2, b2, act, slope)
    return y.view(*lead, w2.shape[0])


class ContextMLP(nn.Sequential):
    """nn.Sequential(Linear(din, dh), ReLU | LeakyReLU(slope), Linear(dh, dout)) whose forward and backward are the fused kernels."""

    def __init__(self, din, dh, dout, act="relu", slope=0.01):
        if act not in _ACTS:
            raise ValueError(f"ContextMLP: act must be 'relu' or 'leaky_relu', got {act!r}")
        super().__init__(nn.Linear(din, dh), nn.ReLU(True) if act == "relu" else nn.LeakyReLU(slope, inplace=True), nn.Linear(dh, dout))

    @classmethod
    def from_sequential(cls, seq):
        """A ContextMLP over the SAME Linear modules (hence the same parameter tensors: an optimiser built on `seq` keeps working)."""
        mods = list(seq)
        if len(mods) != 3 or not isinstance(mods[0], nn.Linear) or not isinstance(mods[2], nn.Linear) or not isinstance(mods[1], (nn.ReLU, nn.LeakyReLU)) \
                or mods[0].bias is None or mods[2].bias is None:
            raise ValueError("ContextMLP.from_sequential: expected Sequential(Linear, ReLU | LeakyReLU, Linear) with biases")
        leaky = isinstance(mods[1], nn.LeakyReLU)
        m = cls(1, 1, 1, "leaky_relu" if leaky else "relu", mods[1].negative_slope if leaky else 0.01)
        m[0], m[2] = mods[0], mods[2]
        return m

    def forward(self, x):
        a = self[1]
        if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and self[0].weight.dtype == torch.float32 and self[0].weight.device == x.device:
            leaky = isinstance(a, nn.LeakyReLU)
            return mlp2(x, self[0].weight, self[0].bias, self[2].weight, self[2].bias, "leaky_relu" if leaky else "relu", a.negative_slope if leaky else 0.0)
        return super().forward(x)


def _channel_outputs(groups, to_dec):
    """groups: five (mean, scale, prob) triples -> the triple of group `to_dec`, or the three concatenations over the groups."""
    if 0 <= to_dec <= 4:
        return groups[to_dec]
    return tuple(torch.cat([grp[j] for grp in groups], dim=-1) for j in range(3))


class Channel_CTX_fea(nn.Module):
    """HAC-plus/scene/gaussian_model.py:117-168: MLP_d0 .. MLP_d4 = Linear(150 + 10 c, 40) - LeakyReLU - Linear(40, 30) over
    cat([groups 0 .. c - 1 of fea_q, mean_scale]); returns (mean_adj, scale_adj, prob_adj): (N, 50) each, or group `to_dec` alone, (N, 10) each."""

    def __init__(self):
        super().__init__()
        for c in range(5):
            setattr(self, f"MLP_d{c}", ContextMLP(50 * 3 + 10 * c, 20 * 2, 10 * 3, "leaky_relu"))

    def forward(self, fea_q, mean_scale, to_dec=-1):
        todo = range(5) if not 0 <= to_dec <= 4 else (to_dec,)
        groups = {c: torch.chunk(getattr(self, f"MLP_d{c}")(torch.cat([fea_q[:, :10 * c], mean_scale], dim=-1)), chunks=3, dim=-1) for c in todo}
        return _channel_outputs([groups.get(c) for c in range(5)], to_dec)


class Channel_CTX_fea_tiny(nn.Module):
    """HAC-plus/scene/gaussian_model.py:170-220: without mean_scale in the context.  Group 0 is three learned (1, 10) constants (mean_d0, scale_d0,
    prob_d0); MLP_d1 .. MLP_d4 = Linear(10 c, 30) - LeakyReLU - Linear(30, 30) over groups 0 .. c - 1 of fea_q."""

    def __init__(self):
        super().__init__()
        self.mean_d0 = nn.Parameter(torch.zeros(size=[1, 10]))
        self.scale_d0 = nn.Parameter(torch.zeros(size=[1, 10]))
        self.prob_d0 = nn.Parameter(torch.zeros(size=[1, 10]))
        for c in range(1, 5):
            setattr(self, f"MLP_d{c}", ContextMLP(10 * c, 10 * 3, 10 * 3, "leaky_relu"))

    def forward(self, fea_q, mean_scale, to_dec=-1):
        n = fea_q.shape[0]
        todo = range(5) if not 0 <= to_dec <= 4 else (to_dec,)
        groups = {}
        for c in todo:
            if c == 0:
                groups[0] = (self.mean_d0.repeat(n, 1), self.scale_d0.repeat(n, 1), self.prob_d0.repeat(n, 1))
            else:
                groups[c] = torch.chunk(getattr(self, f"MLP_d{c}")(fea_q[:, :10 * c]), chunks=3, dim=-1)
        return _channel_outputs([groups.get(c) for c in range(5)], to_dec)
