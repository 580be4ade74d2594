"""torch_scatter.scatter_max on the device (gpcc_scatter_max), the one torch_scatter function HAC, HAC++, TC-GS and CAT-3DGS call
(in anchor_growing):

    from torch_scatter import scatter_max   ->   from gauspcc_amd.scatter import scatter_max

Same signature, same (out, argmax) result, with torch_scatter's race-dependent tie rule made deterministic: among equal maxima the
smallest source index wins, a NaN in a group wins over every number, and the value's bits are those of the winning element
(include/gauspcc.h, gpcc_scatter_max).  Without `out`, a result equal to -FLT_MAX is set to 0, as torch_scatter does when it allocates
the output itself.  float32 CUDA tensors only; there is no CPU path.
"""
import torch

from . import _lib, runtime


def scatter_max_rows(src, index, dim_size, out=None):
    """gpcc_scatter_max on checked tensors: src (M, C) float32, index (M,) int64, both contiguous on one device.  out (S, C) float32
    contiguous gives include-self semantics and is written in place.  Returns (out, arg (S, C) int64)."""
    M, C = src.shape
    dev = src.device
    include_self = out is not None
    if out is None:
        out = torch.empty((dim_size, C), dtype=torch.float32, device=dev)
    arg = torch.empty((dim_size, C), dtype=torch.int64, device=dev)
    if dim_size == 0 and M == 0:
        return out, arg
    _lib.check(_lib.lib().gpcc_scatter_max(runtime.context(dev), src.data_ptr() if M else None, index.data_ptr() if M else None, M, C, dim_size,
                                           int(include_self), out.data_ptr(), arg.data_ptr(), runtime.Workspace(dev).fn(), None,
                                           runtime.stream_ptr(dev)))
    return out, arg


def _broadcast(src, other, dim):
    """torch_scatter.utils.broadcast: a 1-D index is aligned to `dim` and expanded to src's shape."""
    if dim < 0:
        dim = other.dim() + dim
    if src.dim() == 1:
        for _ in range(0, dim):
            src = src.unsqueeze(0)
    for _ in range(src.dim(), other.dim()):
        src = src.unsqueeze(-1)
    return src.expand(other.size())


def _check(src, index, out, dim_size):
    if not isinstance(src, torch.Tensor) or not isinstance(index, torch.Tensor):
        raise TypeError("scatter_max: src and index must be torch.Tensors")
    if src.dtype != torch.float32:
        raise TypeError(f"scatter_max: src must be float32, got {src.dtype}")
    if index.dtype != torch.int64:
        raise TypeError(f"scatter_max: index must be int64, got {index.dtype}")
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("scatter_max: out must be a torch.Tensor")
        if out.dtype != torch.float32:
            raise TypeError(f"scatter_max: out must be float32, got {out.dtype}")
    if dim_size is not None and (isinstance(dim_size, bool) or not isinstance(dim_size, int) or dim_size < 0):
        raise ValueError(f"scatter_max: dim_size must be a non-negative int, got {dim_size!r}")
    for name, t in (("src", src), ("index", index), ("out", out)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"scatter_max: {name} must be a CUDA tensor, got device {t.device}")
    if index.device != src.device or (out is not None and out.device != src.device):
        raise ValueError("scatter_max: src, index and out must be on one device")


class _ScatterMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index, dim, out, dim_size):
        res, arg = _forward(src, index, dim, out, dim_size)
        ctx.mark_non_differentiable(arg)
        ctx.save_for_backward(arg)
        ctx.dim, ctx.size = dim, src.shape[dim]
        if out is not None:
            ctx.mark_dirty(out)
        return res, arg

    @staticmethod
    def backward(ctx, grad_out, grad_arg):
        (arg,) = ctx.saved_tensors
        dim = ctx.dim
        shape = list(grad_out.shape)
        shape[dim] = ctx.size + 1
        grad_src = grad_out.new_zeros(shape)
        grad_src.scatter_(dim, arg, grad_out)   # one arg per (slot, column): no two slots write one element, except the dropped row `size`
        return grad_src.narrow(dim, 0, ctx.size), None, None, None, None


def _forward(src, index, dim, out, dim_size):
    index = _broadcast(index, src, dim)
    M = src.shape[dim]
    if out is not None:
        S = out.shape[dim]
        exp = list(src.shape)
        exp[dim] = S
        if list(out.shape) != exp:
            raise ValueError(f"scatter_max: out must have shape {tuple(exp)}, got {tuple(out.shape)}")
    elif dim_size is not None:
        S = dim_size
    else:
        S = int(index.max()) + 1 if index.numel() > 0 else 0   # torch_scatter's default (one read-back)
    shape = list(src.shape)
    shape[dim] = S
    rest = shape[:dim] + shape[dim + 1:]
    C = 1
    for s in rest:
        C *= s
    src_m = src.detach().movedim(dim, 0).reshape(M, C).contiguous()
    idx_m = index.movedim(dim, 0)
    init = out.detach().movedim(dim, 0).reshape(S, C).contiguous() if out is not None else None
    if C == 0 or all(st == 0 for st in idx_m.stride()[1:]) or idx_m.dim() == 1:
        rows = idx_m.reshape(M, C)[:, 0].contiguous() if C else idx_m.new_zeros(M)
        res, arg = scatter_max_rows(src_m, rows, S, init)
    else:
        # a full index: one column over the flattened key index * C + column
        col = torch.arange(C, device=src.device, dtype=torch.int64)
        key = (idx_m.reshape(M, C) * C + col).reshape(-1).contiguous()
        bad = (idx_m.reshape(M, C) < 0) | (idx_m.reshape(M, C) >= S)
        key = torch.where(bad.reshape(-1), torch.full_like(key, -1), key)   # keep an out-of-range index out of range after flattening
        res, arg = scatter_max_rows(src_m.reshape(M * C, 1), key, S * C, None if init is None else init.reshape(S * C, 1))
        res, arg = res.reshape(S, C), arg.reshape(S, C)
        arg = torch.where(arg == M * C, torch.full_like(arg, M), arg // C)
    res = res.reshape([S] + rest).movedim(0, dim)
    arg = arg.reshape([S] + rest).movedim(0, dim).contiguous()
    if out is not None:
        out.copy_(res)
        res = out
    else:
        res = res.contiguous()
    return res, arg


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    """torch_scatter.scatter_max: (out, argmax).  Differentiable with respect to src: the gradient goes to argmax, slots whose argmax is
    src.size(dim) get none."""
    _check(src, index, out, dim_size)
    if src.dim() == 0:
        raise ValueError("scatter_max: src must have at least one dimension")
    if index.dim() > src.dim():
        raise ValueError(f"scatter_max: index has {index.dim()} dimensions, src {src.dim()}")
    dim = dim + src.dim() if dim < 0 else dim
    if not 0 <= dim < src.dim():
        raise ValueError(f"scatter_max: dim {dim} outside src's {src.dim()} dimensions")
    if torch.is_grad_enabled() and src.requires_grad:
        return _ScatterMax.apply(src, index, dim, out, dim_size)
    return _forward(src, index, dim, out, dim_size)
