"""Densification bookkeeping on the device: drop-ins for `GaussianModel.training_statis` and `GaussianModel.adjust_anchor` of HAC, HAC++,
TC-GS and CAT-3DGS (e.g. HAC/scene/gaussian_model.py:758-775 and :914-968; the four files hold the same program), and the multi-tensor
row compaction that `_prune_anchor_optimizer` needs, with its differentiable form `select_rows` (the masked gathers of the training branches;
backward: gpcc_expand_rows).

`training_statis` is one native call (gpcc_densify_stats) that never waits for the host: the reference's four boolean-mask index
operations are two scans and one update pass.  What the host cannot know from shapes -- that the visible mask counts as many anchors as
`opacity` has rows, and the selection mask as many entries as `update_filter` -- is checked on the device; a disagreement leaves the
accumulators untouched and is raised as a ValueError by the next call that synchronises anyway: `adjust_anchor` or `check`.

The float32 contract is in include/gauspcc.h; tests/densify_ref.py restates it in numpy.  INTEGRATION.md shows the bindings.
"""
import ctypes

import numpy as np
import torch

from . import _lib, runtime

MAX_TENSORS = 32          # gpcc_compact_rows
_ERR_WORDS = 8
_ERR = {}                 # device index -> the sticky error words of gpcc_densify_stats (int32 tensor)


def _tensor(t, name, dtype, who):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    return t


def _flat(t, name, dtype, numel, who):
    """t as it is when it holds numel elements of dtype contiguously (shape (numel,) or (numel, 1))"""
    _tensor(t, name, dtype, who)
    if t.numel() != numel or t.dim() > 2 or (t.dim() == 2 and t.shape[1] != 1 and t.shape[0] != 1):
        raise ValueError(f"{who}: {name} must hold {numel} elements as ({numel},) or ({numel}, 1), got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    return t


def _one_device(who, *ts):
    """the tensors' device: CUDA, and one for all (there is no CPU path)"""
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError(f"{who}: every tensor must be a CUDA tensor, got device {t.device}")
    dev = ts[0].device
    if any(t is not None and t.device != dev for t in ts):
        raise ValueError(f"{who}: all tensors must be on one device")
    return dev


def _ptr(t):   # NULL for None and for an empty tensor
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _err_words(dev):
    idx = runtime._device_index(dev)
    if idx not in _ERR:
        _ERR[idx] = torch.zeros(_ERR_WORDS, dtype=torch.int32, device=torch.device("cuda", idx))
    return _ERR[idx]


def check(device=None):
    """Raises the pending error of an earlier `accumulate_stats` / `training_statis` on this device, if any (and clears it).  Waits for the
    current stream, which must be the one those calls ran on: call it where the loop synchronises anyway."""
    idx = runtime._device_index(device)
    if idx not in _ERR:
        return
    w = _ERR[idx].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    if not w[0]:
        return
    _ERR[idx].zero_()
    what = []
    if w[0] & 1:
        what.append(f"anchor_visible_mask has {w[1]} set entries but opacity has rows for {w[2]} anchors")
    if w[0] & 2:
        what.append(f"offset_selection_mask has {w[3]} set entries but update_filter has {w[4]}")
    raise ValueError("training_statis: " + "; ".join(what) + " (figures of the last such call); that call left the accumulators unchanged")


def accumulate_stats(opacity_accum, anchor_demon, offset_gradient_accum, offset_denom, grad, opacity, update_filter, offset_selection_mask,
                     anchor_visible_mask, n_offsets):
    """One iteration's update of the four float32 accumulators, in place, without a host synchronisation (gpcc_densify_stats).
    opacity_accum, anchor_demon (N, 1); offset_gradient_accum, offset_denom (N K, 1); grad (S, >= 2) float32 (columns 0 and 1 are read, rows
    may be strided); opacity (V K) float32; update_filter (S) bool; offset_selection_mask (V K) bool; anchor_visible_mask (N) bool or None
    (all anchors).  Ill-formed masks are reported by `check`."""
    who = "accumulate_stats"
    if isinstance(n_offsets, bool) or not isinstance(n_offsets, int) or n_offsets < 1:
        raise ValueError(f"{who}: n_offsets must be a positive int, got {n_offsets!r}")
    K = n_offsets
    _tensor(anchor_demon, "anchor_demon", torch.float32, who)
    N = anchor_demon.numel()
    _flat(anchor_demon, "anchor_demon", torch.float32, N, who)
    _flat(opacity_accum, "opacity_accum", torch.float32, N, who)
    _flat(offset_gradient_accum, "offset_gradient_accum", torch.float32, N * K, who)
    _flat(offset_denom, "offset_denom", torch.float32, N * K, who)
    _tensor(opacity, "opacity", torch.float32, who)
    if opacity.numel() % K:
        raise ValueError(f"{who}: opacity holds {opacity.numel()} values, not a multiple of n_offsets = {K}")
    V = opacity.numel() // K
    _flat(offset_selection_mask, "offset_selection_mask", torch.bool, V * K, who)
    _tensor(update_filter, "update_filter", torch.bool, who)
    S = update_filter.numel()
    _flat(update_filter, "update_filter", torch.bool, S, who)
    _tensor(grad, "grad", torch.float32, who)
    if grad.dim() != 2 or grad.shape[0] != S or grad.shape[1] < 2:
        raise ValueError(f"{who}: grad must be ({S}, >= 2) to go with update_filter, got {tuple(grad.shape)}")
    if anchor_visible_mask is not None:
        _flat(anchor_visible_mask, "anchor_visible_mask", torch.bool, N, who)
    elif V != N:
        raise ValueError(f"{who}: no anchor_visible_mask, but opacity has rows for {V} anchors of {N}")
    if S > V * K:
        raise ValueError(f"{who}: update_filter has {S} entries for {V * K} neural Gaussians")
    dev = _one_device(who, anchor_demon, opacity_accum, offset_gradient_accum, offset_denom, opacity, offset_selection_mask, update_filter, grad,
                      anchor_visible_mask)
    opacity = opacity.detach().contiguous()
    grad = grad.detach()
    if S and (grad.stride(1) != 1 or grad.stride(0) < 2):
        grad = grad.contiguous()
    work = runtime.Workspace(dev)
    _lib.check(_lib.lib().gpcc_densify_stats(runtime.context(dev), N, K, _ptr(anchor_visible_mask), _ptr(opacity), V, _ptr(offset_selection_mask),
                                             _ptr(update_filter), S, _ptr(grad), grad.stride(0) if S else 2, _ptr(opacity_accum), _ptr(anchor_demon),
                                             _ptr(offset_gradient_accum), _ptr(offset_denom), _err_words(dev).data_ptr(), work.fn(), None,
                                             runtime.stream_ptr(dev)))


def _floats(buf, *shape):
    n = int(np.prod(shape, dtype=np.int64))
    return buf[:4 * n].view(torch.float32).view(*shape)


def compact_rows(keep, *tensors):
    """[t[keep] for t in tensors] for up to 32 float32 tensors of keep.shape[0] rows (any trailing shape), detached: one scan, one launch
    over all of them and one synchronisation (gpcc_compact_rows) where the indexing does a nonzero and a wait per tensor."""
    who = "compact_rows"
    _tensor(keep, "keep", torch.bool, who)
    if keep.dim() != 1 or not keep.is_contiguous():
        raise ValueError(f"{who}: keep must be a contiguous 1-D mask, got {tuple(keep.shape)}")
    if len(tensors) > MAX_TENSORS:
        raise ValueError(f"{who}: {len(tensors)} tensors, at most {MAX_TENSORS} in one call")
    N = keep.shape[0]
    for i, t in enumerate(tensors):
        _tensor(t, f"tensor {i}", torch.float32, who)
        if t.dim() < 1 or t.shape[0] != N:
            raise ValueError(f"{who}: tensor {i} must have {N} rows, got {tuple(t.shape)}")
    dev = _one_device(who, keep, *tensors)
    srcs = [t.detach().contiguous() for t in tensors]
    widths = [int(np.prod(t.shape[1:], dtype=np.int64)) for t in tensors]
    T = len(srcs)
    work = runtime.Workspace(dev)
    count = ctypes.c_int64(0)
    _lib.check(_lib.lib().gpcc_compact_rows(runtime.context(dev), _ptr(keep), N, T, runtime.ptrs([None if t.numel() == 0 else t for t in srcs], max(T, 1)),
                                            (ctypes.c_int64 * max(T, 1))(*widths), ctypes.byref(count), work.fn(), None, runtime.stream_ptr(dev)))
    n2 = count.value
    if n2 == 0:
        return [torch.empty((0, *t.shape[1:]), dtype=torch.float32, device=dev) for t in tensors]
    return [_floats(work.buffers[1 + i], n2, *t.shape[1:]) for i, t in enumerate(tensors)]   # allocation (1) is the ranks


def _check_rows(who, keep, tensors):
    """the argument checks of select_rows: ValueErrors that name the argument"""
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.dim() != 1 or not keep.is_contiguous() or not keep.is_cuda:
        raise ValueError(f"{who}: mask must be a contiguous 1-D bool CUDA tensor")
    if len(tensors) > MAX_TENSORS:
        raise ValueError(f"{who}: {len(tensors)} tensors, at most {MAX_TENSORS} in one call")
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device != keep.device:
            raise ValueError(f"{who}: tensor {i} must be a float32 CUDA tensor on the mask's device")
        if t.dim() < 1 or t.shape[0] != keep.shape[0]:
            raise ValueError(f"{who}: tensor {i} must have {keep.shape[0]} rows, got {tuple(t.shape)}")


class _SelectRows(torch.autograd.Function):
    """gpcc_compact_rows / gpcc_expand_rows over all tensors at once"""

    @staticmethod
    def forward(ctx, keep, *tensors):
        outs = compact_rows(keep, *tensors)
        ctx.keep, ctx.m, ctx.shapes = keep, (outs[0].shape[0] if outs else 0), [t.shape for t in tensors]
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        keep, m, dev = ctx.keep, ctx.m, ctx.keep.device
        N = keep.shape[0]
        want = [i for i in range(len(grads)) if ctx.needs_input_grad[1 + i]]
        out = [None] * len(grads)
        if want:
            srcs = [torch.zeros((m, *ctx.shapes[i][1:]), dtype=torch.float32, device=dev) if grads[i] is None else grads[i].detach().to(torch.float32).contiguous()
                    for i in want]
            dsts = [torch.empty(ctx.shapes[i], dtype=torch.float32, device=dev) for i in want]
            widths = [int(np.prod(ctx.shapes[i][1:], dtype=np.int64)) for i in want]
            T = len(want)
            _lib.check(_lib.lib().gpcc_expand_rows(runtime.context(dev), _ptr(keep), N, m, T, runtime.ptrs([None if t.numel() == 0 else t for t in srcs], T),
                                                   (ctypes.c_int64 * T)(*widths), runtime.ptrs([None if t.numel() == 0 else t for t in dsts], T),
                                                   runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
            for i, d in zip(want, dsts):
                out[i] = d
        return (None, *out)


def select_rows(mask, *tensors):
    """tuple(t[mask] for t in tensors), differentiable: the values and the gradients are those of the indexing, bit for bit.  The forward is
    one gpcc_compact_rows call (one scan, one launch, one wait for the row count) where the indexing does a nonzero and a wait per tensor;
    the backward is one gpcc_expand_rows call, without a wait, for all the tensors that need a gradient (the others get None).  Up to 32
    float32 CUDA tensors of mask.shape[0] rows, any trailing shape; anything else raises a ValueError that names the argument."""
    _check_rows("select_rows", mask, tensors)
    if not tensors:
        return ()
    return _SelectRows.apply(mask, *tensors)


def front(offset_gradient_accum, offset_denom, offset_thr):
    """(grads_norm (N K) float32, offset_mask (N K) bool): |accum / denom| with NaN -> 0 and denom > float32(offset_thr) (gpcc_densify_front)"""
    who = "adjust_anchor"
    _tensor(offset_denom, "offset_denom", torch.float32, who)
    total = offset_denom.numel()
    _flat(offset_denom, "offset_denom", torch.float32, total, who)
    _flat(offset_gradient_accum, "offset_gradient_accum", torch.float32, total, who)
    dev = _one_device(who, offset_denom, offset_gradient_accum)
    grads_norm = torch.empty(total, dtype=torch.float32, device=dev)
    offset_mask = torch.empty(total, dtype=torch.bool, device=dev)
    _lib.check(_lib.lib().gpcc_densify_front(runtime.context(dev), _ptr(offset_gradient_accum), _ptr(offset_denom), total, float(np.float32(offset_thr)),
                                             _ptr(grads_norm), _ptr(offset_mask), runtime.stream_ptr(dev)))
    return grads_norm, offset_mask


def finish(offset_gradient_accum, offset_denom, offset_mask, opacity_accum, anchor_demon, n_offsets, anchor_thr, min_opacity):
    """(prune_mask (N1) bool, offset_gradient_accum (N2 K, 1), offset_denom (N2 K, 1), opacity_accum (N2, 1), anchor_demon (N2, 1)): the tail
    of adjust_anchor (gpcc_densify_finish).  The offset arrays are the old ones (N0 K), the anchor arrays the grown ones (N1 >= N0)."""
    who = "adjust_anchor"
    K = n_offsets
    _tensor(offset_denom, "offset_denom", torch.float32, who)
    if offset_denom.numel() % K:
        raise ValueError(f"{who}: offset_denom holds {offset_denom.numel()} values, not a multiple of n_offsets = {K}")
    N0 = offset_denom.numel() // K
    _flat(offset_denom, "offset_denom", torch.float32, N0 * K, who)
    _flat(offset_gradient_accum, "offset_gradient_accum", torch.float32, N0 * K, who)
    _flat(offset_mask, "offset_mask", torch.bool, N0 * K, who)
    _tensor(anchor_demon, "anchor_demon", torch.float32, who)
    N1 = anchor_demon.numel()
    _flat(anchor_demon, "anchor_demon", torch.float32, N1, who)
    _flat(opacity_accum, "opacity_accum", torch.float32, N1, who)
    if N1 < N0:
        raise ValueError(f"{who}: anchor_demon has {N1} rows, fewer than the {N0} anchors of offset_denom")
    dev = _one_device(who, offset_denom, offset_gradient_accum, offset_mask, anchor_demon, opacity_accum)
    prune = torch.empty(N1, dtype=torch.bool, device=dev)
    work = runtime.Workspace(dev)
    count = ctypes.c_int64(0)
    _lib.check(_lib.lib().gpcc_densify_finish(runtime.context(dev), _ptr(offset_gradient_accum), _ptr(offset_denom), _ptr(offset_mask), N0, K,
                                              _ptr(opacity_accum), _ptr(anchor_demon), N1, float(np.float32(anchor_thr)), float(np.float32(min_opacity)),
                                              _ptr(prune), ctypes.byref(count), work.fn(), None, runtime.stream_ptr(dev)))
    n2 = count.value
    if n2 == 0:
        return (prune, *(torch.empty((0, 1), dtype=torch.float32, device=dev) for _ in range(4)))
    b = work.buffers   # allocation (1) is the ranks
    return prune, _floats(b[1], n2 * K, 1), _floats(b[2], n2 * K, 1), _floats(b[3], n2, 1), _floats(b[4], n2, 1)


# ------------------------------------------------------------------ the two methods, to be bound on a framework's GaussianModel
def training_statis(self, viewspace_point_tensor, opacity, update_filter, offset_selection_mask, anchor_visible_mask=None, pixels=0):
    """`GaussianModel.training_statis` of all four frameworks (anchor_visible_mask None: all anchors, as TC-GS allows; pixels is ignored as
    upstream ignores it).  Never waits for the host."""
    accumulate_stats(self.opacity_accum, self.anchor_demon, self.offset_gradient_accum, self.offset_denom, viewspace_point_tensor.grad, opacity,
                     update_filter, offset_selection_mask, anchor_visible_mask, self.n_offsets)


def adjust_anchor(self, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005):
    """`GaussianModel.adjust_anchor`: grads_norm and offset_mask, the framework's own `self.anchor_growing`, the new accumulators and prune
    mask in one call, the framework's own `self.prune_anchor`, and a fresh `max_radii2D`."""
    check(self.offset_denom.device)
    grads_norm, offset_mask = front(self.offset_gradient_accum, self.offset_denom, check_interval * success_threshold * 0.5)
    self.anchor_growing(grads_norm, grad_threshold, offset_mask)
    prune_mask, oga, od, oa, ad = finish(self.offset_gradient_accum, self.offset_denom, offset_mask, self.opacity_accum, self.anchor_demon, self.n_offsets,
                                         check_interval * success_threshold, min_opacity)
    self.offset_gradient_accum, self.offset_denom, self.opacity_accum, self.anchor_demon = oga, od, oa, ad
    if prune_mask.shape[0] > 0:
        self.prune_anchor(prune_mask)
    self.max_radii2D = torch.zeros((self.get_anchor.shape[0]), device=prune_mask.device)
