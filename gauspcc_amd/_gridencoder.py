"""Drop-in for HAC's `_gridencoder` extension (gridencoder.zip!gridencoder/src/bindings.cpp): `grid_encode_forward` and
`grid_encode_backward` with the extension's positional arguments, filling the caller's torch tensors in place.  With it the
reference's own `_grid_encode`, `STE_binary` and `GridEncoder` (HAC/utils/encodings.py) train unchanged:

    import _gridencoder as _backend   ->   from gauspcc_amd import _gridencoder as _backend

The backward adds into `grad_embeddings` like the reference's kernel, but without float atomics: two runs give the same bits
(gsge_backward).  When `dy_dx` is passed, `grad_inputs` is computed; its values are recomputed from the inputs by the same device code
that wrote `dy_dx`.  `PV` and `max_level` are accepted and ignored, as in the reference.  float32 only (no autocast half embeddings).
"""
import torch

from . import _lib, runtime
from .runtime import ptr


def _need(t, name, dtype):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"_gridencoder: {name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"_gridencoder: {name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise ValueError(f"_gridencoder: {name} must be contiguous")
    if t.dtype != dtype:
        raise TypeError(f"_gridencoder: {name} must be {dtype}, got {t.dtype}")
    return t


def _numel(t, name, n):
    if t.numel() != n:
        raise ValueError(f"_gridencoder: {name} has {t.numel()} elements, expected {n}")


def _tables(inputs, embeddings, offsets_list, resolutions_list, N, num_dim, n_features, n_levels, binary_vxl, min_level_id):
    """Checks shared by both directions; returns (binary_vxl as uint8 or None, min_level_id or None)."""
    _need(inputs, "inputs", torch.float32)
    _need(embeddings, "embeddings", torch.float32)
    _need(offsets_list, "offsets_list", torch.int32)
    _need(resolutions_list, "resolutions_list", torch.int32)
    if inputs.dim() != 2 or tuple(inputs.shape) != (N, num_dim):
        raise ValueError(f"_gridencoder: inputs must be ({N}, {num_dim}), got {tuple(inputs.shape)}")
    if embeddings.dim() != 2 or embeddings.shape[1] != n_features:
        raise ValueError(f"_gridencoder: embeddings must be (rows, {n_features}), got {tuple(embeddings.shape)}")
    need_levels = n_levels
    if min_level_id is not None:
        _need(min_level_id, "min_level_id", torch.int32)
        _numel(min_level_id, "min_level_id", N)
        if N > 0:
            lo, hi = int(min_level_id.min()), int(min_level_id.max())
            if lo < 0:
                raise ValueError("_gridencoder: min_level_id must be >= 0")
            need_levels = hi + n_levels
    if resolutions_list.numel() < need_levels or offsets_list.numel() < need_levels + 1:
        raise ValueError(f"_gridencoder: offsets / resolutions describe fewer than the {need_levels} levels used")
    bv = None
    if binary_vxl is not None:
        if binary_vxl.dtype == torch.bool:
            binary_vxl = binary_vxl.view(torch.uint8)
        bv = _need(binary_vxl, "binary_vxl", torch.uint8)
        if bv.dim() != num_dim or any(s != bv.shape[-1] for s in bv.shape):
            raise ValueError(f"_gridencoder: binary_vxl must be a {num_dim}-d cube, got {tuple(bv.shape)}")
    return bv, min_level_id


def forward_into(inputs, embeddings, offsets, resolutions, outputs, n_features, n_levels, Rb, bv, ml, dy_dx=None):
    """gsge_forward (dy_dx None) or gsge_forward_train into `outputs` (L, N, F) and `dy_dx` (N, L, D, F); tensors already checked."""
    N, num_dim = inputs.shape
    dev = inputs.device
    args = (runtime.context(dev), inputs.data_ptr(), embeddings.data_ptr(), offsets.data_ptr(), resolutions.data_ptr(), outputs.data_ptr(),
            N, num_dim, n_features, n_levels, Rb, ptr(bv), ptr(ml))
    if dy_dx is None:
        _lib.check(_lib.lib().gsge_forward(*args, runtime.stream_ptr(dev)))
    else:
        _lib.check(_lib.lib().gsge_forward_train(*args, dy_dx.data_ptr(), runtime.stream_ptr(dev)))


def backward_into(grad, inputs, embeddings, offsets, resolutions, grad_embeddings, grad_inputs, n_features, n_levels, Rb, bv, ml):
    """gsge_backward: adds into grad_embeddings (rows, F), overwrites grad_inputs (N, D) unless None; tensors already checked."""
    N, num_dim = inputs.shape
    dev = inputs.device
    _lib.check(_lib.lib().gsge_backward(runtime.context(dev), grad.data_ptr(), inputs.data_ptr(), embeddings.data_ptr(), offsets.data_ptr(),
                                        resolutions.data_ptr(), embeddings.shape[0], grad_embeddings.data_ptr(), ptr(grad_inputs), N, num_dim,
                                        n_features, n_levels, Rb, ptr(bv), ptr(ml), runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))


def grid_encode_forward(inputs, embeddings, offsets_list, resolutions_list, outputs, N, num_dim, n_features, n_levels, max_level, Rb, PV,
                        dy_dx=None, binary_vxl=None, min_level_id=None):
    """bindings.cpp grid_encode_forward: outputs (n_levels, N, n_features); dy_dx (N, n_levels * num_dim * n_features) or None."""
    N, num_dim, n_features, n_levels, Rb = int(N), int(num_dim), int(n_features), int(n_levels), int(Rb)
    bv, ml = _tables(inputs, embeddings, offsets_list, resolutions_list, N, num_dim, n_features, n_levels, binary_vxl, min_level_id)
    _need(outputs, "outputs", torch.float32)
    _numel(outputs, "outputs", n_levels * N * n_features)
    if dy_dx is not None:
        _need(dy_dx, "dy_dx", torch.float32)
        _numel(dy_dx, "dy_dx", N * n_levels * num_dim * n_features)
    forward_into(inputs, embeddings, offsets_list, resolutions_list, outputs, n_features, n_levels, Rb, bv, ml, dy_dx)


def grid_encode_backward(grad, inputs, embeddings, offsets_list, resolutions_list, grad_embeddings, N, num_dim, n_features, n_levels, max_level, Rb,
                         dy_dx=None, grad_inputs=None, binary_vxl=None, min_level_id=None):
    """bindings.cpp grid_encode_backward: grad (n_levels, N, n_features); adds into grad_embeddings; grad_inputs (N, num_dim) when dy_dx is given."""
    N, num_dim, n_features, n_levels, Rb = int(N), int(num_dim), int(n_features), int(n_levels), int(Rb)
    bv, ml = _tables(inputs, embeddings, offsets_list, resolutions_list, N, num_dim, n_features, n_levels, binary_vxl, min_level_id)
    _need(grad, "grad", torch.float32)
    _numel(grad, "grad", n_levels * N * n_features)
    _need(grad_embeddings, "grad_embeddings", torch.float32)
    if grad_embeddings.shape != embeddings.shape:
        raise ValueError(f"_gridencoder: grad_embeddings must be {tuple(embeddings.shape)}, got {tuple(grad_embeddings.shape)}")
    gi = None
    if dy_dx is not None and grad_inputs is not None:
        gi = _need(grad_inputs, "grad_inputs", torch.float32)
        _numel(gi, "grad_inputs", N * num_dim)
    backward_into(grad, inputs, embeddings, offsets_list, resolutions_list, grad_embeddings, gi, n_features, n_levels, Rb, bv, ml)
