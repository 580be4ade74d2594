"""One grid level of anchor growing on the device (gpcc_grow_voxels): the body of `anchor_growing`'s loop in HAC, HAC++, TC-GS and
CAT-3DGS (e.g. HAC/scene/gaussian_model.py:823-911) from `selected_xyz` up to `candidate_anchor` and the features'
`scatter_max(...)[0][remove_duplicates]`, in linear time: the candidates' voxels are sorted once, the anchored ones found by a binary
search in the sorted anchor voxels, and the features maximised per voxel without materialising the repeated feature table.

The result is bit-identical to that torch sequence on the GPU (include/gauspcc.h, gpcc_grow_voxels).  INTEGRATION.md shows the loop
rewritten around it.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, runtime


def _tensor(t, name, dtype, ndim, cols=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"grow_voxels: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"grow_voxels: {name} must be {dtype}, got {t.dtype}")
    if t.dim() != ndim or (cols is not None and t.shape[1] != cols):
        want = f"({name[0].upper()}, {cols})" if cols is not None else f"{ndim}-D"
        raise ValueError(f"grow_voxels: {name} must be {want}, got {tuple(t.shape)}")
    return t


def grow_voxels(xyz, anchors, cur_size, feats, rows=None):
    """(new_anchor (U, 3), new_feat (U, C)) float32, detached: the unique voxels of size cur_size holding a candidate of xyz (M, 3) and no
    anchor of anchors (N, 3), in torch.unique(dim=0) order; new_anchor = voxel * cur_size and new_feat = the elementwise maximum of
    feats[rows[j]] (rows None: feats[j]) over the voxel's candidates, -FLT_MAX set to 0 (torch_scatter).  A non-finite coordinate, a voxel
    outside int32 or a row outside feats raises."""
    _tensor(xyz, "xyz", torch.float32, 2, 3)
    _tensor(anchors, "anchors", torch.float32, 2, 3)
    _tensor(feats, "feats", torch.float32, 2)
    if rows is not None:
        _tensor(rows, "rows", torch.int64, 1)
        if rows.shape[0] != xyz.shape[0]:
            raise ValueError(f"grow_voxels: rows has {rows.shape[0]} entries for {xyz.shape[0]} candidates")
    elif feats.shape[0] != xyz.shape[0]:
        raise ValueError(f"grow_voxels: feats has {feats.shape[0]} rows for {xyz.shape[0]} candidates and no rows given")
    if isinstance(cur_size, bool) or not isinstance(cur_size, (int, float)):
        raise TypeError(f"grow_voxels: cur_size must be a Python number, got {type(cur_size).__name__}")
    if not math.isfinite(cur_size) or cur_size <= 0:
        raise ValueError(f"grow_voxels: cur_size must be finite and positive, got {cur_size}")
    if feats.shape[1] < 1:
        raise ValueError("grow_voxels: feats needs at least one column")
    for name, t in (("xyz", xyz), ("anchors", anchors), ("feats", feats), ("rows", rows)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"grow_voxels: {name} must be a CUDA tensor, got device {t.device}")
    dev = xyz.device
    if any(t is not None and t.device != dev for t in (anchors, feats, rows)):
        raise ValueError("grow_voxels: xyz, anchors, feats and rows must be on one device")
    # torch on the GPU: `x / size` multiplies by the float32 reciprocal of the CPU scalar, `int * size` multiplies by float32(size)
    size = np.float32(cur_size)
    inv = np.float32(1.0) / size
    xyz, anchors, feats = (t.detach().contiguous() for t in (xyz, anchors, feats))
    rows = rows.detach().contiguous() if rows is not None else None
    M, N, (R, C) = xyz.shape[0], anchors.shape[0], feats.shape
    work = runtime.Workspace(dev)
    count = ctypes.c_int64(0)

    def ptr(t):   # NULL for an empty tensor too
        return None if t is None or t.numel() == 0 else t.data_ptr()

    _lib.check(_lib.lib().gpcc_grow_voxels(runtime.context(dev), ptr(xyz), M, ptr(rows), ptr(feats), R, C, ptr(anchors), N, float(inv), float(size),
                                           ctypes.byref(count), work.fn(), None, runtime.stream_ptr(dev)))
    U = count.value
    if U == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, C), dtype=torch.float32, device=dev)
    blk = work.buffers[1]   # allocation (2): anchors at 0, features at (12 U + 255) & ~255
    off = (12 * U + 255) & ~255
    new_anchor = blk[:12 * U].view(torch.float32).view(U, 3)
    new_feat = blk[off:off + 4 * U * C].view(torch.float32).view(U, C)
    return new_anchor, new_feat
