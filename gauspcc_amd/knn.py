"""Exact k-nearest neighbours on the device (gpcc_knn): the two call shapes of the training frameworks.

`distCUDA2` is a drop-in for the `simple_knn` extension (simple-knn.zip!simple-knn/ext.cpp, spatial.cu:16-23): the mean squared distance
to the 3 nearest other points, the value HAC, HAC++, TC-GS and CAT-3DGS set `voxel_size` and the anchors' initial scales from:

    from simple_knn._C import distCUDA2   ->   from gauspcc_amd.knn import distCUDA2

`kneighbors` is TC-GS's `init_knn_indice` (TC-GS/scene/gaussian_model.py:1052-1059), `NearestNeighbors(n_neighbors=K).fit(X).kneighbors(X)`
without the trip through the host.

Both are exact: the distance is float32 `(dx*dx + dy*dy) + dz*dz` without contraction, ties go to the smaller index, and the result
does not depend on the input's order beyond that (include/gauspcc.h, gpcc_knn).
"""
import operator

import torch

from . import _lib, runtime
from .runtime import ptr

MAX_K = 16   # gpcc_knn: neighbours per point, the point itself not counted


def _points(points, who):
    """Type, dtype and shape of `points`; these checks and _on_device's run before anything touches the device."""
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"{who}: points must be a torch.Tensor, got {type(points).__name__}")
    if points.dtype != torch.float32:
        raise TypeError(f"{who}: points must be float32, got {points.dtype}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be (P, 3), got {tuple(points.shape)}")
    return points


def _on_device(points, who):
    if not points.is_cuda:
        raise ValueError(f"{who}: points must be a CUDA tensor, got device {points.device}")
    return points.detach().contiguous()


def knn(points, k, indices=True, distances=True, mean=False):
    """gpcc_knn on checked points: (idx (P, k) int64 or None, dist2 (P, k) float32 or None, mean (P,) float32 or None)."""
    P = points.shape[0]
    dev = points.device
    idx = torch.empty((P, k), dtype=torch.int64, device=dev) if indices else None
    d2 = torch.empty((P, k), dtype=torch.float32, device=dev) if distances else None
    mn = torch.empty(P, dtype=torch.float32, device=dev) if mean else None
    if P == 0:
        return idx, d2, mn
    _lib.check(_lib.lib().gpcc_knn(runtime.context(dev), points.data_ptr(), P, int(k), ptr(idx), ptr(d2), ptr(mn),
                                    runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
    return idx, d2, mn


def distCUDA2(points):
    """simple_knn._C.distCUDA2: (P,) float32, the mean of the squared distances to the 3 nearest other points (FLT_MAX stands in for
    missing neighbours, so P = 1 and 2 give inf and P = 3 a finite value, as in simple_knn).  Non-finite coordinates raise."""
    points = _on_device(_points(points, "distCUDA2"), "distCUDA2")
    if points.shape[0] == 0:
        return torch.empty(0, dtype=torch.float32, device=points.device)
    return knn(points, 3, indices=False, distances=False, mean=True)[2]


def kneighbors(points, K):
    """NearestNeighbors(n_neighbors=K).fit(X).kneighbors(X)[1] for X = points: (P, K) int64, column 0 the point itself, columns 1.. its
    K - 1 nearest other points by increasing distance, ties by index (sklearn's result whenever no two distances tie)."""
    points = _points(points, "kneighbors")
    if isinstance(K, bool):
        raise TypeError("kneighbors: K must be an int, got bool")
    K = operator.index(K)
    if K < 1 or K > MAX_K + 1:
        raise ValueError(f"kneighbors: K = {K} outside [1, {MAX_K + 1}]")
    P = points.shape[0]
    if P < K:
        raise ValueError(f"kneighbors: expected K <= n_samples, got K = {K}, n_samples = {P}")
    points = _on_device(points, "kneighbors")
    self_col = torch.arange(P, dtype=torch.int64, device=points.device)[:, None]
    if K == 1:
        return self_col
    idx = knn(points, K - 1, indices=True, distances=False)[0]
    return torch.cat([self_col, idx], dim=1)
