"""numpy restatement of the two anchor-growing contracts (include/gauspcc.h): gpcc_scatter_max (torch_scatter.scatter_max with a
deterministic tie rule) and gpcc_grow_voxels (one grid level of HAC's anchor_growing)."""
import numpy as np

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)


def _order_key(v):
    """The contract's order of float32 values as uint64: every NaN on top, -0.0 equal to +0.0, otherwise numeric."""
    b = v.view(np.uint32).astype(np.uint64)
    b = np.where(v == 0, np.uint64(0), b)
    o = np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    return np.where(np.isnan(v), np.uint64(0xFFFFFFFF), o).astype(np.uint64)


def scatter_max(src, index, dim_size, out=None):
    """Row form: src (M, C) float32, index (M,) int in [0, dim_size).  Returns (out (S, C) float32, arg (S, C) int64).  For each slot
    and column the winner is the largest value (NaN above all, ties to the smallest row); out given: its value takes part and, when it
    wins (or when nothing beats it), arg = M.  out None: torch_scatter's own output -- an initial -FLT_MAX, then -FLT_MAX masked to 0."""
    src = np.ascontiguousarray(src, F32)
    index = np.asarray(index, np.int64).reshape(-1)
    M, C = src.shape
    S = int(dim_size)
    assert index.shape[0] == M and (M == 0 or (index.min() >= 0 and index.max() < S))
    win = np.zeros((S, C), np.uint64)
    if M:
        j = np.arange(M, dtype=np.uint64)
        key = _order_key(src) << np.uint64(32) | (np.uint64(0xFFFFFFFF) - j)[:, None]
        order = np.argsort(index, kind="stable")
        ids = index[order]
        starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
        win[ids[starts]] = np.maximum.reduceat(key[order], starts, axis=0)
    has = win != 0
    j = np.where(has, (np.uint64(0xFFFFFFFF) - (win & np.uint64(0xFFFFFFFF))).astype(np.int64), 0)
    x = src[j, np.arange(C)[None, :]] if M else np.zeros((S, C), F32)
    v = np.array(out, F32, copy=True) if out is not None else np.full((S, C), -FLT_MAX, F32)
    with np.errstate(invalid="ignore"):
        take = has & (np.isnan(x) | ~(np.isnan(v) | (v > x)))
    value = np.where(take, x, v)
    arg = np.where(take, j, M).astype(np.int64)
    if out is None:
        value = np.where(value == -FLT_MAX, F32(0), value).astype(F32)
    return value.astype(F32), arg


def voxels(x, inv):
    """rint(x * inv) per axis in float32 as int32; raises ValueError where that is not finite or not an int32."""
    t = np.asarray(x, F32) * F32(inv)
    r = np.rint(t)
    ok = np.isfinite(r) & (r >= -2147483648.0) & (r < 2147483648.0)
    if not ok.all():
        raise ValueError("voxel outside int32")
    return r.astype(np.int32)


def grow(xyz, anchors, inv, size, feats, rows=None):
    """(new_anchor (U, 3), new_feat (U, C)): unique candidate voxels without an anchor voxel, lexicographic signed order."""
    feats = np.asarray(feats, F32)
    C = feats.shape[1]
    g = voxels(xyz, inv).reshape(-1, 3)
    a = voxels(anchors, inv).reshape(-1, 3)
    if g.shape[0] == 0:
        return np.zeros((0, 3), F32), np.zeros((0, C), F32)
    uniq, inverse = np.unique(g, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    rec = np.dtype([("x", np.int32), ("y", np.int32), ("z", np.int32)])
    ua = np.ascontiguousarray(uniq).view(rec).reshape(-1)
    aa = np.sort(np.ascontiguousarray(a).view(rec).reshape(-1))
    pos = np.searchsorted(aa, ua)
    member = (pos < aa.shape[0]) & (aa[np.minimum(pos, max(aa.shape[0] - 1, 0))] == ua) if aa.shape[0] else np.zeros(ua.shape[0], bool)
    keep = ~member
    f = feats[np.asarray(rows, np.int64)] if rows is not None else feats
    val, _ = scatter_max(f, inverse, uniq.shape[0])
    return (uniq[keep].astype(F32) * F32(size)).astype(F32), val[keep]
