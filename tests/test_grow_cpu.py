"""The anchor-growing restatement (tests/grow_ref.py) against torch's CPU ops on small clouds, and the device shims' argument checks and
signatures (no device needed: every check runs before the device is touched)."""
import inspect

import numpy as np
import pytest
import torch

from tests import grow_ref
from tests.grow_ref import FLT_MAX

F32 = np.float32


def _brute(src, index, S, out=None):
    """The contract slot by slot, in plain Python."""
    M, C = src.shape
    val = np.zeros((S, C), F32)
    arg = np.full((S, C), M, np.int64)
    for s in range(S):
        G = [j for j in range(M) if index[j] == s]
        for c in range(C):
            vals = [src[j, c] for j in G]
            init = out[s, c] if out is not None else -FLT_MAX
            nan_j = [j for j in G if np.isnan(src[j, c])]
            if nan_j:
                val[s, c], arg[s, c] = src[nan_j[0], c], nan_j[0]
                continue
            if np.isnan(init):
                val[s, c] = init
                continue
            m = max(vals + [init])
            hit = [j for j in G if src[j, c] == m]
            if hit:
                val[s, c], arg[s, c] = src[hit[0], c], hit[0]
            else:
                val[s, c] = init
            if out is None and val[s, c] == -FLT_MAX:
                val[s, c] = 0.0
    return val, arg


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("with_out", [False, True])
def test_scatter_ref_matches_brute(seed, with_out):
    rng = np.random.default_rng(seed)
    M, C, S = int(rng.integers(0, 40)), int(rng.integers(1, 5)), int(rng.integers(1, 9))
    pool = np.array([0.0, -0.0, 1.0, -1.0, 2.5, np.nan, -FLT_MAX, -np.inf, np.inf], F32)
    src = pool[rng.integers(0, len(pool), (M, C))]
    index = rng.integers(0, S, M)
    out = pool[rng.integers(0, len(pool), (S, C))] if with_out else None
    v, a = grow_ref.scatter_max(src, index, S, out)
    bv, ba = _brute(src, index, S, out)
    assert np.array_equal(_bits(v), _bits(bv)) and np.array_equal(a, ba)


@pytest.mark.parametrize("seed", range(4))
def test_scatter_ref_matches_torch_amax(seed):
    rng = np.random.default_rng(seed)
    M, C, S = 500, 7, 60
    src = rng.standard_normal((M, C)).astype(F32)
    index = rng.integers(0, S, M)
    v, a = grow_ref.scatter_max(src, index, S)
    t = torch.full((S, C), float(-FLT_MAX)).scatter_reduce(0, torch.tensor(index)[:, None].expand(-1, C), torch.tensor(src), "amax", include_self=False)
    t = t.masked_fill(t == float(-FLT_MAX), 0.0).numpy()
    assert np.array_equal(_bits(v), _bits(t))
    for s in range(S):
        for c in range(C):
            G = np.flatnonzero(index == s)
            want = G[src[G, c] == v[s, c]].min() if len(G) else M
            assert a[s, c] == want


def _torch_grow(xyz, anchors, cur_size, feats):
    """The reference's loop body in torch CPU ops (broadcast membership instead of the chunks)."""
    g = torch.round(xyz / cur_size).int()
    ga = torch.round(anchors / cur_size).int()
    uniq, inv = torch.unique(g, return_inverse=True, dim=0)
    dup = (uniq.unsqueeze(1) == ga).all(-1).any(-1) if ga.shape[0] else torch.zeros(uniq.shape[0], dtype=torch.bool)
    keep = ~dup
    C = feats.shape[1]
    m = torch.full((uniq.shape[0], C), float(-FLT_MAX)).scatter_reduce(0, inv[:, None].expand(-1, C), feats, "amax", include_self=False)
    m = m.masked_fill(m == float(-FLT_MAX), 0.0)
    return uniq[keep] * cur_size, m[keep]


@pytest.mark.parametrize("seed", range(6))
def test_grow_ref_matches_torch(seed):
    rng = np.random.default_rng(seed)
    M, N, C = int(rng.integers(1, 400)), int(rng.integers(0, 300)), int(rng.integers(1, 6))
    cur_size = float(rng.choice([0.5, 0.25, 0.1, 0.037]))
    xyz = (rng.standard_normal((M, 3)) * 2).astype(F32)
    xyz[: M // 4] = np.round(xyz[: M // 4] * 2) / 2 + 0.25 * (rng.integers(0, 2, (M // 4, 3)) * 2 - 1)   # some on .5 boundaries at size 0.5
    anchors = (rng.standard_normal((N, 3)) * 2).astype(F32)
    feats = rng.standard_normal((M, C)).astype(F32)
    size = F32(cur_size)
    inv = F32(1.0) / size
    # torch on the CPU divides; the restatement multiplies by inv (the GPU's form): compare on inputs where both agree
    q = np.rint(xyz * inv) == np.rint(xyz / size)
    xyz = xyz[q.all(1)]
    feats = feats[q.all(1)]
    qa = np.rint(anchors * inv) == np.rint(anchors / size)
    anchors = anchors[qa.all(1)]
    na, nf = grow_ref.grow(xyz, anchors, inv, size, feats)
    ta, tf = _torch_grow(torch.tensor(xyz), torch.tensor(anchors), cur_size, torch.tensor(feats))
    assert np.array_equal(_bits(na), _bits(ta.numpy())) and np.array_equal(_bits(nf), _bits(tf.numpy()))
    # rows form: the same features through an index
    rows = rng.permutation(xyz.shape[0])
    table = np.empty_like(feats)
    table[rows] = feats
    ra, rf = grow_ref.grow(xyz, anchors, inv, size, table, rows)
    assert np.array_equal(_bits(ra), _bits(na)) and np.array_equal(_bits(rf), _bits(nf))


def test_grow_ref_rejects_non_finite():
    with pytest.raises(ValueError):
        grow_ref.voxels(np.array([[np.nan, 0, 0]], F32), 1.0)
    with pytest.raises(ValueError):
        grow_ref.voxels(np.array([[3e9, 0, 0]], F32), 1.0)


def test_scatter_max_signature():
    from gauspcc_amd.scatter import scatter_max

    p = inspect.signature(scatter_max).parameters
    assert list(p) == ["src", "index", "dim", "out", "dim_size"]
    assert p["dim"].default == -1 and p["out"].default is None and p["dim_size"].default is None


def test_grow_voxels_signature():
    from gauspcc_amd.growing import grow_voxels

    assert list(inspect.signature(grow_voxels).parameters) == ["xyz", "anchors", "cur_size", "feats", "rows"]


def test_scatter_max_checks():
    from gauspcc_amd.scatter import scatter_max

    src = torch.zeros(4, 2)
    idx = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError):
        scatter_max(src.double(), idx, 0)
    with pytest.raises(TypeError):
        scatter_max(src, idx.int(), 0)
    with pytest.raises(TypeError):
        scatter_max(src.numpy(), idx, 0)
    with pytest.raises(ValueError):
        scatter_max(src, idx, 0)   # CPU tensors: no CPU path
    with pytest.raises(ValueError):
        scatter_max(src, idx, 0, dim_size=-1)


def test_grow_voxels_checks():
    from gauspcc_amd.growing import grow_voxels

    x = torch.zeros(5, 3)
    a = torch.zeros(2, 3)
    f = torch.zeros(5, 4)
    with pytest.raises(TypeError):
        grow_voxels(x.double(), a, 0.1, f)
    with pytest.raises(ValueError):
        grow_voxels(torch.zeros(5, 2), a, 0.1, f)
    with pytest.raises(TypeError):
        grow_voxels(x, a, torch.tensor(0.1), f)
    with pytest.raises(ValueError):
        grow_voxels(x, a, 0.0, f)
    with pytest.raises(ValueError):
        grow_voxels(x, a, float("nan"), f)
    with pytest.raises(ValueError):
        grow_voxels(x, a, 0.1, torch.zeros(4, 4))   # no rows: one feature row per candidate
    with pytest.raises(TypeError):
        grow_voxels(x, a, 0.1, f, rows=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError):
        grow_voxels(x, a, 0.1, f, rows=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        grow_voxels(x, a, 0.1, f)   # CPU tensors: no CPU path
