"""gpcc_scatter_max and gpcc_grow_voxels on the device: bit-exact against the numpy restatement (tests/grow_ref.py) across sizes, widths,
skewed and degenerate clouds, NaN / signed zero / -FLT_MAX features and both key paths; the torch_scatter call shapes and the backward;
GPCC_ERR_ARG with outputs untouched; determinism across runs and streams; the one-voxel case in linear time; and a HAC-shaped model
against the reference's torch sequence run on the GPU."""
import time

import numpy as np
import pytest
import torch

from gauspcc_amd import _lib
from gauspcc_amd.growing import grow_voxels
from gauspcc_amd.scatter import scatter_max, scatter_max_rows
from tests import grow_ref
from tests.grow_ref import FLT_MAX

pytestmark = pytest.mark.gpu
F32 = np.float32

SIZES = [0, 1, 63, 64, 65, 4095, 4097, 100_000, 1_000_000]
WIDTHS = [1, 3, 50, 64, 257]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _feats(rng, M, C):
    f = rng.standard_normal((M, C)).astype(F32)
    if M * C:
        special = np.array([np.nan, 0.0, -0.0, -FLT_MAX, -np.inf], F32)
        k = max(1, M * C // 20)
        f.reshape(-1)[rng.integers(0, M * C, k)] = special[rng.integers(0, len(special), k)]
    return f


def _pairs():
    for M in SIZES:
        for C in WIDTHS:
            if M * C <= 30_000_000:
                yield M, C


@pytest.mark.parametrize("M,C", list(_pairs()))
def test_scatter_rows_bit_exact(M, C):
    rng = np.random.default_rng(M * 7 + C)
    S = max(1, M // 7)
    src = _feats(rng, M, C)
    index = rng.integers(0, S, M)
    if M > 100:
        index[: M // 3] = 0   # one slot holding a third of the rows
    v, a = scatter_max_rows(torch.tensor(src, device="cuda"), torch.tensor(index, device="cuda"), S)
    rv, ra = grow_ref.scatter_max(src, index, S)
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(rv)) and np.array_equal(a.cpu().numpy(), ra)


@pytest.mark.parametrize("M", [0, 65, 4097, 100_000])
def test_scatter_out_include_self(M):
    rng = np.random.default_rng(M + 1)
    C, S = 5, 300
    src = _feats(rng, M, C)
    index = rng.integers(0, S, M)
    init = _feats(rng, S, C)
    out = torch.tensor(init, device="cuda")
    res, arg = scatter_max(torch.tensor(src, device="cuda"), torch.tensor(index, device="cuda").unsqueeze(1).expand(-1, C), dim=0, out=out)
    rv, ra = grow_ref.scatter_max(src, index, S, init)
    assert res.data_ptr() == out.data_ptr()
    assert np.array_equal(_bits(res.cpu().numpy()), _bits(rv)) and np.array_equal(arg.cpu().numpy(), ra)


def test_scatter_torch_scatter_shapes():
    rng = np.random.default_rng(3)
    src = _feats(rng, 6, 40).reshape(6, 40)
    d = torch.tensor(src, device="cuda")
    # dim = -1 with a 1-D index (torch_scatter's default), dim_size given and defaulted
    idx = rng.integers(0, 9, 40)
    ti = torch.tensor(idx, device="cuda")
    for ds in (None, 12):
        v, a = scatter_max(d, ti, dim_size=ds)
        S = ds or int(idx.max()) + 1
        rv, ra = grow_ref.scatter_max(src.T, idx, S)
        assert v.shape == (6, S) and np.array_equal(_bits(v.cpu().numpy()), _bits(rv.T)) and np.array_equal(a.cpu().numpy(), ra.T)
    # a full 2-D index, its own index per column
    full = rng.integers(0, 4, (6, 40))
    v, a = scatter_max(d, torch.tensor(full, device="cuda"), dim=0)
    S = int(full.max()) + 1
    for c in range(40):
        rv, ra = grow_ref.scatter_max(src[:, c:c + 1], full[:, c], S)
        assert np.array_equal(_bits(v[:, c].cpu().numpy()), _bits(rv[:, 0])) and np.array_equal(a[:, c].cpu().numpy(), ra[:, 0])
    # a 3-D source, dim 1
    s3 = _feats(rng, 24, 5).reshape(2, 12, 5)
    i1 = rng.integers(0, 4, 12)
    v, a = scatter_max(torch.tensor(s3, device="cuda"), torch.tensor(i1, device="cuda"), dim=1)
    flat = np.moveaxis(s3, 1, 0).reshape(12, 10)
    rv, ra = grow_ref.scatter_max(flat, i1, 4)
    assert np.array_equal(_bits(np.moveaxis(v.cpu().numpy(), 1, 0).reshape(4, 10)), _bits(rv))
    assert np.array_equal(np.moveaxis(a.cpu().numpy(), 1, 0).reshape(4, 10), ra)


def test_scatter_backward():
    rng = np.random.default_rng(5)
    src = torch.tensor(rng.standard_normal((300, 8)).astype(F32), device="cuda", requires_grad=True)
    idx = torch.tensor(rng.integers(0, 40, 300), device="cuda")
    v, a = scatter_max(src, idx.unsqueeze(1).expand(-1, 8), dim=0, dim_size=50)
    g = torch.randn_like(v)
    (v * g).sum().backward()
    want = torch.zeros(301, 8, device="cuda")
    want.scatter_(0, a, g)
    assert torch.equal(src.grad, want[:300])
    assert (a[40:] == 300).all()


def test_scatter_bad_index_leaves_outputs():
    src = torch.ones(100, 3, device="cuda")
    for bad in (-1, 10):
        idx = torch.zeros(100, dtype=torch.int64, device="cuda")
        idx[57] = bad
        out = torch.full((10, 3), 7.0, device="cuda")
        with pytest.raises(_lib.GpccError):
            scatter_max(src, idx.unsqueeze(1).expand(-1, 3), dim=0, out=out)
        assert (out == 7.0).all()


# ------------------------------------------------------------------ grow_voxels
def _cloud(kind, M, rng):
    if kind == "random":
        return (rng.standard_normal((M, 3)) * 3).astype(F32), 0.1
    if kind == "one_voxel":
        return (rng.random((M, 3)) * 0.4 - 0.2).astype(F32) + F32(5.0), 1.0
    if kind == "own_voxel":
        g = rng.permutation(M * 2)[:M]
        return np.stack([g % 211, (g // 211) % 199, g // (211 * 199)], 1).astype(F32) * F32(0.5) - F32(40.0), 0.5
    if kind == "negative":
        return (-rng.random((M, 3)) * 50).astype(F32), 0.25
    if kind == "half":
        return (rng.integers(-40, 40, (M, 3)) + 0.5).astype(F32) * F32(0.5), 0.5   # exactly on .5 boundaries of the voxel grid
    if kind == "wide":
        x = (rng.standard_normal((M, 3)) * 3).astype(F32)
        x[::3, 0] += F32(3.0e6)   # span beyond 2^21 voxels on x: the general key path
        x[1::3, 2] -= F32(2.5e6)
        return x, 1.0
    raise KeyError(kind)


def _anchors(kind, xyz, rng, size):
    M = xyz.shape[0]
    if kind == "none":
        return np.zeros((0, 3), F32)
    if kind == "all":
        return xyz[rng.permutation(M)].copy() if M else np.zeros((0, 3), F32)
    a = xyz[rng.integers(0, max(M, 1), max(M // 3, 1))].copy() if M else np.zeros((5, 3), F32)
    return np.concatenate([a, (rng.standard_normal((M // 2 + 7, 3)) * 3).astype(F32)])


def _run_grow(xyz, anchors, size, feats, rows=None):
    d = lambda a: torch.tensor(a, device="cuda")   # noqa: E731
    na, nf = grow_voxels(d(xyz), d(anchors), size, d(feats), None if rows is None else d(rows))
    return na.cpu().numpy(), nf.cpu().numpy()


def _check_grow(xyz, anchors, size, feats, rows=None):
    s = F32(size)
    ra, rf = grow_ref.grow(xyz, anchors, F32(1.0) / s, s, feats, rows)
    na, nf = _run_grow(xyz, anchors, size, feats, rows)
    assert na.shape == ra.shape and nf.shape == rf.shape
    assert np.array_equal(_bits(na), _bits(ra)) and np.array_equal(_bits(nf), _bits(rf))
    return na.shape[0]


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("kind", ["random", "one_voxel", "own_voxel", "negative", "half", "wide"])
def test_grow_bit_exact(kind, M):
    rng = np.random.default_rng(M + len(kind))
    xyz, size = _cloud(kind, M, rng)
    C = 50 if M <= 100_000 else 3
    feats = _feats(rng, M, C)
    _check_grow(xyz, _anchors("some", xyz, rng, size), size, feats)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("anchors", ["none", "all", "some"])
def test_grow_widths_rows_anchors(C, anchors):
    rng = np.random.default_rng(C)
    M = 20_000
    xyz, size = _cloud("random", M, rng)
    table = _feats(rng, 3000, C)
    rows = rng.integers(0, 3000, M)
    U = _check_grow(xyz, _anchors(anchors, xyz, rng, size), size, table, rows)
    if anchors == "all":
        assert U == 0


def test_grow_bad_input():
    x = torch.zeros(100, 3, device="cuda")
    a = torch.zeros(3, 3, device="cuda")
    f = torch.zeros(100, 4, device="cuda")
    for bad in (float("nan"), float("inf"), 1e12):
        y = x.clone()
        y[42, 1] = bad
        with pytest.raises(_lib.GpccError):
            grow_voxels(y, a, 0.1, f)
        b = a.clone()
        b[1, 2] = bad
        with pytest.raises(_lib.GpccError):
            grow_voxels(x + 1, b, 0.1, f)
    with pytest.raises(_lib.GpccError):
        grow_voxels(x, a, 0.1, f, rows=torch.full((100,), 100, dtype=torch.int64, device="cuda"))


def test_determinism_and_streams():
    rng = np.random.default_rng(11)
    xyz, size = _cloud("random", 200_000, rng)
    xyz = torch.tensor(xyz, device="cuda")
    anchors = torch.tensor(_anchors("some", xyz.cpu().numpy(), rng, size), device="cuda")
    feats = torch.tensor(_feats(rng, 200_000, 50), device="cuda")
    idx = torch.tensor(rng.integers(0, 5000, 200_000), device="cuda")
    base = [t.clone() for t in grow_voxels(xyz, anchors, size, feats)] + list(scatter_max(feats, idx, dim=0, dim_size=5000))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for s in streams:
        with torch.cuda.stream(s):
            got.append(list(grow_voxels(xyz, anchors, size, feats)) + list(scatter_max(feats, idx, dim=0, dim_size=5000)))
    torch.cuda.synchronize()
    for g in got + [list(grow_voxels(xyz, anchors, size, feats)) + list(scatter_max(feats, idx, dim=0, dim_size=5000))]:
        for x, y in zip(base, g):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def _time(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def test_one_voxel_linear_time():
    rng = np.random.default_rng(2)
    t = {}
    for M in (100_000, 1_000_000):
        x = torch.tensor((rng.random((M, 3)) * 0.1).astype(F32), device="cuda")
        f = torch.tensor(rng.standard_normal((M, 50)).astype(F32), device="cuda")
        z = torch.zeros(M, dtype=torch.int64, device="cuda")
        a = torch.zeros(0, 3, device="cuda")
        t[M] = (_time(lambda: grow_voxels(x, a, 1.0, f)), _time(lambda: scatter_max(f, z, dim=0)))
    for k in range(2):
        assert t[1_000_000][k] < 30 * t[100_000][k] + 2e-3, t


def test_hac_shaped_model_against_torch_sequence():
    """anchor_growing's body (HAC/scene/gaussian_model.py:836-874) restated in torch on the GPU, at 2e5 anchors, 10 offsets, feat_dim 50 and
    HAC's three levels; scatter_max restated as scatter_reduce("amax") on a -FLT_MAX start masked to 0 (torch_scatter's own output)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    N, K, F = 200_000, 10, 50
    voxel_size = 0.01
    anchor = torch.round(torch.rand(N, 3, device="cuda", generator=g) * 8 / voxel_size) * voxel_size
    offset = torch.randn(N, K, 3, device="cuda", generator=g) * 0.5
    scaling = torch.rand(N, 3, device="cuda", generator=g) * 0.05
    feat = torch.randn(N, F, device="cuda", generator=g)
    mask = torch.rand(N * K, device="cuda", generator=g) > 0.9
    all_xyz = anchor.unsqueeze(1) + offset * scaling.unsqueeze(1)
    for i in range(3):
        cur_size = voxel_size * (16 // 4 ** i)
        grid_coords = torch.round(anchor / cur_size).int()
        selected_xyz = all_xyz.view(-1, 3)[mask]
        sel = torch.round(selected_xyz / cur_size).int()
        uniq, inverse = torch.unique(sel, return_inverse=True, dim=0)
        dup = torch.zeros(uniq.shape[0], dtype=torch.bool, device="cuda")
        for c in range(0, grid_coords.shape[0], 4096):
            dup |= (uniq.unsqueeze(1) == grid_coords[c:c + 4096]).all(-1).any(-1)
        keep = ~dup
        candidate_anchor = uniq[keep] * cur_size
        new_feat = feat.unsqueeze(1).repeat(1, K, 1).view(-1, F)[mask]
        m = torch.full((uniq.shape[0], F), float(-FLT_MAX), device="cuda").scatter_reduce(0, inverse.unsqueeze(1).expand(-1, F), new_feat, "amax",
                                                                                         include_self=False)
        m = m.masked_fill(m == float(-FLT_MAX), 0.0)[keep]
        rows = torch.nonzero(mask).squeeze(1) // K
        na, nf = grow_voxels(selected_xyz, anchor, cur_size, feat, rows)
        assert candidate_anchor.shape[0] > 0
        assert torch.equal(na.view(torch.int32), candidate_anchor.contiguous().view(torch.int32))
        assert torch.equal(nf.view(torch.int32), m.contiguous().view(torch.int32))
        # and through the drop-in, as the reference calls it
        v = scatter_max(new_feat, inverse.unsqueeze(1).expand(-1, F), dim=0)[0][keep]
        assert torch.equal(v.view(torch.int32), m.contiguous().view(torch.int32))
