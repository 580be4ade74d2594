"""gpcc_knn on the device: bit-exact against the numpy restatement of its contract (tests/knn_ref.py) on clouds with ties, degenerate
shapes and overflowing distances; the all-equal cloud in linear time; non-finite input; determinism and streams; the workspace bound;
and the two call shapes of the frameworks (HAC's distCUDA2 median and scales, TC-GS's kneighbors)."""
import functools
import time

import numpy as np
import pytest
import torch

from gauspcc_amd import _lib
from gauspcc_amd.knn import distCUDA2, kneighbors, knn
from tests import knn_ref
from tests.knn_ref import CLOUDS, make_cloud

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 4095, 4097, 100_000, 1_000_000]
KS = [1, 3, 4, 16]
FLT_MAX = np.float32(np.finfo(np.float32).max)


@functools.lru_cache(maxsize=None)
def _ref16(kind, n):
    pts = make_cloud(kind, n)
    j, d, _ = knn_ref.knn(pts, 16)
    return pts, j, d


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(kind, n, k):
    pts, j16, d16 = _ref16(kind, n)
    j, d = j16[:, :k], d16[:, :k]
    m = knn_ref.mean_of(d)
    x = torch.tensor(pts, device="cuda")
    gi, gd, gm = knn(x, k, indices=True, distances=True, mean=True)
    _, hd, hm = knn(x, k, indices=False, distances=True, mean=True)   # the distance-only search
    gi, gd, gm, hd, hm = (t.cpu().numpy() for t in (gi, gd, gm, hd, hm))
    bad = np.nonzero(np.any(gi != j, axis=1))[0]
    assert len(bad) == 0, f"{kind} n={n} k={k}: {len(bad)} rows differ, first {bad[0]}: {gi[bad[0]]} vs {j[bad[0]]} ({gd[bad[0]]} vs {d[bad[0]]})"
    assert np.array_equal(_bits(gd), _bits(d)) and np.array_equal(_bits(hd), _bits(d)), f"{kind} n={n} k={k}: distances"
    assert np.array_equal(_bits(gm), _bits(m)) and np.array_equal(_bits(hm), _bits(m)), f"{kind} n={n} k={k}: mean"
    if k == 3:
        assert np.array_equal(_bits(distCUDA2(x).cpu().numpy()), _bits(m))


@pytest.mark.parametrize("kind", CLOUDS)
@pytest.mark.parametrize("n", SIZES[:10])
def test_exact_small(kind, n):
    for k in KS:
        _check(kind, n, k)


@pytest.mark.parametrize("kind", CLOUDS)
@pytest.mark.parametrize("n", SIZES[10:])
def test_exact_large(kind, n):
    for k in KS:
        _check(kind, n, k)
    _ref16.cache_clear()


def test_all_equal_million_is_linear():
    """Every box contains every query at distance 0: a search that prunes by distance alone would be quadratic (10^12 pairs)."""
    n = 1_000_000
    x = torch.full((n, 3), 0.25, device="cuda")
    distCUDA2(x[:1000])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = distCUDA2(x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert dt < 5.0, f"{dt:.2f} s"
    assert int(torch.count_nonzero(d)) == 0
    t0 = time.perf_counter()
    nb = kneighbors(x, 5)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert dt < 5.0, f"kneighbors: {dt:.2f} s"
    # ties at distance 0 go to the smallest other indices
    nb = nb.cpu().numpy()
    i = np.arange(n)[:, None]
    t = np.arange(4)[None, :]
    expect = np.where(t < i, t, t + 1)
    assert np.array_equal(nb[:, 0], np.arange(n)) and np.array_equal(nb[:, 1:], expect)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_input_raises_and_context_recovers(bad):
    pts = make_cloud("uniform", 5000)
    x = torch.tensor(pts, device="cuda")
    y = x.clone()
    y[1234, 1] = bad
    with pytest.raises(_lib.GpccError, match="NaN or infinite"):
        distCUDA2(y)
    with pytest.raises(_lib.GpccError):
        kneighbors(y, 4)
    _, _, m = knn_ref.knn(pts, 3)
    assert np.array_equal(_bits(distCUDA2(x).cpu().numpy()), _bits(m))


def test_deterministic_and_stream_ordered():
    pts = make_cloud("blobs", 200_000)
    x = torch.tensor(pts, device="cuda")
    a = distCUDA2(x).cpu().numpy()
    b = distCUDA2(x).cpu().numpy()
    assert np.array_equal(_bits(a), _bits(b))
    ka = kneighbors(x, 4).cpu().numpy()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        xs = x * 1.0                  # produced on s: the search must be ordered behind it on s
        c = distCUDA2(xs)
        kc = kneighbors(xs, 4)
        c2 = c.clone()
    torch.cuda.current_stream().wait_stream(s)
    assert np.array_equal(_bits(c2.cpu().numpy()), _bits(a))
    assert np.array_equal(kc.cpu().numpy(), ka)


def test_workspace_within_stated_bound():
    for n in (1000, 300_000):
        x = torch.tensor(make_cloud("uniform", n), device="cuda")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        d = distCUDA2(x)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        out = -(-d.numel() * 4 // 512) * 512
        assert peak <= out + 26 * n + 65536 + 512, (n, peak)


def test_hac_voxel_size_and_scales():
    """HAC/scene/gaussian_model.py:456-476: the median of distCUDA2 sets voxel_size, log(sqrt(clamp_min(d, 1e-7))) the scales."""
    pts = make_cloud("dup2", 100_000)
    x = torch.tensor(pts, device="cuda")
    init_dist = distCUDA2(x).float().cuda()
    median, _ = torch.kthvalue(init_dist, int(init_dist.shape[0] * 0.5))
    _, _, m = knn_ref.knn(pts, 3)
    kv = int(len(m) * 0.5)
    assert _bits(np.float32(median.item())) == _bits(np.partition(m, kv - 1)[kv - 1])
    scales = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(x).float().cuda(), 0.0000001)))[..., None].repeat(1, 6)
    assert bool(torch.isfinite(scales).all())


def test_tcgs_kneighbors():
    from sklearn.neighbors import NearestNeighbors

    pts = make_cloud("uniform", 20_000)
    x = torch.tensor(pts, device="cuda")
    nb = kneighbors(x, 4)
    assert nb.dtype == torch.int64 and tuple(nb.shape) == (20_000, 4)
    nb = nb.cpu().numpy()
    j, _, _ = knn_ref.knn(pts, 3)
    assert np.array_equal(nb[:, 0], np.arange(len(pts))) and np.array_equal(nb[:, 1:], j)
    _, ind = NearestNeighbors(n_neighbors=4, algorithm="auto").fit(pts).kneighbors(pts)
    assert np.array_equal(nb, ind)
    lat = make_cloud("lattice", 4097)   # with ties: the restatement's order (distance, then index)
    j, _, _ = knn_ref.knn(lat, 16)
    nb = kneighbors(torch.tensor(lat, device="cuda"), 17).cpu().numpy()
    assert np.array_equal(nb[:, 1:], j)
    assert np.array_equal(kneighbors(torch.tensor(lat[:5], device="cuda"), 1).cpu().numpy(), np.arange(5)[:, None])


def test_edge_shapes():
    assert distCUDA2(torch.zeros((0, 3), device="cuda")).shape == (0,)
    x = torch.tensor(make_cloud("uniform", 1000), device="cuda")
    nc = x.t().contiguous().t()   # non-contiguous (P, 3) view
    assert not nc.is_contiguous()
    assert np.array_equal(_bits(distCUDA2(nc).cpu().numpy()), _bits(distCUDA2(x).cpu().numpy()))
    d = distCUDA2(torch.tensor([[1.0, 2.0, 3.0]], device="cuda")).cpu().numpy()
    assert np.isinf(d[0])
