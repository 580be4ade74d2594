"""CPU checks of the kNN work: the numpy restatement of gpcc_knn's contract (tests/knn_ref.py) against independent statements of it,
simple_knn's values for P <= 3, and the argument checks of gauspcc_amd.knn, which must all raise before anything touches a device."""
import numpy as np
import pytest
import torch

from tests import knn_ref

FLT_MAX = float(np.finfo(np.float32).max)


def _uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32) * np.float32(10.0) - np.float32(5.0)


@pytest.mark.parametrize("k", [1, 3, 4, 16])
def test_restatement_matches_scalar_statement(k):
    rng = np.random.default_rng(k)
    clouds = [_uniform(70, 1), np.repeat(_uniform(20, 2), 3, axis=0), rng.integers(-3, 4, (90, 3)).astype(np.float32),
              (_uniform(40, 3) * np.float32(2e19)).astype(np.float32)]
    for pts in clouds:
        j, d, m = knn_ref.knn(pts, k)
        j2, d2, m2 = knn_ref.brute_scalar(pts, k)
        assert np.array_equal(j, j2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
        assert np.array_equal(m.view(np.uint32), m2.view(np.uint32))


@pytest.mark.parametrize("k", [1, 3, 16])
def test_restatement_against_float64(k):
    """On tie-free data the lists are those of exact float64 distances, and each distance is within float32 rounding of exact."""
    pts = _uniform(3000, 7)
    j, d, _ = knn_ref.knn(pts, k)
    p = pts.astype(np.float64)
    d64 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d64, np.inf)
    order = np.argsort(d64, axis=1, kind="stable")[:, :k]
    assert np.array_equal(j, order)
    exact = np.take_along_axis(d64, order, axis=1)
    assert np.all(np.abs(d.astype(np.float64) - exact) <= 1e-6 * exact)


def test_restatement_against_sklearn():
    from sklearn.neighbors import NearestNeighbors

    pts = _uniform(5000, 11)
    _, ind = NearestNeighbors(n_neighbors=4).fit(pts).kneighbors(pts)
    j, _, _ = knn_ref.knn(pts, 3)
    assert np.array_equal(ind[:, 0], np.arange(len(pts)))
    assert np.array_equal(ind[:, 1:], j)


@pytest.mark.parametrize("dup", [1, 5])
def test_tree_path_matches_brute_force(dup):
    """Above BRUTE_MAX the restatement takes cKDTree candidates; with mass ties (lattice, duplicates) it must fall back where needed."""
    rng = np.random.default_rng(dup)
    base = rng.integers(0, 30, (knn_ref.BRUTE_MAX // dup + 500, 3)).astype(np.float32)
    pts = np.repeat(base, dup, axis=0)[rng.permutation(len(base) * dup)]
    assert len(pts) > knn_ref.BRUTE_MAX
    j, d, m = knn_ref.knn(pts, 16)
    rows = rng.choice(len(pts), 300, replace=False)
    d2, j2 = knn_ref._brute_rows(pts, rows, 16)
    assert np.array_equal(j[rows], j2) and np.array_equal(d[rows], d2)
    assert np.array_equal(m[rows], knn_ref.mean_of(d2))


def test_simple_knn_sentinels():
    """simple_knn keeps FLT_MAX in the slots it cannot fill: P = 1, 2 give inf, P = 3 (d0 + d1 + FLT_MAX) / 3, finite."""
    j, d, m = knn_ref.knn(np.zeros((1, 3), np.float32), 3)
    assert np.isinf(m[0]) and np.array_equal(j, [[-1, -1, -1]]) and np.all(d == np.float32(FLT_MAX))
    _, _, m = knn_ref.knn(np.array([[0, 0, 0], [1, 0, 0]], np.float32), 3)
    assert np.all(np.isinf(m))
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    j, d, m = knn_ref.knn(pts, 3)
    assert np.all(np.isfinite(m))
    assert m[0] == np.float32((np.float32(1) + np.float32(4) + np.float32(FLT_MAX)) / np.float32(3))
    assert np.array_equal(j[:, 2], [-1, -1, -1]) and np.array_equal(j[0, :2], [1, 2])


def test_overflowing_pairs_do_not_count():
    pts = np.array([[-1e20, 0, 0], [1e20, 0, 0], [1e20, 1, 0]], np.float32)
    j, d, _ = knn_ref.knn(pts, 2)
    assert np.array_equal(j[0], [-1, -1])           # (2e20)^2 overflows: no neighbour counts
    assert np.array_equal(j[1], [2, -1]) and d[1, 0] == np.float32(1.0)


def _no_device(monkeypatch):
    from gauspcc_amd import _lib, runtime

    def boom(*a, **k):
        raise AssertionError("an argument check let the call reach the library")

    monkeypatch.setattr(runtime, "context", boom)
    monkeypatch.setattr(runtime, "stream_ptr", boom)
    monkeypatch.setattr(_lib, "lib", boom)


def test_distcuda2_argument_checks(monkeypatch):
    from gauspcc_amd.knn import distCUDA2

    _no_device(monkeypatch)
    with pytest.raises(TypeError, match="float32"):
        distCUDA2(torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(TypeError, match="float32"):
        distCUDA2(torch.zeros((4, 3), dtype=torch.int32))
    with pytest.raises(TypeError, match="Tensor"):
        distCUDA2(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match=r"\(P, 3\)"):
        distCUDA2(torch.zeros((4, 2)))
    with pytest.raises(ValueError, match=r"\(P, 3\)"):
        distCUDA2(torch.zeros(12))
    with pytest.raises(ValueError, match="CUDA"):
        distCUDA2(torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        distCUDA2(torch.zeros((0, 3)))


def test_kneighbors_argument_checks(monkeypatch):
    from gauspcc_amd.knn import kneighbors

    _no_device(monkeypatch)
    x = torch.zeros((20, 3))
    with pytest.raises(TypeError, match="float32"):
        kneighbors(x.double(), 4)
    with pytest.raises(ValueError, match=r"\(P, 3\)"):
        kneighbors(torch.zeros((20, 4)), 4)
    for K in (0, -1, 18):
        with pytest.raises(ValueError, match="outside"):
            kneighbors(x, K)
    with pytest.raises(ValueError, match="n_samples"):
        kneighbors(torch.zeros((3, 3)), 4)
    with pytest.raises(TypeError):
        kneighbors(x, 4.0)
    with pytest.raises(TypeError):
        kneighbors(x, True)
    with pytest.raises(ValueError, match="CUDA"):
        kneighbors(x, np.int64(4))


def test_export_bound():
    from gauspcc_amd import _lib

    assert "gpcc_knn" in _lib.EXPORTS
    assert _lib.lib().gpcc_knn.argtypes is not None
