"""numpy restatement of gpcc_knn's contract (include/gauspcc.h), the yardstick of the kNN tests.

d(i, j) = (dx*dx + dy*dy) + dz*dz with dx = x_j - x_i, every operation in float32 (numpy rounds each one; nothing is fused).  L_i = the k
smallest pairs (d(i, j), j) over j != i in lexicographic order, pairs with d > FLT_MAX left out, padded with (FLT_MAX, -1).  mean = the
sequential float32 sum of L_i's distances divided by float32(k).

Up to BRUTE_MAX points every pair is scored.  Above that a cKDTree proposes candidates in float64 that are re-scored with the float32
formula; a row is trusted only when its farthest candidate's float64 distance is clear of its k-th float32 distance by a relative
1e-5 (every point left out then scores above the k-th in float32: the float32 formula is within ~4e-7 relative of the exact value,
overflow included); the other rows are scored against every point.
"""
import numpy as np

from gauspcc_amd.synth import synthetic_cloud

FLT_MAX = np.float32(np.finfo(np.float32).max)
BRUTE_MAX = 20000
_BLOCK_ELEMS = 1 << 24   # float32 elements per brute-force block


def dist2_f32(q, p):
    """The contract's distance between every row of q (m, 3) and every row of p (n, 3): (m, n) float32."""
    q = np.asarray(q, np.float32)
    p = np.asarray(p, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = p[None, :, 0] - q[:, None, 0]
        dy = p[None, :, 1] - q[:, None, 1]
        dz = p[None, :, 2] - q[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz


def _select(d, j, self_idx, k):
    """Rows of candidate distances d (m, c) float32 with indices j (m, c) int64: the k lexicographically smallest counted pairs."""
    m = d.shape[0]
    ok = (d <= FLT_MAX) & (j != self_idx[:, None]) & (j >= 0)
    # d >= 0, so its float32 bits order like the value; (bits << 32) | j orders like (d, j)
    key = np.where(ok, (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64), np.uint64(np.iinfo(np.uint64).max))
    c = key.shape[1]
    if c > k:
        key = np.partition(key, k - 1, axis=1)[:, :k]
    key = np.sort(key, axis=1)
    out_d = np.full((m, k), FLT_MAX, np.float32)
    out_j = np.full((m, k), -1, np.int64)
    kk = min(k, c)
    valid = key[:, :kk] != np.uint64(np.iinfo(np.uint64).max)
    out_d[:, :kk] = np.where(valid, (key[:, :kk] >> np.uint64(32)).astype(np.uint32).view(np.float32), FLT_MAX)
    out_j[:, :kk] = np.where(valid, (key[:, :kk] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    return out_d, out_j


def _brute_rows(pts, rows, k):
    n = pts.shape[0]
    out_d = np.empty((len(rows), k), np.float32)
    out_j = np.empty((len(rows), k), np.int64)
    step = max(1, _BLOCK_ELEMS // max(n, 1))
    allj = np.arange(n, dtype=np.int64)
    for s in range(0, len(rows), step):
        r = rows[s:s + step]
        d = dist2_f32(pts[r], pts)
        out_d[s:s + step], out_j[s:s + step] = _select(d, np.broadcast_to(allj, d.shape), r, k)
    return out_d, out_j


def mean_of(dist):
    """Sequential float32 sum over the k columns, then / float32(k)."""
    k = dist.shape[1]
    s = dist[:, 0].astype(np.float32)
    with np.errstate(over="ignore"):
        for t in range(1, k):
            s = (s + dist[:, t]).astype(np.float32)
    return (s / np.float32(k)).astype(np.float32)


def knn(points, k, workers=16):
    """(idx (P, k) int64, dist2 (P, k) float32, mean (P,) float32) of the contract."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    n = pts.shape[0]
    if n == 0:
        return np.zeros((0, k), np.int64), np.zeros((0, k), np.float32), np.zeros(0, np.float32)
    if n <= BRUTE_MAX:
        d, j = _brute_rows(pts, np.arange(n, dtype=np.int64), k)
        return j, d, mean_of(d)
    from scipy.spatial import cKDTree

    p64 = pts.astype(np.float64)
    kq = min(n, 2 * k + 9)
    _, cand = cKDTree(p64).query(p64, k=kq, workers=workers)
    cand = cand.astype(np.int64)
    rows = np.arange(n, dtype=np.int64)
    d32 = np.empty(cand.shape, np.float32)
    step = max(1, _BLOCK_ELEMS // kq)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, n, step):
            q = pts[s:s + step, None, :]
            c = pts[cand[s:s + step]]
            dx, dy, dz = c[..., 0] - q[..., 0], c[..., 1] - q[..., 1], c[..., 2] - q[..., 2]
            d32[s:s + step] = (dx * dx + dy * dy) + dz * dz
    d, j = _select(d32, cand, rows, k)
    last64 = ((p64[cand[:, -1]] - p64) ** 2).sum(axis=1)
    kth = d[:, -1].astype(np.float64)
    unsure = np.nonzero(~(last64 > kth * (1.0 + 1e-5)))[0] if kq < n else np.zeros(0, np.int64)
    if len(unsure):
        d[unsure], j[unsure] = _brute_rows(pts, unsure, k)
    return j, d, mean_of(d)


def brute_scalar(points, k):
    """Second statement of the contract for small clouds, written the plain way: the float32 formula pair by pair on numpy scalars,
    each row's pairs sorted with Python's tuple order."""
    pts = np.asarray(points, np.float32)
    n = pts.shape[0]
    idx = np.full((n, k), -1, np.int64)
    dist = np.full((n, k), FLT_MAX, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            pairs = []
            for jj in range(n):
                if jj == i:
                    continue
                dx, dy, dz = pts[jj, 0] - pts[i, 0], pts[jj, 1] - pts[i, 1], pts[jj, 2] - pts[i, 2]
                dd = np.float32(np.float32(dx * dx + dy * dy) + dz * dz)
                if dd <= FLT_MAX:
                    pairs.append((float(dd), jj))
            pairs.sort()
            for t, (dd, jj) in enumerate(pairs[:k]):
                dist[i, t] = dd
                idx[i, t] = jj
    return idx, dist, mean_of(dist)


# ------------------------------------------------------------------ test clouds (float32), shared by the GPU tests and tools/knn_probe.py
def _shuffle(a, rng):
    return np.ascontiguousarray(a[rng.permutation(len(a))], dtype=np.float32)


def make_cloud(kind, n, seed=0):
    rng = np.random.default_rng(seed * 1000 + n)
    if kind == "uniform":
        return (rng.random((n, 3), dtype=np.float32) * np.float32(10) - np.float32(5)).astype(np.float32)
    if kind == "blobs":   # blob sigmas 1 and 0.1: point density differs 1000x
        c = rng.random((16, 3)) * 40
        s = np.where(np.arange(16) % 2 == 0, 1.0, 0.1)
        b = rng.integers(0, 16, n)
        return (c[b] + rng.standard_normal((n, 3)) * s[b, None]).astype(np.float32)
    if kind == "synth":
        return synthetic_cloud(n, seed=seed + 7).astype(np.float32)
    if kind == "plane":
        p = rng.random((n, 3), dtype=np.float32) * np.float32(8)
        p[:, 2] = np.float32(1.5)
        return p
    if kind == "line":
        t = rng.random(n, dtype=np.float32) * np.float32(100)
        return np.stack([t, np.float32(2) * t, np.float32(-3) * t], 1).astype(np.float32)
    if kind == "lattice":   # mass ties: every distance is an integer
        m = int(np.ceil(n ** (1 / 3)))
        g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
        return _shuffle(g[rng.permutation(len(g))[:n]] - m // 2, rng)
    if kind in ("dup2", "dup5"):
        r = 2 if kind == "dup2" else 5
        base = rng.random((-(-n // r), 3), dtype=np.float32) * np.float32(10)
        return _shuffle(np.repeat(base, r, axis=0)[:n], rng)
    if kind == "huge":   # coordinates near +-1e20: many squared distances overflow float32
        return ((rng.random((n, 3)) * 2 - 1) * 1e20).astype(np.float32)
    raise ValueError(kind)


CLOUDS = ["uniform", "blobs", "synth", "plane", "line", "lattice", "dup2", "dup5", "huge"]
