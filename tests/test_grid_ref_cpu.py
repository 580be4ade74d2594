"""CPU checks of tests/grid_ref.py, the float64 restatement the grid encoder's GPU gradient tests compare against: it matches the
oracle's forward, its autograd passes gradcheck, and inside the grid its dy_dx formula is the true input derivative."""
import numpy as np
import pytest
import torch

from tests import grid_ref as gr


def _table(num_dim, n_features, res, log2_size, seed):
    offsets, off = [], 0
    for r in res:
        n = min(2 ** log2_size, r ** num_dim)
        offsets.append(off)
        off += int(np.ceil(n / 8) * 8)
    offsets.append(off)
    rng = np.random.RandomState(seed)
    return np.array(offsets, np.int32), np.array(res, np.int32), rng.uniform(-1, 1, (off, n_features)).astype(np.float32)


def _points(n, num_dim, seed):
    x = np.random.RandomState(seed).rand(n, num_dim).astype(np.float32)
    x[:4] = np.array([[0.0] * num_dim, [1.0] * num_dim, [1.25] * num_dim, [-0.1] + [0.5] * (num_dim - 1)], np.float32)
    return x


def _oracle(orc, x, emb, off, res, n_levels, rb=128, bv=None, ml=None):
    """orc_grid_forward with an explicit level count (a per-point min_level_id reads the full tables)."""
    x, emb = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(emb, np.float32)
    off, res = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(res, np.int32)
    out = np.empty((n_levels, x.shape[0], emb.shape[1]), np.float32)
    bv = None if bv is None else np.ascontiguousarray(bv, np.uint8)
    ml = None if ml is None else np.ascontiguousarray(ml, np.int32)
    orc.lib().orc_grid_forward(orc._p(x), orc._p(emb), orc._p(off), orc._p(res), orc._p(out), x.shape[0], x.shape[1], emb.shape[1], n_levels, rb,
                               orc._p(bv), orc._p(ml))
    return out


CASES = [  # num_dim, n_features, resolutions, log2 table size
    (3, 4, (18, 33, 59, 108), 13),      # dense (18^3 < 2^13) and hashed levels
    (3, 1, (16, 46, 92), 13),
    (2, 2, (130, 258, 514), 15),        # dense, then hashed
    (2, 8, (40, 300), 12),
]


@pytest.mark.parametrize("num_dim,n_features,res,log2_size", CASES)
@pytest.mark.parametrize("mode", ["plain", "binary_vxl", "min_level_id"])
def test_restatement_matches_oracle_forward(orc, num_dim, n_features, res, log2_size, mode):
    off, res_a, emb = _table(num_dim, n_features, res, log2_size, seed=num_dim * 7 + n_features)
    x = _points(1500, num_dim, seed=n_features)
    rb, bv, ml, nl = 128, None, None, len(res)
    if mode == "binary_vxl":
        rb = 32
        bv = (np.random.RandomState(3).rand(*([rb] * num_dim)) < 0.15).astype(np.uint8)
    if mode == "min_level_id":
        nl = len(res) - 1
        ml = np.random.RandomState(4).randint(0, 2, x.shape[0]).astype(np.int32)
    ref = _oracle(orc, x, emb, off, res_a, nl, rb, bv, ml)
    got = gr.forward(torch.tensor(x), torch.tensor(emb), off, res_a, nl, rb=rb, binary_vxl=bv, min_level_id=ml).numpy()
    assert got.shape == ref.shape
    scale = np.abs(emb).max()
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6 * scale)
    assert np.all(got[:, 2] == 0) and np.all(got[:, 3] == 0)      # out of range
    if mode == "binary_vxl":
        assert np.any(ref == 0) and np.any(ref != 0)               # the mask is exercised both ways


@pytest.mark.parametrize("num_dim,n_features", [(3, 2), (2, 4)])
def test_restatement_gradcheck_embeddings(num_dim, n_features):
    res = (10, 14, 40) if num_dim == 3 else (12, 90)
    off, res_a, emb = _table(num_dim, n_features, res, 6, seed=1)       # 64-row levels: every level hashed
    x = torch.tensor(_points(40, num_dim, seed=2))
    bv = (np.random.RandomState(5).rand(*([16] * num_dim)) < 0.4).astype(np.uint8)
    e = torch.tensor(emb, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: gr.forward(x, t, off, res_a, len(res), rb=16, binary_vxl=bv), (e,), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("num_dim,n_features,res,log2_size", CASES)
def test_dy_dx_is_the_derivative_inside_the_grid(num_dim, n_features, res, log2_size):
    off, res_a, emb = _table(num_dim, n_features, res, log2_size, seed=9)
    # interior: every corner of every level off the border, and away from cell boundaries (the interpolant has kinks there)
    rng = np.random.RandomState(num_dim + n_features)
    x = rng.uniform(0.1, 0.9, (400, num_dim))
    ok = np.ones(len(x), bool)
    for r in res:
        pos = x * (r - 2) + 0.5
        frac = pos - np.floor(pos)
        ok &= ((frac > 1e-3) & (frac < 1 - 1e-3)).all(1)
        ok &= ((np.floor(pos) >= 1) & (np.floor(pos) + 1 <= r - 2)).all(1)
    x = torch.tensor(x[ok])
    assert len(x) > 100
    xi = x.clone().requires_grad_(True)
    y = gr.forward(xi, torch.tensor(emb), off, res_a, len(res), f32_pos=False)     # (L, N, F)
    d = gr.dy_dx(x, emb, off, res_a, len(res), f32_pos=False)                     # (N, L, D, F)
    for l in range(len(res)):
        for ch in range(n_features):
            g, = torch.autograd.grad(y[l, :, ch].sum(), xi, retain_graph=True)
            np.testing.assert_allclose(d[:, l, :, ch].numpy(), g.numpy(), rtol=1e-9, atol=1e-9 * (res[l] - 2))
