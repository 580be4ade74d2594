"""float64 torch restatement of the training branch of generate_neural_gaussians (the contract of gsnn_forward_train / gsnn_backward),
written from its definition: view vector and distance, the optional feature bank (softmax over strides 4 / 2 / 1), three two-layer MLPs on
[feat | view | dist], and the assembly of the kept Gaussians.  `mask_after=False` is HAC (mask in the opacity before the keep test),
True is HAC++ (keep = tanh > 0; the mask multiplies the kept rows' opacity and scaling).  Differentiable in every input."""
import torch


def mlp(x, w1, b1, w2, b2):
    return torch.relu(x @ w1.t() + b1) @ w2.t() + b2


def normalize(q, eps=1e-12):
    return q / q.norm(dim=-1, keepdim=True).clamp_min(eps)


def ng_train_ref(anchor, feat, offsets, scaling, masks, cam, params, mask_after=False):
    """params: 16 tensors {w1, b1, w2, b2} of bank (None x 4 without), opacity, cov, colour.  Returns (xyz, color, opacity, scaling, rot,
    neural_opacity (n K, 1), keep (n K))."""
    n, F = feat.shape
    K = offsets.shape[1]
    v = anchor - cam.view(1, 3)
    dist = v.norm(dim=1, keepdim=True)
    view = v / dist
    if params[0] is not None:
        w = torch.softmax(mlp(torch.cat([view, dist], 1), *params[0:4]), dim=1)
        idx4 = torch.arange(F) % (F // 4) * 4
        idx2 = torch.arange(F) % (F // 2) * 2
        feat = feat[:, idx4] * w[:, 0:1] + feat[:, idx2] * w[:, 1:2] + feat * w[:, 2:3]
    x = torch.cat([feat, view, dist], 1)
    t = torch.tanh(mlp(x, *params[4:8])).reshape(-1, 1)
    m = masks.reshape(-1, 1)
    if mask_after:
        nopa = t
        keep = (t > 0).view(-1)
    else:
        nopa = t * m
        keep = (nopa > 0).view(-1)
    color = torch.sigmoid(mlp(x, *params[12:16])).reshape(n * K, 3)[keep]
    sr = mlp(x, *params[8:12]).reshape(n * K, 7)[keep]
    rep_s = scaling.repeat_interleave(K, dim=0)[keep]
    rep_a = anchor.repeat_interleave(K, dim=0)[keep]
    opacity = nopa[keep]
    sc = rep_s[:, 3:] * torch.sigmoid(sr[:, :3])
    if mask_after:
        opacity = opacity * m[keep]
        sc = sc * m[keep]
    rot = normalize(sr[:, 3:7])
    xyz = rep_a + offsets.reshape(-1, 3)[keep] * rep_s[:, :3]
    return xyz, color, opacity, sc, rot, nopa, keep


def random_params(F, K, bank, gen, dtype=torch.float64, scale=1.0):
    def lin(o, i):
        b = 1.0 / i ** 0.5
        return [(torch.rand(o, i, generator=gen, dtype=dtype) * 2 - 1) * b * scale, (torch.rand(o, generator=gen, dtype=dtype) * 2 - 1) * b * scale]
    bk = lin(F, 4) + lin(3, F) if bank else [None] * 4
    return bk + lin(F, F + 4) + lin(K, F) + lin(F, F + 4) + lin(7 * K, F) + lin(F, F + 4) + lin(3 * K, F)


def ste_masks(n, K, gen, dtype=torch.float64):
    """(b - s) + s with s = sigmoid(logit), b = s > 0.01, in float32 as HAC's get_mask: values only nearly {0, 1}"""
    s = torch.sigmoid(torch.randn(n, K, 1, generator=gen, dtype=torch.float32) * 4.0)
    return (((s > 0.01).float() - s) + s).to(dtype)


def fixture(n, F, K, bank, mask_after, seed, device):
    """inputs (float64 on `device`) without a candidate the keep test could decide either way: anchors with an unmasked (HAC) or any (HAC++)
    candidate at |tanh z| < 1e-4 are left out, so that the fp32 and float64 keep sets must agree"""
    g = torch.Generator().manual_seed(seed)
    d = torch.float64
    anchor = torch.rand(n, 3, generator=g, dtype=d) * 4 - 2
    feat = torch.randn(n, F, generator=g, dtype=d) * 0.8
    off = torch.randn(n, K, 3, generator=g, dtype=d) * 0.3
    sc = torch.exp(torch.randn(n, 6, generator=g, dtype=d) * 0.4 - 2.5)
    masks = ste_masks(n, K, g)
    if n > 4:
        masks[: n // 5] = 0.0       # fully masked anchors
    cam = torch.tensor([0.3, -4.0, 1.1], dtype=d)
    params = random_params(F, K, bank, g)
    ts = [t.to(device) for t in (anchor, feat, off, sc, masks, cam)]
    ps = [None if p is None else p.to(device) for p in params]
    t = ng_train_ref(*ts, ps, True)[5].view(n, K)        # tanh(z)
    live = masks.to(device).view(n, K) != 0 if not mask_after else torch.ones_like(t, dtype=torch.bool)
    ok = ~((t.abs() < 1e-4) & live).any(dim=1)
    ts = [x[ok] for x in ts[:5]] + [ts[5]]
    t = t[ok]
    assert not ((t.abs() < 1e-4) & (live[ok])).any()
    return ts, ps


# ---- every emission class, wave count and strip count of csrc/neural_gaussians.hip ---------------------------------------------------------------
# (F, K, bank).  K = 1, 3, 4: k_ng_emit's NIT = ceil(16 K / 64) = 1, K = 4 filling its 64 candidates exactly; 8 | 9: NIT 2 | 3, and 7 K = 63 one row short
# of a 64-row strip of the weight gradients; 13, 14, 15: NIT = 4 with ragged head tiles, 13 | 14 the eight-wave | four-wave edge at F = 50; 16: full
# tiles; 22: the lane kernels, 3 K = 66 is two strips; 64: the limit, with the bank all 16 strips of k_ngb_wgrad's table.
EDGE_K = [1, 3, 4, 8, 9, 13, 14, 15, 16, 22, 64]
NG_EDGES = [(F, K, bank) for K in EDGE_K for F, bank in ((32, True), (50, False))] + [(32, K, False) for K in (4, 13, 64)]
GRAD_K = [1, 4, 9, 13, 14, 16, 22, 64]
EDGE_ROWS = [1, 16, 17, 333]        # less than a 16-anchor tile, a full one, one anchor more, several workgroups' worth
LOOP_ROWS = 32787                   # 2050 tiles: more than 256 workgroups x 4 or 8 waves take in one trip, and a ragged last tile
LOOP_EDGES = [(50, 14, False), (32, 8, True)]
GUARDED_EDGES = [(32, 3, True), (50, 14, False), (32, 22, False)]
BITWISE_EDGES = [(32, 64, True), (50, 14, False)]
# The seed of a case is 100 F + K + 10000 j with the smallest j for which, at every row count above (and LOOP_ROWS where it runs) and in both mask
# orders, between 10 % and 90 % of the candidates are kept and, at 1, 16 and 17 anchors, at least one is (tests/test_ng_train_cpu.py); j = 0 where
# the case is not listed.  A head of few outputs can come out one-sided: with the suite's older rule 7 F + K, (50, 1) keeps 0.6 %.
EDGE_SEED_J = {(32, 1, True): 31, (50, 1, False): 12, (32, 3, True): 1}


def edge_seed(F, K, bank):
    return 100 * F + K + 10000 * EDGE_SEED_J.get((F, K, bank), 0)


def edge_case(n, F, K, bank, mask_after, device, seed=None):
    """(ts, ps, dropped share): `fixture` drawn with a margin and cut to exactly n anchors -- the last n, the fully masked fifth stands in front --
    so that the row counts keep their meaning"""
    m = n + max(64, n // 8)
    ts, ps = fixture(m, F, K, bank, mask_after, edge_seed(F, K, bank) if seed is None else seed, device)
    left = ts[0].shape[0]
    assert left >= n, "margin too small"
    return [t[left - n:].contiguous() for t in ts[:5]] + [ts[5]], ps, 1.0 - left / m
