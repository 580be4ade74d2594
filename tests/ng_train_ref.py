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
