"""The project's own restatement of CAT-3DGS's tri-plane ARM rate term, written from the formulas (not from the reference's text):

  per latent y[c, h, w] of a level [C, H, W]:
    ctx_i = y[c, h - 2 + i // 5, w - 2 + i % 5], i = 0..11, zero outside the plane
    a layer is x W^T + b, plus x where a hidden layer's input and output widths agree; a ReLU behind every hidden layer
    (mu, ls) = MLP(ctx); s = exp(-0.5 clamp(ls, -10, 13.8155))
    F(t) = 0.5 - 0.5 sign(t - mu) expm1(-|t - mu| / s); p0 = F(y + 0.5) - F(y - 0.5); rate = -log2(max(p0, 2^-16))

`forward64` / `grads64` are numpy float64 with analytic gradients (autograd's choices at the kinks: the floor passes iff p0 >= 2^-16, the
clamp iff -10 <= ls <= 13.8155, a ReLU iff its output is > 0).  `rate_torch` is the float32 torch sequence a framework would run (pad,
unfold twice, a materialised [n, 25] matrix, index_select, linear layers); the GPU test calibrates its tolerance by that sequence's own
error against float64, and tools/arm_probe.py times it.

Parameters are a list in state-dict order: [w0, b0, w1, b1, ...], w (out, in)."""
import numpy as np
import torch
import torch.nn.functional as F

N_CTX, MASK = 12, 5
P_FLOOR = 2.0 ** -16
LS_MIN, LS_MAX = -10.0, 13.8155
CASES = ("round", "noise", "kinks", "wide")


def _layers(params):
    """[(w, b, residual, hidden)] from the flat list"""
    ws, bs = params[0::2], params[1::2]
    last = len(ws) - 1
    return [(w, b, l < last and w.shape[0] == w.shape[1], l < last) for l, (w, b) in enumerate(zip(ws, bs))]


def contexts64(y):
    """y (C, H, W) -> (C * H * W, 12)"""
    C, H, W = y.shape
    pad = np.pad(y, ((0, 0), (2, 2), (2, 2)))
    return np.stack([pad[:, i // MASK:i // MASK + H, i % MASK:i % MASK + W] for i in range(N_CTX)], axis=-1).reshape(-1, N_CTX)


def _level_shape(y):
    return tuple(y.shape[-3:])


def forward64(levels, params):
    """levels: arrays (C, H, W) or (1, C, H, W); returns a dict of flat float64 arrays in (level, c, h, w) order plus the activations"""
    params = [np.asarray(p, dtype=np.float64) for p in params]
    ys = [np.asarray(y, dtype=np.float64).reshape(_level_shape(y)) for y in levels]
    x = np.concatenate([y.reshape(-1) for y in ys])
    acts = [np.concatenate([contexts64(y) for y in ys], axis=0)]
    for w, b, res, hidden in _layers(params):
        z = acts[-1] @ w.T + b
        if res:
            z = z + acts[-1]
        acts.append(np.maximum(z, 0.0) if hidden else z)
    mu, ls = acts[-1][:, 0], acts[-1][:, 1]
    s = np.exp(-0.5 * np.clip(ls, LS_MIN, LS_MAX))
    du, dl = x + 0.5 - mu, x - 0.5 - mu
    cdf = lambda d: 0.5 - 0.5 * np.sign(d) * np.expm1(-np.abs(d) / s)   # noqa: E731
    p0 = cdf(du) - cdf(dl)
    return {"x": x, "acts": acts, "mu": mu, "ls": ls, "scale": s, "du": du, "dl": dl, "p0": p0, "rate": -np.log2(np.maximum(p0, P_FLOOR)),
            "shapes": [y.shape for y in ys]}


def grads64(levels, params, wts, fwd=None):
    """gradients of sum(wts * rate): ([g_level (C, H, W)], [g_param], per-latent (g_mu, g_ls))"""
    params = [np.asarray(p, dtype=np.float64) for p in params]
    f = fwd or forward64(levels, params)
    wts = np.asarray(wts, dtype=np.float64).reshape(-1)
    s, du, dl, p0 = f["scale"], f["du"], f["dl"], f["p0"]
    gp = np.where(p0 >= P_FLOOR, -wts / (np.maximum(p0, 1e-300) * np.log(2.0)), 0.0)
    eu, el = np.exp(-np.abs(du) / s), np.exp(-np.abs(dl) / s)
    gx = gp * (0.5 * np.sign(du) ** 2 * eu - 0.5 * np.sign(dl) ** 2 * el) / s
    ls_in = (f["ls"] >= LS_MIN) & (f["ls"] <= LS_MAX)
    gls = np.where(ls_in, gp * 0.25 * (du * eu - dl * el) / s, 0.0)
    dz = np.stack([-gx, gls], axis=1)
    layers = _layers(params)
    gparams = [None] * len(params)
    for l in range(len(layers) - 1, -1, -1):
        w, b, res, hidden = layers[l]
        if hidden:
            dz = dz * (f["acts"][l + 1] > 0)
        gparams[2 * l], gparams[2 * l + 1] = dz.T @ f["acts"][l], dz.sum(axis=0)
        dz = dz @ w + (dz if res else 0.0)
    glevels, off = [], 0
    for C, H, W in f["shapes"]:
        n = C * H * W
        gpad = np.zeros((C, H + 4, W + 4))
        gc = dz[off:off + n].reshape(C, H, W, N_CTX)
        for i in range(N_CTX):
            gpad[:, i // MASK:i // MASK + H, i % MASK:i % MASK + W] += gc[..., i]
        glevels.append(gpad[:, 2:2 + H, 2:2 + W] + gx[off:off + n].reshape(C, H, W))
        off += n
    return glevels, gparams, (-gx, gls)


def near_floor(p0, rel):
    """latents whose probability lies within rel of the 2^-16 floor: either side of the kink in float32"""
    return np.abs(p0 / P_FLOOR - 1.0) <= rel


def context_positions(shape, c, h, w):
    """the (c, h', w') of the up to 12 context entries of (c, h, w) that lie inside the plane"""
    _, H, W = shape
    out = []
    for i in range(N_CTX):
        hh, ww = h - 2 + i // MASK, w - 2 + i % MASK
        if 0 <= hh < H and 0 <= ww < W:
            out.append((c, hh, ww))
    return out


def mlp_torch(x, params):
    ws, bs = params[0::2], params[1::2]
    for l, (w, b) in enumerate(zip(ws, bs)):
        z = F.linear(x, w, b)
        if l < len(ws) - 1:
            x = torch.relu(z + x if w.shape[0] == w.shape[1] else z)
        else:
            x = z
    return x


def contexts_torch(y):
    """y (1, C, H, W) -> the materialised (C * H * W, 25) window matrix, then its first 12 columns"""
    pad = F.pad(y, (2, 2, 2, 2), mode="constant", value=0.0)
    win = pad.unfold(2, MASK, 1).unfold(3, MASK, 1).reshape(-1, MASK * MASK)
    return torch.index_select(win, 1, torch.arange(N_CTX, device=y.device))


def rate_torch(levels, params):
    """the torch sequence in the tensors' own dtype: (rate, mu, scale), flat in (level, c, h, w) order"""
    ys = [y.reshape((1,) + tuple(y.shape[-3:])) for y in levels]
    ctx = torch.cat([contexts_torch(y) for y in ys], dim=0)
    x = torch.cat([y.reshape(-1) for y in ys])
    raw = mlp_torch(ctx, params)
    mu, ls = raw[:, 0], raw[:, 1]
    s = torch.exp(-0.5 * torch.clamp(ls, min=LS_MIN, max=LS_MAX))
    cdf = lambda t: 0.5 - 0.5 * (t - mu).sign() * torch.expm1(-(t - mu).abs() / s)   # noqa: E731
    p = torch.clamp_min(cdf(x + 0.5) - cdf(x - 0.5), P_FLOOR)
    return -torch.log2(p), mu, s


def golden_case(z, key):
    """one case of tests/golden/arm_rate.npz as numpy arrays"""
    nlev, npar = int(z[f"{key}_nlevels"]), len(z[f"{key}_keys"])
    return {"levels": [z[f"{key}_y{i}"] for i in range(nlev)], "params": [z[f"{key}_p{j}"] for j in range(npar)],
            "keys": [str(k) for k in z[f"{key}_keys"]], "layers": [int(v) for v in z[f"{key}_layers"]], "w": z[f"{key}_w"],
            "rate": z[f"{key}_rate"], "mu": z[f"{key}_mu"], "scale": z[f"{key}_scale"],
            "g_levels": [z[f"{key}_gy{i}"] for i in range(nlev)], "g_params": [z[f"{key}_gp{j}"] for j in range(npar)]}
