"""A float64 torch restatement of GausPcgc's training forward (src/ai_pcc/GausPcgc/network_ue_4stage_conv.py:100-182, kit/nn.py),
independent of the library and of the oracle: its own octree (numpy), its own neighbour search (sorted numpy keys), level by level as
the reference loops.  The yardstick of the training path's loss and gradients."""
import numpy as np
import torch

STAGE_M = (2, 2, 4, 16)
_B = 1 << 20


def build_levels(points):
    """[(coords (n, 3) int64, occupancy (n,) int64), ...] base level first: the FOG loop, stopping at the first level below 64 nodes."""
    c = np.unique(np.asarray(points, dtype=np.int64), axis=0)
    levels = []
    while True:
        par = c >> 1
        bit = (c[:, 0] & 1) + 2 * (c[:, 1] & 1) + 4 * (c[:, 2] & 1)
        up, inv = np.unique(par, axis=0, return_inverse=True)
        occ = np.zeros(up.shape[0], dtype=np.int64)
        np.add.at(occ, inv.reshape(-1), np.int64(1) << bit)
        levels.append((up, occ))
        c = up
        if up.shape[0] < 64:
            break
    return levels[::-1]


def _keys(c):
    c = np.asarray(c, dtype=np.int64) + _B
    return (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def lookup(coords, query):
    """Row of each query point in coords, -1 where absent."""
    k = _keys(coords)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    q = _keys(query)
    pos = np.clip(np.searchsorted(ks, q), 0, len(ks) - 1)
    return np.where(ks[pos] == q, order[pos], -1)


def neighbours(coords, k):
    """(n, k^3): row of coords[i] + d_o, o = (dx + r) + k (dy + r) + k^2 (dz + r) (model.conv_offset_layout), -1 where absent."""
    r = k // 2
    out = np.empty((coords.shape[0], k ** 3), dtype=np.int64)
    for o in range(k ** 3):
        d = np.array([o % k - r, (o // k) % k - r, o // (k * k) - r], dtype=np.int64)
        out[:, o] = lookup(coords, coords + d)
    return out


def conv(x, nbr, w, res=None, relu=False):
    """out[i] = sum_o x[nbr[i, o]] @ w[o] (+ res) (ReLU)."""
    out = torch.zeros(x.shape[0], w.shape[2], dtype=x.dtype, device=x.device)
    for o in range(nbr.shape[1]):
        m = np.nonzero(nbr[:, o] >= 0)[0]
        if m.size:
            out = out.index_add(0, torch.as_tensor(m), x[torch.as_tensor(nbr[m, o])] @ w[o])
    if res is not None:
        out = out + res
    return torch.relu(out) if relu else out


def _trunk(p, pre, x, nbr):
    x = conv(x, nbr, p[f"{pre}.0.kernel"], relu=True)
    for b in (2, 3):
        y = conv(x, nbr, p[f"{pre}.{b}.conv0.kernel"], relu=True)
        x = conv(y, nbr, p[f"{pre}.{b}.conv1.kernel"], res=x, relu=True)
    return x


def total_bits(p, points, k):
    """Sum over coded symbols of clamp(-log2(p_gt + 1e-10), 0, 50).  p: upstream key -> torch tensor (dtype of the computation)."""
    levels = build_levels(points)
    dt = p["prior_embedding.weight"].dtype
    total = torch.zeros((), dtype=dt)
    for d in range(len(levels) - 1):
        (pc, po), (cc, co) = levels[d], levels[d + 1]
        x = p["prior_embedding.weight"][torch.as_tensor(po)]
        x = _trunk(p, "prior_resnet", x, neighbours(pc, k))
        par = lookup(pc, cc >> 1)
        octant = (cc[:, 0] & 1) + 2 * (cc[:, 1] & 1) + 4 * (cc[:, 2] & 1)
        x = x[torch.as_tensor(par)] + p["target_embedding.target_res_embedding.weight"][torch.as_tensor(octant)]
        nb = neighbours(cc, k)
        X = _trunk(p, "target_resnet", x, nb)
        o = torch.as_tensor(co)
        sym = ((o >> 7) & 1, (o >> 6) & 1, (o >> 4) & 3, o & 15)
        prev = (None, sym[0], sym[0] * 2 + sym[1], (sym[0] * 2 + sym[1]) * 4 + sym[2])
        for s in range(4):
            u = X if s == 0 else X + p[f"pred_head_s{s}_emb.weight"][prev[s]]
            y = conv(conv(u, nb, p[f"spatial_conv_s{s}.0.kernel"], relu=True), nb, p[f"spatial_conv_s{s}.2.kernel"])
            h = torch.relu(y @ p[f"pred_head_s{s}.0.weight"].T + p[f"pred_head_s{s}.0.bias"])
            pr = torch.softmax(h @ p[f"pred_head_s{s}.2.weight"].T + p[f"pred_head_s{s}.2.bias"], dim=-1)
            total = total + torch.clamp(-torch.log2(pr.gather(1, sym[s].view(-1, 1)) + 1e-10), 0, 50).sum()
    return total


def params(sd, dtype=torch.float64, requires_grad=False):
    """upstream state dict (numpy or torch) -> {key: tensor} without the constant FOG kernel."""
    out = {}
    for key, v in sd.items():
        if key == "fog.conv.kernel":
            continue
        t = (v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype).clone()
        out[key] = t.requires_grad_(requires_grad)
    return out
