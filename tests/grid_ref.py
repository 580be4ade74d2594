"""Float64 torch restatement of the hash-grid encoder (gridencoder.zip!gridencoder/src/gridencoder.cu:100-361 and :363-657): the
forward with binary_vxl, per-point min_level_id and out-of-range inputs, and the reference's dy_dx formula.  Differentiable with
respect to the embeddings (and, with f32_pos=False, the inputs), so autograd gives the embedding gradient the backward must match.

f32_pos=True places the points exactly as the device does (position, cell and fraction in float32) and only then widens the
fraction: corner choice and masks then agree with the device at every cell boundary, and the weights differ by float32 rounding.
"""
import torch

PRIMES = (1, 2654435761, 805459861)
M32 = 0xFFFFFFFF


def _place(x, res, f32_pos):
    """x (N, D), res (N,) int64 -> (fraction (N, D) float64, cell (N, D) int64)."""
    r2 = (res - 2).unsqueeze(1)
    if f32_pos:
        pos = x.detach().float() * r2.float() + 0.5          # two float32 roundings, as on the device
        pg = torch.floor(pos)
        return (pos - pg).double(), pg.long()
    pos = x.double() * r2.double() + 0.5
    pg = torch.floor(pos.detach())
    return pos - pg, pg.long()


def _index(pl, res, hms):
    """Row within the level of corners pl (N, D): dense index when res^D <= hashmap size, else the xor hash; modulo the size."""
    D = pl.shape[1]
    dense = torch.zeros_like(res)
    stride = torch.ones_like(res)
    for d in range(D):
        dense = dense + pl[:, d] * stride
        stride = stride * res
    h = torch.zeros_like(res)
    for d in range(D):
        h = h ^ ((pl[:, d] * PRIMES[d]) & M32)
    return torch.where(stride <= hms, dense, h) % hms


def _footprint(pl, res, rb, sat):
    """binary_vxl test of gridencoder.cu:262-317: any occupied voxel in the corner's box (float32 arithmetic), via a summed-area table."""
    D = pl.shape[1]
    scale_re = (1.0 / (res.double() - 2.0)).float()
    lo, hi = [], []
    for d in range(D):
        pn = ((pl[:, d].double() - 0.5) * scale_re.double()).float()
        a = ((pn - scale_re) * float(rb)).clamp(0.0, float(rb - 1)).long()
        b = ((pn + scale_re) * float(rb)).clamp(0.0, float(rb - 1)).long()
        lo.append(a)
        hi.append(b + 1)
    total = torch.zeros(pl.shape[0], dtype=torch.int64)
    for corner in range(1 << D):    # inclusion-exclusion over the box's 2^D corners in the padded table
        idx = tuple(hi[d] if (corner >> d) & 1 else lo[d] for d in range(D))
        sign = -1 if (D - bin(corner).count("1")) % 2 else 1
        total = total + sign * sat[idx]
    return total > 0


def _sat(binary_vxl):
    s = torch.as_tensor(binary_vxl).to(torch.int64)
    for d in range(s.dim()):
        s = torch.nn.functional.pad(s.cumsum(d), [0, 0] * (s.dim() - 1 - d) + [1, 0])
    return s


def _levels(offsets, resolutions, N, L, min_level_id):
    off = torch.as_tensor(offsets).long()
    res = torch.as_tensor(resolutions).long()
    ml = torch.zeros(N, dtype=torch.int64) if min_level_id is None else torch.as_tensor(min_level_id).long()
    for l in range(L):
        lev = ml + l
        yield l, off[lev], off[lev + 1] - off[lev], res[lev]


def forward(inputs, emb, offsets, resolutions, n_levels, rb=128, binary_vxl=None, min_level_id=None, f32_pos=True):
    """(n_levels, N, F) float64.  emb (rows, F) may require grad; so may inputs with f32_pos=False."""
    x = inputs if torch.is_tensor(inputs) else torch.as_tensor(inputs)
    emb = emb if torch.is_tensor(emb) else torch.as_tensor(emb)
    emb = emb.double() if emb.dtype != torch.float64 else emb
    N, D = x.shape
    sat = None if binary_vxl is None else _sat(binary_vxl)
    inside = ((x.detach() >= 0) & (x.detach() <= 1)).all(1)
    outs = []
    for l, off, hms, res in _levels(offsets, resolutions, N, n_levels, min_level_id):
        frac, pg = _place(x, res, f32_pos)
        acc, wn = 0.0, torch.zeros(N, dtype=torch.float64)
        terms = []
        for c in range(1 << D):
            w = torch.ones(N, dtype=torch.float64)
            pl = torch.empty_like(pg)
            for d in range(D):
                if (c >> d) & 1:
                    w = w * frac[:, d]
                    pl[:, d] = torch.minimum(pg[:, d] + 1, res - 1)
                else:
                    w = w * (1 - frac[:, d])
                    pl[:, d] = pg[:, d]
            use = ~((pl == 0) | (pl == (res - 1).unsqueeze(1))).any(1) & inside
            if sat is not None:
                use = use & _footprint(pl, res, rb, sat)
            row = torch.where(use, off + _index(pl.clamp(min=0), res, hms), 0)
            terms.append((w, use, row))
            wn = wn + torch.where(use, w, torch.zeros_like(w))
        wn = torch.where(wn == 0, torch.full_like(wn, 1e-9), wn)
        for w, use, row in terms:
            acc = acc + torch.where(use, w / wn, torch.zeros_like(w)).unsqueeze(1) * emb[row]
        outs.append(acc)
    return torch.stack(outs)


def dy_dx(inputs, emb, offsets, resolutions, n_levels, min_level_id=None, f32_pos=True, magnitude=False):
    """(N, n_levels, D, F) float64: gridencoder.cu:363-657, edge differences times (res - 2), border corners read as 0, no wn, no mask.
    magnitude=True sums the edges' |terms| instead: the scale a float32 evaluation's rounding error is measured against."""
    x = torch.as_tensor(inputs)
    emb = torch.as_tensor(emb).double()
    N, D = x.shape
    F = emb.shape[1]
    inside = ((x >= 0) & (x <= 1)).all(1)
    out = torch.zeros(N, n_levels, D, F, dtype=torch.float64)
    for l, off, hms, res in _levels(offsets, resolutions, N, n_levels, min_level_id):
        frac, pg = _place(x, res, f32_pos)
        frac = frac.detach()
        for gd in range(D):
            g = torch.zeros(N, F, dtype=torch.float64)
            for e in range(1 << (D - 1)):
                w = (res - 2).double()
                pl = pg.clone()
                for nd in range(D - 1):
                    d = nd + 1 if nd >= gd else nd
                    if (e >> nd) & 1:
                        w = w * frac[:, d]
                        pl[:, d] = torch.minimum(pg[:, d] + 1, res - 1)
                    else:
                        w = w * (1 - frac[:, d])
                vals = []
                for right in (False, True):
                    q = pl.clone()
                    q[:, gd] = torch.minimum(pg[:, gd] + 1, res - 1) if right else pg[:, gd]
                    zero = ((q == 0) | (q == (res - 1).unsqueeze(1))).any(1) | ~inside
                    row = torch.where(zero, 0, off + _index(q.clamp(min=0), res, hms))
                    vals.append(torch.where(zero.unsqueeze(1), torch.zeros(N, F, dtype=torch.float64), emb[row]))
                t = w.unsqueeze(1) * (vals[1] - vals[0])
                g = g + (t.abs() if magnitude else t)
            out[:, l, gd] = torch.where(inside.unsqueeze(1), g, torch.zeros_like(g))
    return out


def grad_inputs(grad, dydx, dydx_mag=None):
    """(N, D): sum over levels and channels of grad (L, N, F) times dy_dx (N, L, D, F), and the same sum of magnitudes (with the edges'
    magnitudes dydx_mag when given)."""
    g = torch.as_tensor(grad).double().permute(1, 0, 2).unsqueeze(2)        # (N, L, 1, F)
    return (g * dydx).sum((1, 3)), (g.abs() * (dydx.abs() if dydx_mag is None else dydx_mag)).sum((1, 3))


def grad_embeddings(inputs, emb, offsets, resolutions, n_levels, grad, **kw):
    """Autograd embedding gradient of forward() under grad (L, N, F), and the per-element sum of contribution magnitudes (|grad|)."""
    e = torch.as_tensor(emb).double().clone().requires_grad_(True)
    y = forward(inputs, e, offsets, resolutions, n_levels, **kw)
    g = torch.as_tensor(grad).double()
    ge, = torch.autograd.grad(y, e, g, retain_graph=True)
    ga, = torch.autograd.grad(y, e, g.abs())
    return ge, ga
