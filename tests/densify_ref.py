"""Restatements of the densification bookkeeping (gauspcc_amd/densify.py; contracts in include/gauspcc.h).

* `stats`, `front`, `finish`, `compact`: numpy, in the operation order the kernels are specified to use.  With dtype=np.float32 they are what
  the device must reproduce bit for bit; with dtype=np.float64 they are the twin that the fixture's float64 reference run is compared with.
* `torch_sequence_statis` / `torch_sequence_adjust`: the steps the four frameworks' `training_statis` and `adjust_anchor` take, written for
  this project's tests (boolean-mask indexing, `torch.norm`, the `anchors_mask.sum()` branch), to run on the CPU or the GPU.
* `make_case`: the seeded inputs of the fixture cases (tests/golden/make_densify_golden.py stores them in tests/golden/densify.npz).
"""
import types

import numpy as np

REL_MARGIN = 1e-3      # how far every compared float of a fixture case stays from its threshold, relatively
UPDATE_DEPTH, UPDATE_HIERARCHY_FACTOR = 3, 4   # anchor_growing's levels: threshold * (factor // 2) ** i


# ------------------------------------------------------------------ numpy restatements
def stats(acc, visible, opacity, selection, update_filter, grad, K, dtype=np.float32):
    """One training_statis call.  acc = (opacity_accum (N), anchor_demon (N), offset_gradient_accum (N K), offset_denom (N K)) of dtype;
    returns the new four, or None when a count disagrees with its shape (the device then writes nothing)."""
    oa, ad, og, od = (np.array(a, dtype=dtype).reshape(-1) for a in acc)
    N = ad.shape[0]
    visible = np.ones(N, bool) if visible is None else np.asarray(visible, bool).reshape(-1)
    opacity = np.asarray(opacity).reshape(-1).astype(dtype)
    selection = np.asarray(selection, bool).reshape(-1)
    update_filter = np.asarray(update_filter, bool).reshape(-1)
    V, S = opacity.shape[0] // K, update_filter.shape[0]
    if visible.sum() != V or selection.sum() != S:
        return None
    grad = np.asarray(grad).astype(dtype)
    clamped = np.where(opacity < 0, dtype(0), opacity).reshape(V, K)
    total = np.zeros(V, dtype)
    for k in range(K):                       # ascending k from 0, one rounded add per term
        total = total + clamped[:, k]
    vis = np.flatnonzero(visible)
    oa[vis] = oa[vis] + total
    ad[vis] = ad[vis] + dtype(1)
    sel = np.flatnonzero(selection)          # entry j of the (V, K) table; its rank in sel is s(j)
    hit = sel[update_filter]
    g = grad[update_filter]
    gx, gy = g[:, 0], g[:, 1]
    norm = np.sqrt(gx * gx + gy * gy)        # numpy rounds each product, the sum and the root once, in dtype
    dst = vis[hit // K] * K + hit % K
    og[dst] = og[dst] + norm
    od[dst] = od[dst] + dtype(1)
    return oa, ad, og, od


def front(og, od, offset_thr, dtype=np.float32):
    """(grads_norm, offset_mask) of adjust_anchor's head; the threshold is compared as a float32, as torch compares a Python scalar"""
    og, od = np.asarray(og, dtype).reshape(-1), np.asarray(od, dtype).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = og / od
    return np.where(np.isnan(g), dtype(0), np.abs(g)), od > dtype(np.float32(offset_thr))


def finish(og, od, offset_mask, oa, ad, K, anchor_thr, min_opacity, dtype=np.float32):
    """(prune (N1), og (N2 K), od (N2 K), oa (N2), ad (N2)) of adjust_anchor's tail; og, od, offset_mask are the old arrays (N0 K), oa, ad
    the grown ones (N1 >= N0)"""
    og, od, oa, ad = (np.asarray(a, dtype).reshape(-1) for a in (og, od, oa, ad))
    offset_mask = np.asarray(offset_mask, bool).reshape(-1)
    N1, N0 = ad.shape[0], od.shape[0] // K
    anchors_mask = ad > dtype(np.float32(anchor_thr))
    prune = (oa < dtype(np.float32(min_opacity)) * ad) & anchors_mask
    pad = np.zeros((N1 - N0) * K, dtype)
    og2 = np.concatenate([np.where(offset_mask, dtype(0), og), pad]).reshape(N1, K)[~prune].reshape(-1)
    od2 = np.concatenate([np.where(offset_mask, dtype(0), od), pad]).reshape(N1, K)[~prune].reshape(-1)
    oa2 = np.where(anchors_mask, dtype(0), oa)[~prune]
    ad2 = np.where(anchors_mask, dtype(0), ad)[~prune]
    return prune, og2, od2, oa2, ad2


def compact(keep, *mats):
    keep = np.asarray(keep, bool)
    return [np.asarray(m)[keep] for m in mats]


def level_thresholds(grad_threshold):
    return [grad_threshold * ((UPDATE_HIERARCHY_FACTOR // 2) ** i) for i in range(UPDATE_DEPTH)]


def margins_ok(oa, ad, grads_norm, min_opacity, grad_threshold):
    """The fixture's input conditions on one state: every opacity_accum at least a relative REL_MARGIN from min_opacity * anchor_demon and
    every grads_norm at least that far from each level's threshold (so float32 and float64 decide alike)."""
    oa, ad, gn = (np.asarray(a, np.float64).reshape(-1) for a in (oa, ad, grads_norm))
    t = np.float64(np.float32(min_opacity)) * ad
    ok = np.all((np.abs(oa - t) >= REL_MARGIN * np.maximum(np.abs(t), np.abs(oa))) & ((oa != t) | (ad == 0)))   # a never-seen anchor: 0 < 0 either way
    for th in level_thresholds(grad_threshold):
        ok &= bool(np.all(np.abs(gn - th) >= REL_MARGIN * th))
    return bool(ok)


# ------------------------------------------------------------------ the torch sequence
def torch_sequence_statis(m, grad, opacity, update_filter, offset_selection_mask, anchor_visible_mask=None):
    """training_statis as the frameworks run it: m holds n_offsets and the four accumulators ((N, 1) and (N K, 1)), updated in place"""
    import torch

    K = m.n_offsets
    temp = opacity.clone().view(-1).detach()
    temp[temp < 0] = 0
    temp = temp.view([-1, K])
    if anchor_visible_mask is None:
        anchor_visible_mask = torch.ones(m.anchor_demon.shape[0], dtype=torch.bool, device=m.anchor_demon.device)
    m.opacity_accum[anchor_visible_mask] += temp.sum(dim=1, keepdim=True)
    m.anchor_demon[anchor_visible_mask] += 1
    wide = anchor_visible_mask.unsqueeze(dim=1).repeat([1, K]).view(-1)
    combined = torch.zeros_like(m.offset_gradient_accum, dtype=torch.bool).squeeze(dim=1)
    combined[wide] = offset_selection_mask
    first = combined.clone()
    combined[first] = update_filter
    norm = torch.norm(grad[update_filter, :2], dim=-1, keepdim=True)
    m.offset_gradient_accum[combined] += norm
    m.offset_denom[combined] += 1


def torch_sequence_adjust(m, anchor_growing, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005):
    """adjust_anchor as the frameworks run it, up to the call of prune_anchor: anchor_growing(m, grads_norm, grad_threshold, offset_mask) grows
    m.opacity_accum / m.anchor_demon; returns (grads_norm, offset_mask, prune_mask) and leaves the four new accumulators on m"""
    import torch

    K = m.n_offsets
    grads = m.offset_gradient_accum / m.offset_denom
    grads[grads.isnan()] = 0.0
    grads_norm = torch.norm(grads, dim=-1)
    offset_mask = (m.offset_denom > check_interval * success_threshold * 0.5).squeeze(dim=1)
    anchor_growing(m, grads_norm, grad_threshold, offset_mask)
    N1 = m.anchor_demon.shape[0]
    for name in ("offset_denom", "offset_gradient_accum"):
        t = getattr(m, name)
        t[offset_mask] = 0
        setattr(m, name, torch.cat([t, torch.zeros([N1 * K - t.shape[0], 1], dtype=torch.int32, device=t.device)], dim=0))
    prune_mask = (m.opacity_accum < min_opacity * m.anchor_demon).squeeze(dim=1)
    anchors_mask = (m.anchor_demon > check_interval * success_threshold).squeeze(dim=1)
    prune_mask = torch.logical_and(prune_mask, anchors_mask)
    for name in ("offset_denom", "offset_gradient_accum"):
        setattr(m, name, getattr(m, name).view([-1, K])[~prune_mask].view([-1, 1]))
    if anchors_mask.sum() > 0:
        m.opacity_accum[anchors_mask] = 0.0
        m.anchor_demon[anchors_mask] = 0.0
    m.opacity_accum = m.opacity_accum[~prune_mask]
    m.anchor_demon = m.anchor_demon[~prune_mask]
    return grads_norm, offset_mask, prune_mask


# ------------------------------------------------------------------ fixture cases
# name: (N, K, visible, selection, iterations, appended anchors)
CASES = {
    "n1k1": (1, 1, "all", "some", 3, 0),
    "n65k10": (65, 10, "half", "some", 3, 0),
    "n257k5_grown": (257, 5, "half", "some", 3, 37),
    "n300k10": (300, 10, "half", "some", 1, 37),
    "n65k10_all": (65, 10, "all", "some", 3, 37),
    "n65k10_none": (65, 10, "none", "some", 3, 0),
    "n257k5_empty": (257, 5, "half", "empty", 1, 0),
}
MIN_OPACITY, GRAD_THRESHOLD, SUCCESS_THRESHOLD = 0.12, 0.0005, 0.9   # check_interval = the case's iterations: some anchors prune, some offsets pass


def make_case(name, attempt=0):
    """The seeded inputs of a fixture case: dict(N, K, appended, check_interval, iters=[dict(visible, opacity, selection, update_filter, grad)]).
    grad's third column is NaN: nothing may read it.  `attempt` reseeds (the generator looks for inputs that meet margins_ok)."""
    N, K, vmode, smode, iters, appended = CASES[name]
    rng = np.random.default_rng([sorted(CASES).index(name), attempt, 20])
    scale = (10.0 ** rng.uniform(-2.5, 0.0, N)).astype(np.float32)      # per-anchor opacity level: a spread of opacity_accum / anchor_demon
    out = []
    for _ in range(iters):
        visible = {"all": np.ones(N, bool), "none": np.zeros(N, bool), "half": rng.random(N) < 0.5}[vmode]
        V = int(visible.sum())
        opacity = (rng.standard_normal((V, K)) * scale[visible][:, None]).astype(np.float32).reshape(-1)
        selection = (opacity > 0) & (rng.random(V * K) < 0.9) if smode == "some" else np.zeros(V * K, bool)
        S = int(selection.sum())
        update_filter = rng.random(S) < 0.7
        grad = np.full((S, 3), np.nan, np.float32)
        grad[:, :2] = (rng.standard_normal((S, 2)) * 0.0008).astype(np.float32)
        out.append(dict(visible=visible, opacity=opacity, selection=selection, update_filter=update_filter, grad=grad))
    return dict(N=N, K=K, appended=appended, check_interval=iters, iters=out)


def model(N, K, dtype, lib="numpy", device=None):
    """A namespace with n_offsets and four zero accumulators of the frameworks' shapes"""
    if lib == "numpy":
        z = lambda n: np.zeros((n, 1), dtype)
    else:
        import torch
        z = lambda n: torch.zeros((n, 1), dtype=dtype, device=device)
    return types.SimpleNamespace(n_offsets=K, opacity_accum=z(N), anchor_demon=z(N), offset_gradient_accum=z(N * K), offset_denom=z(N * K))
