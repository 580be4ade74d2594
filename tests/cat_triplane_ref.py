"""The multi-scale tri-plane feature contract (include/gauspcc.h: gsge_msplane_forward), restated in torch for the tests of
gauspcc_amd.cat_triplane.

`sample` is the contract in plain tensor operations with a hand-written border-padded bilinear step (any dtype; the tests use float64),
`closed_form_grads` its plane and coordinate gradients written out, `torch_formula` the float32 sequence a framework runs (rounded plane
copies, one grid_sample per level and plane, cats and level sums; the yardstick of the accuracy criterion), `near_texel_boundary` the
points whose coordinate gradient is discontinuous.  The CPU tests pin `sample` to the reference's recorded output
(tests/golden/cat_triplane.npz) and `closed_form_grads` to its autograd gradients.

A transform is a dict: aabb (2, 3) and, for the contract path, pca_mean (3), rotation (3, 3), variance (3), con_aabb (2, 3)."""
import torch

PAIRS = ((0, 1), (0, 2), (1, 2))     # plane p reads these components of the normalised point, the first along W

# (name, N, C, resolution, multipliers, levels to run, cluster): the cases of tests/test_gpu_cat_triplane.py
CASES = [("one", 1, 1, (2, 2, 2), (1,), (2,), False),
         ("tiny", 7, 1, (2, 2, 2), (1,), (2,), False),
         ("odd", 65, 3, (5, 7, 3), (1, 2), (2,), False),
         ("ref_c", 1000, 72, (9, 6, 11), (1, 2), (2,), False),
         ("cluster", 5000, 50, (16, 16, 16), (1, 2), (2,), True),
         ("three", 300, 8, (4, 5, 6), (1, 2, 4), (1, 2, 3), False)]
SEEDS = {"one": 1, "tiny": 2, "odd": 3, "ref_c": 4, "cluster": 5, "three": 6}


def plane_shapes(resolution, multipliers):
    """[(H, W)] in (level, plane) order: (m ry, m rx), (m rz, m rx), (m rz, m ry)"""
    return [(m * resolution[j], m * resolution[i]) for m in multipliers for i, j in PAIRS]


def contract_to_unisphere(x):
    """x (N, 3) after the PCA step -> [0, 1]^3: the unit ball keeps its place, the rest is drawn into radius 2 (NaN at the origin, as the
    reference's blend of both branches gives)"""
    x = ((x + 1) / 2) * 2 - 1
    mag = torch.linalg.norm(x, dim=-1, keepdim=True)
    m = (mag > 1).to(x.dtype)
    x = (2 - 1 / mag) * (x / mag) * m + x * (1 - m)
    return x / 4 + 0.5


def to_unit_box(pts, aabb):
    """the plain path: the box aabb becomes [-1, 1]^3"""
    return (pts - aabb[0]) * (2 / (aabb[1] - aabb[0])) - 1


def contracted_to_box(y, aabb, con_aabb):
    """the contract path's last step: the box con_aabb of contracted points becomes the box aabb"""
    return (y - con_aabb[0]) * ((aabb[1] - aabb[0]) / (con_aabb[1] - con_aabb[0])) + aabb[0]


def normalised(pts, xf, contract):
    """g (N, 3)"""
    if not contract:
        return to_unit_box(pts, xf["aabb"])
    q = ((pts - xf["pca_mean"]) @ xf["rotation"]) / xf["variance"]
    return contracted_to_box(contract_to_unisphere(q), xf["aabb"], xf["con_aabb"])


def pixels(g, p, H, W):
    """unclamped pixel coordinates (along W, along H) of plane p"""
    i, j = PAIRS[p]
    return (g[:, i] + 1) / 2 * (W - 1), (g[:, j] + 1) / 2 * (H - 1)


def quantised(v):
    return torch.round(v * 16) / 16


def _corners(ux, uy, H, W):
    """[(flat index, weight, d weight / d ix, d weight / d iy)] of the four corners; the clamped coordinates' pass masks"""
    ix, iy = ux.clamp(0, W - 1), uy.clamp(0, H - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = []
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xc, yc = x0 + dx, y0 + dy
        wx, wy = 1 - (ix - xc).abs(), 1 - (iy - yc).abs()
        ok = ((xc < W) & (yc < H)).to(ux.dtype)
        idx = (yc.clamp(0, H - 1) * W + xc.clamp(0, W - 1)).long()
        out.append((idx, wx * wy * ok, wy * ok * (1.0 if dx else -1.0), wx * ok * (1.0 if dy else -1.0)))
    return out, ((ux > 0) & (ux < W - 1)).to(ux.dtype), ((uy > 0) & (uy < H - 1)).to(ux.dtype)


def _used(l, level):
    return l == 0 or level > l


def sample(pts, grids, level, quantise, xf, contract):
    """The contract: pts (N, 3), grids [[(C, H, W)] * 3] * L -> (N, L * 3 * C); rows of points whose g is not finite are zero."""
    g = normalised(pts, xf, contract)
    finite = torch.isfinite(g).all(-1)
    g = torch.where(finite[:, None], g, torch.zeros_like(g))
    blocks, run = [], None
    for l, planes in enumerate(grids):
        if _used(l, level):
            reads = []
            for p, plane in enumerate(planes):
                C, H, W = plane.shape[-3:]
                flat = (quantised(plane) if quantise else plane).reshape(C, H * W)
                corners, _, _ = _corners(*pixels(g, p, H, W), H, W)
                reads.append(sum((flat[:, idx] * w).t() for idx, w, _, _ in corners))
            t = torch.cat(reads, dim=1)
            run = t if run is None else t + run
        blocks.append(run)
    return torch.cat(blocks, dim=1) * finite[:, None].to(pts.dtype)


def closed_form_grads(pts, grids, level, quantise, xf, contract, grad_out):
    """([d plane], d pts) of sum(sample(...) * grad_out), written out; d pts is None with contract (the reference detaches the points)."""
    g = normalised(pts, xf, contract)
    finite = torch.isfinite(g).all(-1)
    g = torch.where(finite[:, None], g, torch.zeros_like(g))
    L = len(grids)
    C = grids[0][0].shape[-3]
    go = (grad_out * finite[:, None].to(pts.dtype)).reshape(-1, L, 3, C)
    gps, gg = [], torch.zeros_like(g)
    for l, planes in enumerate(grids):
        up = go[:, l:].sum(1) if _used(l, level) else torch.zeros_like(go[:, 0])      # (N, 3, C)
        for p, plane in enumerate(planes):
            _, H, W = plane.shape[-3:]
            flat = (quantised(plane) if quantise else plane).reshape(C, H * W)
            corners, inx, iny = _corners(*pixels(g, p, H, W), H, W)
            gp = torch.zeros(C, H * W, dtype=pts.dtype)
            gix, giy = torch.zeros_like(g[:, 0]), torch.zeros_like(g[:, 0])
            for idx, w, wdx, wdy in corners:
                gp.index_add_(1, idx, (up[:, p] * w[:, None]).t())
                dot = (flat[:, idx].t() * up[:, p]).sum(1)
                gix += dot * wdx
                giy += dot * wdy
            gps.append(gp.reshape(plane.shape))
            i, j = PAIRS[p]
            gg[:, i] += gix * inx * (W - 1) / 2
            gg[:, j] += giy * iny * (H - 1) / 2
    if contract:
        return gps, None
    return gps, gg * (2 / (xf["aabb"][1] - xf["aabb"][0]))


def torch_formula(pts, grids, level, quantise, xf, contract):
    """The float32 sequence a framework runs: the transform in tensor operations, rounded copies of the planes behind a straight-through
    estimator, one grid_sample call per level and plane, a cat per level, the level sums and a final cat.  grids: [1, C, H, W] planes."""
    if contract:
        q = pts - xf["pca_mean"]
        q = torch.matmul(q, xf["rotation"])
        q = q / xf["variance"]
        g = contract_to_unisphere(q.detach())
        c0, c1, a0, a1 = xf["con_aabb"][0], xf["con_aabb"][1], xf["aabb"][0], xf["aabb"][1]
        g = (g - c0) * ((a1 - a0) / (c1 - c0)) + a0
    else:
        g = (pts - xf["aabb"][0]) * (2.0 / (xf["aabb"][1] - xf["aabb"][0])) - 1.0
    out = []
    for l, planes in enumerate(grids):
        reads = []
        if not _used(l, level):
            out.append(out[-1])
            continue
        for p, plane in enumerate(planes):
            if quantise:
                y = plane * 16
                plane = (y + (torch.round(y) - y).detach()) / 16
            coords = g[:, list(PAIRS[p])].reshape(1, 1, -1, 2)
            f = torch.nn.functional.grid_sample(plane, coords, align_corners=True, mode='bilinear', padding_mode='border')
            reads.append(f.reshape(plane.shape[1], -1).transpose(0, 1))
        t = torch.cat(reads, dim=1)
        out.append(t + out[-1] if l else t)
    return torch.cat(out, dim=-1)


def near_texel_boundary(pts, shapes, xf, contract, tol=1e-3):
    """(N,) bool: on some plane the float64 pixel coordinate lies within tol of an integer of [0, size - 1] (the coordinate gradient is
    discontinuous there, and at the two ends the clamp's mask flips).  Points further outside the plane than tol are clamped in every
    precision and are not flagged.  shapes: [(H, W)] in (level, plane) order."""
    g = normalised(pts.double(), {k: v.double() for k, v in xf.items()}, contract)
    flag = torch.zeros(pts.shape[0], dtype=torch.bool)
    for i, (H, W) in enumerate(shapes):
        for u, size in zip(pixels(g, i % 3, H, W), (W, H)):
            flag |= ((u - torch.round(u)).abs() < tol) & (u > -tol) & (u < size - 1 + tol)
    return flag


# ------------------------------------------------------------------ the tests' inputs
def transform(seed, dtype=torch.float32):
    """A rotation that is no permutation, unequal variances, a mean off the origin, a con_aabb inside the contraction's range (so points
    are clamped on every side) and an aabb whose first row is the upper corner, as TriPlaneField's constructor builds it."""
    g = torch.Generator().manual_seed(1000 + seed)
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    return {"pca_mean": torch.tensor([0.3, -0.2, 0.1], dtype=dtype), "rotation": q.to(dtype), "variance": torch.tensor([1.5, 0.8, 1.1], dtype=dtype),
            "aabb": torch.tensor([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]], dtype=dtype),
            "con_aabb": torch.tensor([[0.30, 0.28, 0.33], [0.72, 0.69, 0.70]], dtype=dtype)}


def plain_aabb(dtype=torch.float32):
    """the normalize_aabb path's box: g = -pts / 2 exactly (the first row is the upper corner: a negative scale)"""
    return {"aabb": torch.tensor([[2.0, 2.0, 2.0], [-2.0, -2.0, -2.0]], dtype=dtype)}


def make_planes(C, resolution, multipliers, seed):
    """[[ (1, C, H, W) ] * 3] * L float32: values of a few sixteenths, and in every plane three texels whose 16 v is exactly on .5
    (0.5, 1.5, -2.5: ties go to 0, 2, -2)"""
    g = torch.Generator().manual_seed(2000 + seed)
    grids, shapes = [], plane_shapes(resolution, multipliers)
    for l in range(len(multipliers)):
        level = []
        for H, W in shapes[3 * l:3 * l + 3]:
            p = torch.randn(1, C, H, W, generator=g) * 0.2
            flat = p.view(-1)
            flat[0], flat[1], flat[-1] = 0.5 / 16, 1.5 / 16, -2.5 / 16
            level.append(p)
        grids.append(level)
    return grids


def make_points(N, seed, contract, cluster=False):
    """(N, 3) float32.  The first point is clamped in every component (with the three pairings: the left and the bottom border of plane
    0, the top border of plane 1, the right border of plane 2), the second at the opposite borders, the third (cases of 20 points and
    more: it is one the near-boundary mask leaves out) sits on texel centres (on the normalize_aabb path g = (0, -1, 1) exactly: the
    middle of an odd size, the first and the last texel); then a mix of points
    inside, just outside and far outside the planes.  cluster: half the points inside one texel of the finest level.
    With contract the points are laid out behind the PCA step (inside the unit ball, outside it, far away) and mapped back."""
    g = torch.Generator().manual_seed(3000 + seed)
    kind = torch.arange(N) % 8
    u = torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1
    if contract:
        xf = transform(seed, torch.float64)
        q = torch.where((kind < 3)[:, None], u * 0.55, torch.where((kind < 6)[:, None], u * 1.6, u * 4.0))
        q = torch.where((kind == 7)[:, None], u * 60.0, q)
        special = torch.tensor([[-3.0, 3.0, -3.0], [3.0, -3.0, 3.0], [0.0, 0.0, 0.25]], dtype=torch.float64)
        q[:min(N, 3 if N >= 20 else 2)] = special[:min(N, 3 if N >= 20 else 2)]
        if cluster:
            q[N // 2:] = torch.tensor([0.11, -0.07, 0.05], dtype=torch.float64) + (torch.rand(N - N // 2, 3, generator=g, dtype=torch.float64) - 0.5) * 2e-3
        pts = (q * xf["variance"]) @ xf["rotation"].t() + xf["pca_mean"]
    else:
        gg = torch.where((kind < 5)[:, None], u, torch.where((kind < 7)[:, None], u * 1.2, u * 5.0))
        special = torch.tensor([[-1.5, 1.5, -1.5], [1.5, -1.5, 1.5], [0.0, -1.0, 1.0]], dtype=torch.float64)
        gg[:min(N, 3 if N >= 20 else 2)] = special[:min(N, 3 if N >= 20 else 2)]
        if cluster:
            gg[N // 2:] = torch.tensor([0.31, -0.27, 0.22], dtype=torch.float64) + (torch.rand(N - N // 2, 3, generator=g, dtype=torch.float64) - 0.5) * 2e-3
        pts = -2.0 * gg
    return pts.to(torch.float32)


def make_case(name, contract):
    """(pts, grids, transform, (H, W) shapes) of a case, float32 on the CPU"""
    _, N, C, res, mult, _, cluster = next(c for c in CASES if c[0] == name)
    seed = SEEDS[name]
    return (make_points(N, seed, contract, cluster), make_planes(C, res, mult, seed), transform(seed) if contract else plain_aabb(),
            plane_shapes(res, mult))


def as64(grids):
    return [[p.double().reshape(p.shape[-3:]) for p in level] for level in grids]


def xf64(xf):
    return {k: v.double() for k, v in xf.items()}


def borders_clamped(pts, shapes, xf, contract):
    """{(plane index, 'left' | 'right' | 'top' | 'bottom')} that some point is clamped at (float64)"""
    g = normalised(pts.double(), xf64(xf), contract)
    g = g[torch.isfinite(g).all(-1)]
    hit = set()
    for i, (H, W) in enumerate(shapes):
        ux, uy = pixels(g, i % 3, H, W)
        for name, cond in (("left", ux < 0), ("right", ux > W - 1), ("top", uy < 0), ("bottom", uy > H - 1)):
            if bool(cond.any()):
                hit.add((i, name))
    return hit


def on_texel_centre(pts, shapes, xf, contract, interior=False):
    """some point's float64 pixel coordinates, clamped as the sampler clamps them, are both integers on some plane (all the weight on
    one texel); interior: without the help of the clamp"""
    g = normalised(pts.double(), xf64(xf), contract)
    for i, (H, W) in enumerate(shapes):
        ux, uy = pixels(g, i % 3, H, W)
        inside = (ux >= 0) & (ux <= W - 1) & (uy >= 0) & (uy <= H - 1)
        if not interior:
            ux, uy = ux.clamp(0, W - 1), uy.clamp(0, H - 1)
        if bool(((ux == torch.round(ux)) & (uy == torch.round(uy)) & (inside | (not interior))).any()):
            return True
    return False
