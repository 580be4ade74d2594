"""gauspcc_amd.densify on the device: accumulate_stats, front / finish and compact_rows bit-exact against the numpy restatement
(tests/densify_ref.py) across the sizes at which the scans change kernels; the reference's own results (tests/golden/densify.npz); the
torch sequence run on the GPU behind the real chain of a HAC-shaped model; no host synchronisation in training_statis; the deferred error
of ill-formed masks; bitwise repeatability across runs and streams."""
import math
import os
import types

import numpy as np
import pytest
import torch

from gauspcc_amd import densify
from tests import densify_ref as dr
from tests.test_densify_ref_cpu import GOLDEN, NAMES, SUMS, compare, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
# around one look-back tile (4096 words) and around the largest single-launch scan (16384 words; the scans run over N + 1 words)
SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 100_000]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32).reshape(-1)).view(np.uint32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(N, K, vis, seed, sel_frac=0.6, filt_frac=0.7, S0=False):
    """numpy inputs of one call; vis: fraction of visible anchors or None (no mask).  grad has row stride 3 and a NaN third column."""
    rng = np.random.default_rng([N, K, seed])
    visible = None if vis is None else (rng.random(N) < vis if 0 < vis < 1 else np.full(N, bool(vis)))
    V = N if visible is None else int(visible.sum())
    opacity = rng.standard_normal(V * K).astype(F32)
    opacity[rng.random(V * K) < 0.05] = -0.0
    selection = np.zeros(V * K, bool) if S0 else rng.random(V * K) < sel_frac
    S = int(selection.sum())
    update_filter = rng.random(S) < filt_frac
    grad = np.full((S, 3), np.nan, F32)
    grad[:, :2] = (rng.standard_normal((S, 2)) * 0.001).astype(F32)
    acc = (rng.random(N).astype(F32) * 10, rng.integers(0, 50, N).astype(F32), rng.random(N * K).astype(F32), rng.integers(0, 50, N * K).astype(F32))
    return dict(visible=visible, opacity=opacity, selection=selection, update_filter=update_filter, grad=grad), acc


def _device_stats(inp, acc, K):
    d = [_t(a).view(-1, 1) for a in acc]
    densify.accumulate_stats(*d, _t(inp["grad"]), _t(inp["opacity"]).view(-1, 1), _t(inp["update_filter"]), _t(inp["selection"]),
                             None if inp["visible"] is None else _t(inp["visible"]), K)
    return [t.cpu().numpy().reshape(-1) for t in d]


def _check_stats(N, K, vis, seed=0, **kw):
    inp, acc = _inputs(N, K, vis, seed, **kw)
    want = dr.stats(acc, inp["visible"], inp["opacity"], inp["selection"], inp["update_filter"], inp["grad"], K)
    got = _device_stats(inp, acc, K)
    densify.check(DEV)
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(_bits(g), _bits(w)), (name, N, K, vis, int(np.sum(_bits(g) != _bits(w))))
    return inp, want, acc


@pytest.mark.parametrize("N", SIZES)
def test_stats_bit_exact_sizes(N):
    inp, want, acc = _check_stats(N, 10, 0.5)
    if N >= 63:
        assert not np.array_equal(want[2], acc[2]) and not np.isnan(want[2]).any()   # something moved, and the NaN column was not read


@pytest.mark.parametrize("K", [1, 5, 10, 11])
@pytest.mark.parametrize("vis", [0.0, 0.5, 1.0, None])
def test_stats_bit_exact_offsets_and_visibility(K, vis):
    _check_stats(4097, K, vis, seed=1)
    _check_stats(65, K, vis, seed=2)


def test_stats_wide_rows():
    """two anchors and one anchor per workgroup, and the widest row the kernel takes"""
    from gauspcc_amd import _lib

    for K in (100, 128, 256):
        _check_stats(65, K, 0.5, seed=7)
    with pytest.raises(_lib.GpccError):
        _check_stats(3, 257, 0.5, seed=7)


def test_stats_no_selection_and_nothing_passing():
    inp, want, acc = _check_stats(4097, 10, 0.5, seed=3, S0=True)                   # S = 0
    assert inp["update_filter"].shape[0] == 0 and np.array_equal(want[2], acc[2]) and not np.array_equal(want[0], acc[0])
    inp, want, acc = _check_stats(4097, 5, 0.5, seed=4, filt_frac=0.0)              # no row passes the filter
    assert inp["update_filter"].shape[0] > 0 and np.array_equal(want[3], acc[3]) and not np.array_equal(want[1], acc[1])
    inp, want, acc = _check_stats(300, 5, 1.0, seed=5, sel_frac=1.0, filt_frac=1.0)  # every entry selected and passing
    assert np.array_equal(want[3], acc[3] + 1)


def test_stats_strided_and_wide_grad():
    """grad as a column slice of a wider tensor (row stride 5) and a non-unit column stride (copied by the wrapper)"""
    K, N = 10, 1000
    inp, acc = _inputs(N, K, 0.5, 6)
    want = dr.stats(acc, inp["visible"], inp["opacity"], inp["selection"], inp["update_filter"], inp["grad"], K)
    S = inp["grad"].shape[0]
    wide = torch.full((S, 5), float("nan"), device=DEV)
    wide[:, 1:3] = _t(inp["grad"][:, :2])
    for g in (wide[:, 1:4], _t(np.ascontiguousarray(inp["grad"].T)).T):
        d = [_t(a).view(-1, 1) for a in acc]
        densify.accumulate_stats(*d, g, _t(inp["opacity"]), _t(inp["update_filter"]), _t(inp["selection"]), _t(inp["visible"]), K)
        for t, w in zip(d, want):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(w))


def _finish_case(N0, K, appended, seed):
    rng = np.random.default_rng([N0, K, appended, seed])
    N1 = N0 + appended
    og, od = rng.random(N0 * K).astype(F32), rng.integers(0, 4, N0 * K).astype(F32)
    og[od == 0] = 0
    if N0 * K > 4:
        og[:2], od[:2] = (1.0, -1.0), (0.0, 0.0)           # x / 0 = +-inf stays, 0 / 0 -> 0
    ad = np.concatenate([rng.integers(0, 4, N0).astype(F32), np.zeros(appended, F32)])
    oa = (rng.random(N1).astype(F32) * ad).astype(F32)
    return og, od, oa, ad, N1


@pytest.mark.parametrize("N0", SIZES)
@pytest.mark.parametrize("appended", [0, 37])
def test_front_and_finish_bit_exact(N0, appended):
    K = 10 if N0 != 65 else 11
    og, od, oa, ad, N1 = _finish_case(N0, K, appended, 0)
    gn_w, om_w = dr.front(og, od, 1.35)
    gn, om = densify.front(_t(og).view(-1, 1), _t(od).view(-1, 1), 1.35)
    assert np.array_equal(_bits(gn.cpu().numpy()), _bits(gn_w)) and np.array_equal(om.cpu().numpy(), om_w)
    want = dr.finish(og, od, om_w, oa, ad, K, 1.7, 0.4)
    got = densify.finish(_t(og).view(-1, 1), _t(od).view(-1, 1), om, _t(oa).view(-1, 1), _t(ad).view(-1, 1), K, 1.7, 0.4)
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    n2 = N1 - int(want[0].sum())
    for g, w, rows in zip(got[1:], want[1:], (n2 * K, n2 * K, n2, n2)):
        assert tuple(g.shape) == (rows, 1) and np.array_equal(_bits(g.cpu().numpy()), _bits(w))
    if N0 >= 63:
        assert 0 < want[0].sum() < N1 and 0 < om_w.sum() < om_w.size


def test_finish_prunes_everything_or_nothing():
    K, N = 5, 300
    og, od = np.ones(N * K, F32), np.ones(N * K, F32)
    for oa_val, n2 in ((0.0, 0), (9.0, N)):
        oa, ad = np.full(N, oa_val, F32), np.full(N, 3.0, F32)
        om = torch.zeros(N * K, dtype=torch.bool, device=DEV)
        got = densify.finish(_t(og), _t(od), om, _t(oa), _t(ad), K, 1.7, 0.4)
        want = dr.finish(og, od, np.zeros(N * K, bool), oa, ad, K, 1.7, 0.4)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and got[3].shape[0] == n2
        for g, w in zip(got[1:], want[1:]):
            assert np.array_equal(_bits(g.cpu().numpy()), _bits(w))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("keep_frac", [0.5, 1.0, 0.0])
def test_compact_rows_bit_exact(N, keep_frac):
    rng = np.random.default_rng([N, int(keep_frac * 10)])
    keep = rng.random(N) < keep_frac if 0 < keep_frac < 1 else np.full(N, bool(keep_frac))
    shapes = [(N, 1), (N, 3), (N, 50), (N, 257)] if N <= 16385 else [(N, 1), (N, 3), (N, 50)]
    shapes += [(N,), (N, 10, 3)]
    mats = [rng.standard_normal(s).astype(F32) for s in shapes]
    for m in mats:
        if m.size:
            m.reshape(-1)[0] = np.nan
    got = densify.compact_rows(_t(keep), *[_t(m) for m in mats])
    want = dr.compact(keep, *mats)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(g.shape) == w.shape and g.dtype == torch.float32 and np.array_equal(_bits(g.cpu().numpy()), _bits(w))
    assert densify.compact_rows(_t(keep)) == []


def test_compact_rows_32_tensors_and_a_transposed_one():
    N = 1000
    rng = np.random.default_rng(3)
    keep = rng.random(N) < 0.3
    mats = [rng.standard_normal((N, 1 + i % 7)).astype(F32) for i in range(31)]
    tr = rng.standard_normal((4, N)).astype(F32)
    got = densify.compact_rows(_t(keep), *[_t(m) for m in mats], _t(tr).T)
    for g, w in zip(got, dr.compact(keep, *mats, tr.T)):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w))


# ------------------------------------------------------------------ the reference's own results
class _Model:
    """what the two methods touch on a framework's GaussianModel, with a growing stand-in that appends zero rows"""

    def __init__(self, N, K, appended=0, device=DEV):
        self.__dict__.update(vars(dr.model(N, K, torch.float32, lib="torch", device=device)))
        self.appended, self._n = appended, N
        self.pruned = None

    @property
    def get_anchor(self):
        return torch.empty(self._n, 3, device=self.anchor_demon.device)

    def anchor_growing(self, grads_norm, threshold, offset_mask):
        self.grads_norm, self.threshold, self.offset_mask = grads_norm.clone(), threshold, offset_mask.clone()
        for k in ("opacity_accum", "anchor_demon"):
            setattr(self, k, torch.cat([getattr(self, k), torch.zeros(self.appended, 1, device=self.anchor_demon.device)], dim=0))
        self._n += self.appended

    def prune_anchor(self, mask):
        self.pruned = mask.clone()
        self._n -= int(mask.sum())

    training_statis = densify.training_statis
    adjust_anchor = densify.adjust_anchor


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_against_reference_fixture(golden, name):
    c = load_case(golden, name)
    m = _Model(c["N"], c["K"], c["appended"])
    for it in c["iters"]:
        vp = types.SimpleNamespace(grad=_t(it["grad"]))
        m.training_statis(vp, _t(it["opacity"]).view(-1, 1), _t(it["update_filter"]), _t(it["selection"]), _t(it["visible"]))
    np_ = lambda t: t.cpu().numpy().reshape(-1)
    got = {"stats_" + k: np_(getattr(m, k)) for k in NAMES}
    ci, st = c["check_interval"], float(golden["success_threshold"])
    m.adjust_anchor(ci, st, float(golden["grad_threshold"]), float(golden["min_opacity"]))
    assert m.threshold == float(golden["grad_threshold"])
    got.update({"after_" + k: np_(getattr(m, k)) for k in NAMES})
    got.update(grads_norm=np_(m.grads_norm), offset_mask=np_(m.offset_mask), prune_mask=np_(m.pruned), max_radii2D_len=np.int64(m.max_radii2D.shape[0]))
    assert tuple(m.offset_denom.shape) == (m.max_radii2D.shape[0] * c["K"], 1) and tuple(m.anchor_demon.shape) == (m.max_radii2D.shape[0], 1)
    compare(got, c["want"], name + " device")
    for k in SUMS:   # the measured ratio to the reference's own float32 rounding (profiles/r07_densify.txt)
        ref = float(c["want"][k + "/f32_vs_f64"])
        err = float(np.abs(got[k].astype(np.float64) - c["want"][k]).max(initial=0.0))
        print(f"RATIO {name} {k}: device error {err:.3e} / reference f32-vs-f64 {ref:.3e}" + (f" = {err / ref:.2f}" if ref > 0 else ""))


def test_none_mask_is_all_anchors():
    K, N = 10, 777
    inp, acc = _inputs(N, K, 1.0, 9)
    a = _device_stats(inp, acc, K)
    b = _device_stats(dict(inp, visible=None), acc, K)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------ the torch sequence behind the real chain
def _scene(n, seed=3):
    from gauspcc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from gauspcc_amd.synth import SyntheticGaussianModel

    pc = SyntheticGaussianModel(n, seed=seed, device=DEV)
    with torch.no_grad():   # opacity outputs well away from 0 (as tests/test_gpu_ng_train.py); footprints of a few pixels
        pc.mlp_opacity[2].weight.mul_(0.05)
        pc.mlp_opacity[2].bias.copy_(torch.tensor([2.0, -2.0] * (pc.n_offsets // 2) + [2.0] * (pc.n_offsets % 2), device=DEV))
        pc._scaling.add_(3.0)
        a = pc.get_anchor
        ctr, ext = a.mean(dim=0), float((a.max(dim=0).values - a.min(dim=0).values).max())
    W = H = 96
    fov, zn, zf = math.radians(60), 0.01, 100.0
    P = torch.zeros(4, 4, device=DEV)
    P[0, 0] = P[1, 1] = 1 / math.tan(fov / 2); P[3, 2] = 1.0; P[2, 2] = zf / (zf - zn); P[2, 3] = -(zf * zn) / (zf - zn)
    views = []
    for dx in (0.0, 0.3, -0.4):
        eye = ctr + torch.tensor([dx * ext, 0.0, -1.1 * ext], device=DEV)
        Rt = torch.eye(4, device=DEV); Rt[:3, 3] = -eye
        view = Rt.T.contiguous()
        st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(fov / 2), tanfovy=math.tan(fov / 2), bg=torch.zeros(3, device=DEV),
                                           scale_modifier=1.0, viewmatrix=view, projmatrix=(view @ P.T).contiguous(), sh_degree=0, campos=eye,
                                           prefiltered=False, debug=False)
        views.append((types.SimpleNamespace(camera_center=eye), GaussianRasterizer(st)))
    return pc, views


def test_against_torch_sequence_on_real_chain():
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians

    N, K = 3000, 10
    pc, views = _scene(N)
    ours, ref = _Model(N, K, appended=41), _Model(N, K, appended=41)
    f64 = dr.model(N, K, torch.float64, lib="torch", device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    target = torch.rand(3, 96, 96, device=DEV, generator=gen)
    for it, (cam, rast) in enumerate(views):
        vis = torch.rand(N, device=DEV, generator=gen) < 0.6
        xyz, color, opacity, scaling, rot, neural_opacity, mask = generate_neural_gaussians(cam, pc, vis, is_training=True, step=0)[:7]
        screen = torch.zeros_like(xyz, requires_grad=True)
        image, radii = rast(means3D=xyz, means2D=screen, shs=None, colors_precomp=color, opacities=opacity, scales=scaling, rotations=rot, cov3D_precomp=None)
        ((image - target) ** 2).mean().backward()
        filt = radii > 0
        assert 0 < int(filt.sum()) and float(screen.grad[filt, :2].abs().max()) > 0
        ours.training_statis(screen, neural_opacity, filt, mask, vis)
        dr.torch_sequence_statis(ref, screen.grad, neural_opacity, filt, mask, vis)
        dr.torch_sequence_statis(f64, screen.grad.double(), neural_opacity.double(), filt, mask, vis)
    densify.check(DEV)
    # the float sums: the torch sequence's own float32 error against its float64 run sets the tolerance
    for k in NAMES:
        g, r, e = (getattr(x, k).double().cpu().numpy().reshape(-1) for x in (ours, ref, f64))
        if k in ("anchor_demon", "offset_denom"):
            assert np.array_equal(g, r) and np.array_equal(g, e) and g.max() >= 2, k
            continue
        ref_err = float(np.abs(r - e).max())
        tol = np.maximum(4 * ref_err, np.spacing(np.abs(e).astype(F32)).astype(np.float64))
        err = np.abs(g - e)
        print(f"RATIO chain {k}: device error {err.max():.3e}, torch float32 error {ref_err:.3e}")
        assert np.all(err <= tol), (k, float(err.max()), ref_err)
    # thresholds between the values that occur, so that rounding decides nothing: min_opacity in a gap of the seen opacity levels
    ratio = (f64.opacity_accum / f64.anchor_demon.clamp(min=1)).view(-1)
    seen = ratio[f64.anchor_demon.view(-1) > 1.5].sort().values
    mid = int((seen[1:] - seen[:-1]).argmax()) + 1          # the widest gap: anchors on both sides of it
    min_opacity = float((seen[mid - 1] + seen[mid]) / 2)
    assert len(seen) > 10 and float(seen[mid] - seen[mid - 1]) > 1e-4 * min_opacity
    args = dict(check_interval=3, success_threshold=0.5, grad_threshold=0.0002, min_opacity=min_opacity)

    def grow(m, grads_norm, threshold, offset_mask):
        for k in ("opacity_accum", "anchor_demon"):
            setattr(m, k, torch.cat([getattr(m, k), torch.zeros(41, 1, device=DEV)], dim=0))

    out_r = dr.torch_sequence_adjust(ref, grow, **args)
    out_e = dr.torch_sequence_adjust(f64, grow, **args)
    ours.adjust_anchor(**args)
    assert all(torch.equal(a, b) for a, b in zip(out_r[1:], out_e[1:]))
    assert torch.equal(ours.offset_mask, out_e[1]) and torch.equal(ours.pruned, out_e[2])
    assert 0 < int(out_e[2].sum()) < N and 0 < int(out_e[1].sum()) < N * K
    assert ours.max_radii2D.shape[0] == N + 41 - int(out_e[2].sum()) == f64.anchor_demon.shape[0] == ours.anchor_demon.shape[0]
    triples = [(k, getattr(ours, k), getattr(ref, k), getattr(f64, k)) for k in NAMES] + [("grads_norm", ours.grads_norm, out_r[0], out_e[0])]
    for k, g, r, e in triples:
        g, r, e = (x.double().cpu().numpy().reshape(-1) for x in (g, r, e))
        assert g.shape == e.shape, k
        if k in ("anchor_demon", "offset_denom"):
            assert np.array_equal(g, e), k
            continue
        ref_err = float(np.abs(r - e).max())
        err = np.abs(g - e)
        print(f"RATIO chain after adjust_anchor {k}: device error {err.max():.3e}, torch float32 error {ref_err:.3e}")
        assert np.all(err <= np.maximum(4 * ref_err, np.spacing(np.abs(e).astype(F32)).astype(np.float64))), (k, float(err.max()), ref_err)


def test_no_host_sync():
    K, N = 10, 5000
    inp, acc = _inputs(N, K, 0.5, 11)
    m = _Model(N, K)
    args = (types.SimpleNamespace(grad=_t(inp["grad"])), _t(inp["opacity"]).view(-1, 1), _t(inp["update_filter"]), _t(inp["selection"]), _t(inp["visible"]))
    m.training_statis(*args)      # warm: the library's context, scan state and error words are created once
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(8, device=DEV).nonzero()   # the mode is live on this build
        m.training_statis(*args)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert float(m.anchor_demon.max()) == 2.0
    densify.check(DEV)


def test_deferred_error():
    K, N = 10, 5000
    inp, acc = _inputs(N, K, 0.5, 12)
    before = [a.copy() for a in acc]
    # (a) one more visible anchor than opacity has rows
    vis = inp["visible"].copy()
    vis[np.flatnonzero(~vis)[0]] = True
    got = _device_stats(dict(inp, visible=vis), acc, K)
    assert all(np.array_equal(_bits(g), _bits(b)) for g, b in zip(got, before))
    with pytest.raises(ValueError, match="anchor_visible_mask"):
        densify.check(DEV)
    densify.check(DEV)            # raised once
    # (b) one more selected entry than update_filter has
    sel = inp["selection"].copy()
    sel[np.flatnonzero(~sel)[0]] = True
    got = _device_stats(dict(inp, selection=sel), acc, K)
    assert all(np.array_equal(_bits(g), _bits(b)) for g, b in zip(got, before))
    m = _Model(N, K)
    with pytest.raises(ValueError, match="offset_selection_mask"):
        m.adjust_anchor()
    assert m.pruned is None
    # (c) both, then a well-formed call works and nothing is pending
    _device_stats(dict(inp, visible=vis, selection=sel), acc, K)
    with pytest.raises(ValueError, match="anchor_visible_mask.*offset_selection_mask"):
        densify.check(DEV)
    want = dr.stats(acc, inp["visible"], inp["opacity"], inp["selection"], inp["update_filter"], inp["grad"], K)
    got = _device_stats(inp, acc, K)
    densify.check(DEV)
    assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
    m.adjust_anchor()
    assert m.pruned is not None


def test_bitwise_repeatable_across_runs_and_streams():
    K, N = 10, 100_000
    inp, acc = _inputs(N, K, 0.5, 13)
    first = _device_stats(inp, acc, K)
    again = _device_stats(inp, acc, K)
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        other = _device_stats(inp, acc, K)
        og, od, oa, ad, N1 = _finish_case(N, K, 37, 1)
        om = _t(od > 1.35)
        fin_s = [t.cpu() for t in densify.finish(_t(og), _t(od), om, _t(oa), _t(ad), K, 1.7, 0.4)]
        keep = _t(ad[:N] > 1)
        rows_s = [t.cpu() for t in densify.compact_rows(keep, _t(og).view(N, K), _t(oa[:N]))]
    s.synchronize()
    fin = [t.cpu() for t in densify.finish(_t(og), _t(od), om, _t(oa), _t(ad), K, 1.7, 0.4)]
    rows = [t.cpu() for t in densify.compact_rows(keep, _t(og).view(N, K), _t(oa[:N]))]
    for a, b, c in zip(first, again, other):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    for a, b in zip(fin + rows, fin_s + rows_s):
        assert torch.equal(a, b)
    densify.check(DEV)


# ------------------------------------------------------------------ INTEGRATION.md's _prune_anchor_optimizer on compact_rows
def _prune_masked_copies(self, mask):
    """the frameworks' own form (HAC's skip list): one masked copy per parameter and Adam moment"""
    out = {}
    for group in self.optimizer.param_groups:
        if any(s in group['name'] for s in ('mlp', 'conv', 'feat_base', 'encoding')):
            continue
        st = self.optimizer.state.get(group['params'][0], None)
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][mask], st["exp_avg_sq"][mask]
            del self.optimizer.state[group['params'][0]]
        p = group["params"][0][mask].detach().clone()
        if group['name'] == "scaling":
            t = p[:, 3:]
            t[t > 0.05] = 0.05
        group["params"][0] = torch.nn.Parameter(p.requires_grad_(True))
        if st is not None:
            self.optimizer.state[group['params'][0]] = st
        out[group["name"]] = group["params"][0]
    return out


def _prune_compact_rows(self, mask):
    """INTEGRATION.md's rewrite"""
    nn = torch.nn
    groups = [g for g in self.optimizer.param_groups
              if not any(s in g['name'] for s in ('mlp', 'conv', 'feat_base', 'encoding'))]
    states = [self.optimizer.state.get(g['params'][0], None) for g in groups]
    tensors = [g['params'][0] for g in groups]
    for st in states:
        if st is not None:
            tensors += [st["exp_avg"], st["exp_avg_sq"]]
    kept = densify.compact_rows(mask, *tensors)
    moments = iter(kept[len(groups):])
    optimizable_tensors = {}
    for g, st, p in zip(groups, states, kept):
        if g['name'] == "scaling":
            p[:, 3:].clamp_(max=0.05)
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = next(moments), next(moments)
            del self.optimizer.state[g['params'][0]]
        g["params"][0] = nn.Parameter(p.requires_grad_(True))
        if st is not None:
            self.optimizer.state[g['params'][0]] = st
        optimizable_tensors[g["name"]] = g["params"][0]
    return optimizable_tensors


def test_prune_anchor_optimizer_on_compact_rows():
    N, K = 3001, 10
    shapes = dict(anchor=(N, 3), offset=(N, K, 3), mask=(N, K, 1), anchor_feat=(N, 50), opacity=(N, 1), scaling=(N, 6), rotation=(N, 4), mlp_opacity=(7, 5))
    gen = torch.Generator(device=DEV).manual_seed(2)
    init = {k: torch.randn(s, device=DEV, generator=gen) for k, s in shapes.items()}
    mask = torch.rand(N, device=DEV, generator=gen) < 0.7
    results = []
    for fn in (_prune_masked_copies, _prune_compact_rows):
        params = {k: torch.nn.Parameter(v.clone()) for k, v in init.items()}
        m = types.SimpleNamespace(optimizer=torch.optim.Adam([dict(params=[p], lr=1e-2, name=k) for k, p in params.items() if k != "rotation"]))
        m.optimizer.add_param_group(dict(params=[params["rotation"]], lr=1e-2, name="rotation"))   # a group without Adam state yet
        sum((p ** 2).sum() for k, p in params.items() if k != "rotation").backward()
        m.optimizer.step()
        out = fn(m, mask)
        assert set(out) == set(shapes) - {"mlp_opacity"}
        state = {g["name"]: m.optimizer.state.get(g["params"][0], None) for g in m.optimizer.param_groups}
        results.append((out, state))
    (a, sa), (b, sb) = results
    assert int(mask.sum()) == a["anchor"].shape[0] and float(b["scaling"].detach()[:, 3:].max()) <= float(F32(0.05))
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]) and b[k].requires_grad, k
        assert (sa[k] is None) == (sb[k] is None)
        if sa[k] is not None:
            assert torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"])
    assert sb["mlp_opacity"] is not None and sb["mlp_opacity"]["exp_avg"].shape == (7, 5)
