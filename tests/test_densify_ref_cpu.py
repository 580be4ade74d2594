"""tests/densify_ref.py against tests/golden/densify.npz (what the reference's own training_statis / adjust_anchor computed, float64, with
its measured float32 rounding; tests/golden/make_densify_golden.py), the fixture's input conditions, the torch sequence on the CPU, and
the argument errors of gauspcc_amd/densify.py that need no GPU."""
import os
import types

import numpy as np
import pytest
import torch

from tests import densify_ref as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify.npz")
NAMES = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def load_case(g, name):
    pre = name + "/"
    c = {k: int(g[pre + k]) for k in ("N", "K", "appended", "check_interval", "attempt")}
    c["iters"] = [{k: g[f"{pre}it{i}/{k}"] for k in ("visible", "opacity", "selection", "update_filter", "grad")} for i in range(c["check_interval"])]
    c["want"] = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre) and "/it" not in k}
    return c


def tolerance(want, key):
    """the issue's rule for a float sum: max(4 x the reference's own float32-vs-float64 difference, one float32 ulp of the value)"""
    v = want[key]
    return np.maximum(4.0 * float(want[key + "/f32_vs_f64"]), np.spacing(np.abs(v).astype(np.float32)).astype(np.float64))


def run_restatement(c, dtype, g):
    """the case through stats x iterations, front, a growing stand-in that appends zeros, finish -> dict named like the fixture"""
    N, K, ci = c["N"], c["K"], c["check_interval"]
    acc = (np.zeros(N, dtype), np.zeros(N, dtype), np.zeros(N * K, dtype), np.zeros(N * K, dtype))
    for it in c["iters"]:
        acc = dr.stats(acc, it["visible"], it["opacity"], it["selection"], it["update_filter"], it["grad"], K, dtype)
        assert acc is not None
    oa, ad, og, od = acc
    st, mo = float(g["success_threshold"]), float(g["min_opacity"])
    gn, om = dr.front(og, od, ci * st * 0.5, dtype)
    pad = np.zeros(c["appended"], dtype)
    prune, og2, od2, oa2, ad2 = dr.finish(og, od, om, np.concatenate([oa, pad]), np.concatenate([ad, pad]), K, ci * st, mo, dtype)
    return dict(stats_opacity_accum=oa, stats_anchor_demon=ad, stats_offset_gradient_accum=og, stats_offset_denom=od, grads_norm=gn, offset_mask=om,
                prune_mask=prune, after_offset_gradient_accum=og2, after_offset_denom=od2, after_opacity_accum=oa2, after_anchor_demon=ad2,
                max_radii2D_len=np.int64(len(ad2)))


EXACT = ("offset_mask", "prune_mask", "max_radii2D_len", "stats_anchor_demon", "stats_offset_denom", "after_anchor_demon", "after_offset_denom")
SUMS = ("stats_opacity_accum", "stats_offset_gradient_accum", "grads_norm", "after_opacity_accum", "after_offset_gradient_accum")


def compare(got, want, label):
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (label, k)
    for k in SUMS:
        assert got[k].shape == want[k].shape, (label, k)
        err = np.abs(got[k].astype(np.float64) - want[k])
        tol = tolerance(want, k)
        print(f"{label} {k}: max error {err.max(initial=0.0):.3e}, stored f32-vs-f64 {float(want[k + '/f32_vs_f64']):.3e}")
        assert np.all(err <= tol), (label, k, float(err.max()))


@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_fixture_inputs_are_the_seeded_cases_and_meet_the_conditions(golden, name):
    c = load_case(golden, name)
    N, K, _, _, iters, appended = dr.CASES[name]
    assert (c["N"], c["K"], c["check_interval"], c["appended"]) == (N, K, iters, appended)
    made = dr.make_case(name, c["attempt"])
    for a, b in zip(made["iters"], c["iters"]):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, k)
    w = c["want"]
    assert dr.margins_ok(w["stats_opacity_accum"], w["stats_anchor_demon"], w["grads_norm"], float(golden["min_opacity"]), float(golden["grad_threshold"]))
    st = float(golden["success_threshold"])
    for thr in (iters * st, iters * st * 0.5):      # the counts meet their thresholds only as integers: never equal
        assert thr != round(thr)
    assert all(np.isnan(it["grad"][:, 2]).all() for it in c["iters"])


def test_fixture_covers_what_it_should(golden):
    cases = {n: load_case(golden, n) for n in dr.CASES}
    assert {(c["N"], c["K"]) for c in cases.values()} >= {(1, 1), (65, 10), (300, 10), (257, 5)}
    assert {c["appended"] for c in cases.values() if c["check_interval"] == 3} == {0, 37}
    assert any(all(it["visible"].all() for it in c["iters"]) and c["N"] > 1 for c in cases.values())
    assert any(not any(it["visible"].any() for it in c["iters"]) for c in cases.values())
    assert any(not any(it["selection"].any() for it in c["iters"]) for c in cases.values())
    some = [c["want"] for c in cases.values()]
    assert any(0 < w["prune_mask"].sum() < len(w["prune_mask"]) for w in some) and any(0 < w["offset_mask"].sum() < len(w["offset_mask"]) for w in some)
    assert any(np.count_nonzero(w["after_offset_gradient_accum"]) for w in some)
    assert os.path.getsize(GOLDEN) <= 200 * 1024


@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_float64_restatement_equals_reference(golden, name):
    c = load_case(golden, name)
    compare(run_restatement(c, np.float64, golden), c["want"], name + " f64")


@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_float32_restatement_within_reference_rounding(golden, name):
    c = load_case(golden, name)
    got = run_restatement(c, np.float32, golden)
    assert all(got[k].dtype == np.float32 for k in SUMS)
    compare(got, c["want"], name + " f32")


@pytest.mark.parametrize("name", ["n65k10", "n257k5_grown"])
def test_torch_sequence_on_cpu_matches_restatement(golden, name):
    """the torch restatement and the numpy one agree on masks and counts, and on the float sums to the fixture's tolerance"""
    c = load_case(golden, name)
    m = dr.model(c["N"], c["K"], torch.float32, lib="torch")
    for it in c["iters"]:
        dr.torch_sequence_statis(m, torch.from_numpy(it["grad"]), torch.from_numpy(it["opacity"]).view(-1, 1), torch.from_numpy(it["update_filter"]),
                                 torch.from_numpy(it["selection"]), torch.from_numpy(it["visible"]))
    stats = {"stats_" + k: getattr(m, k).numpy().reshape(-1).copy() for k in NAMES}

    def grow(m, grads_norm, threshold, offset_mask):
        for k in ("opacity_accum", "anchor_demon"):
            setattr(m, k, torch.cat([getattr(m, k), torch.zeros(c["appended"], 1)], dim=0))

    ci, st = c["check_interval"], float(golden["success_threshold"])
    gn, om, prune = dr.torch_sequence_adjust(m, grow, ci, st, float(golden["grad_threshold"]), float(golden["min_opacity"]))
    got = dict(stats, grads_norm=gn.numpy(), offset_mask=om.numpy(), prune_mask=prune.numpy(), max_radii2D_len=np.int64(m.anchor_demon.shape[0]),
               **{"after_" + k: getattr(m, k).numpy().reshape(-1) for k in NAMES})
    compare(got, c["want"], name + " torch")


def test_ill_formed_counts_give_none():
    acc = tuple(np.zeros(n, np.float32) for n in (4, 4, 8, 8))
    vis = np.array([1, 1, 1, 0], bool)
    sel = np.array([1, 0, 1, 1], bool)
    ok = dict(opacity=np.ones(4, np.float32), selection=sel, update_filter=np.ones(3, bool), grad=np.ones((3, 3), np.float32), K=2)
    assert dr.stats(acc, np.array([1, 1, 0, 0], bool), **ok) is not None
    assert dr.stats(acc, vis, **ok) is None                                       # one more visible anchor than opacity has rows
    assert dr.stats(acc, np.array([1, 1, 0, 0], bool), **dict(ok, update_filter=np.ones(2, bool), grad=np.ones((2, 3), np.float32))) is None


# ------------------------------------------------------------------ argument errors of gauspcc_amd.densify that need no GPU
def _args(N=4, K=2, V=2, S=3):
    z = lambda n: torch.zeros(n, 1)
    return dict(opacity_accum=z(N), anchor_demon=z(N), offset_gradient_accum=z(N * K), offset_denom=z(N * K), grad=torch.zeros(S, 3),
                opacity=torch.zeros(V * K, 1), update_filter=torch.zeros(S, dtype=torch.bool), offset_selection_mask=torch.zeros(V * K, dtype=torch.bool),
                anchor_visible_mask=torch.zeros(N, dtype=torch.bool), n_offsets=K)


@pytest.mark.parametrize("change, exc", [
    (dict(anchor_demon=torch.zeros(4, 1, dtype=torch.float64)), TypeError),
    (dict(opacity_accum=np.zeros((4, 1), np.float32)), TypeError),
    (dict(update_filter=torch.zeros(3, dtype=torch.uint8)), TypeError),
    (dict(offset_denom=torch.zeros(7, 1)), ValueError),
    (dict(opacity=torch.zeros(5, 1)), ValueError),
    (dict(grad=torch.zeros(2, 3)), ValueError),
    (dict(grad=torch.zeros(3, 1)), ValueError),
    (dict(anchor_visible_mask=torch.zeros(5, dtype=torch.bool)), ValueError),
    (dict(anchor_visible_mask=None), ValueError),                                  # V != N without a mask
    (dict(offset_gradient_accum=torch.zeros(16, 1)[::2]), ValueError),             # not contiguous
    (dict(n_offsets=0), ValueError),
    (dict(), ValueError),                                                          # well-formed, but CPU tensors: there is no CPU path
])
def test_accumulate_stats_argument_errors(change, exc):
    from gauspcc_amd import densify

    with pytest.raises(exc):
        densify.accumulate_stats(**dict(_args(), **change))


def test_other_argument_errors_and_no_cpu_path():
    from gauspcc_amd import densify

    with pytest.raises(ValueError):
        densify.compact_rows(torch.ones(3, dtype=torch.bool), torch.zeros(3, 2))        # CPU tensors
    with pytest.raises(TypeError):
        densify.compact_rows(torch.ones(3), torch.zeros(3, 2))
    with pytest.raises(ValueError):
        densify.compact_rows(torch.ones(3, dtype=torch.bool), *[torch.zeros(3, 1)] * 33)
    m = types.SimpleNamespace(n_offsets=2, opacity_accum=torch.zeros(4, 1), anchor_demon=torch.zeros(4, 1), offset_gradient_accum=torch.zeros(8, 1),
                              offset_denom=torch.zeros(8, 1))
    vp = types.SimpleNamespace(grad=torch.zeros(3, 3))
    with pytest.raises(ValueError):
        densify.training_statis(m, vp, torch.zeros(4, 1), torch.zeros(3, dtype=torch.bool), torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            densify.check()
        with pytest.raises(RuntimeError):
            densify.adjust_anchor(m)
