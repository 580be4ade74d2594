"""Generate tests/golden/densify.npz by RUNNING the reference's own `GaussianModel.training_statis` and `GaussianModel.adjust_anchor` from a
checkout of the reference project (not part of this repository):

    python tests/golden/make_densify_golden.py <reference checkout>

The four `scene/gaussian_model.py` (HAC, HAC-plus, TC-GS, CAT-3DGS) are imported under stub modules for everything they import besides
torch and numpy, and with a torch proxy that drops device='cuda'.  Their methods run unbound on a plain namespace that holds n_offsets,
the four accumulators, get_anchor and two recorder stand-ins: `anchor_growing` records its arguments and appends the case's number of zero
rows to opacity_accum / anchor_demon / get_anchor, `prune_anchor` records the mask.  Every case (tests/densify_ref.py: CASES, make_case) is
its iterations of training_statis followed by one adjust_anchor, run in float64 -- the expectation -- and in float32 -- the reference's own
rounding.  Asserted here: the four frameworks give identical results in both precisions (TC-GS's anchor_visible_mask=None equal to an
all-set mask), the input conditions of densify_ref.margins_ok hold, float32 and float64 make the same decisions, and the file stays under
200 KB.  Stored: only the inputs, what the reference computed (float64) and the measured float32-vs-float64 differences -- no reference
source text.
"""
import importlib.abc
import importlib.machinery
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_wiring import _TorchProxy, save_npz      # noqa: E402
from tests import densify_ref as dr                # noqa: E402

MAX_FIXTURE_BYTES = 200 * 1024
FRAMEWORKS = ("HAC", "HAC-plus", "TC-GS", "CAT-3DGS")
STUB_ROOTS = ("utils", "scene", "plyfile", "simple_knn", "torch_scatter", "sklearn", "PIL", "torchvision", "diff_gaussian_rasterization", "_gridencoder",
              "gridencoder", "torchac", "arithmetic", "einops", "tinycudann", "lpips")


class _KeepDtype(torch.Tensor):
    """zeros whose .float() keeps the run's dtype: the reference writes `torch.zeros(..., device='cuda').float()` into its accumulators, which
    index_put accepts only in the accumulators' own dtype"""

    def float(self):
        return self.as_subclass(torch.Tensor)


class _CpuTorch(_TorchProxy):
    run_dtype = torch.float32   # set per run (run_case)

    @staticmethod
    def zeros(*a, **kw):
        if kw.get("device") == "cuda":
            kw.pop("device")
        t = torch.zeros(*a, **kw)
        return t.to(_CpuTorch.run_dtype).as_subclass(_KeepDtype) if t.dtype == torch.float32 and _CpuTorch.run_dtype != torch.float32 else t

    @staticmethod
    def ones(*a, **kw):
        if kw.get("device") == "cuda":
            kw.pop("device")
        return torch.ones(*a, **kw)


class _Stub(types.ModuleType):
    """A module whose every public attribute is an empty class: enough for the import statements and base classes of a file whose two
    methods under test use none of them."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (), {"__init__": lambda self, *a, **kw: None})
        setattr(self, name, cls)
        return cls


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in STUB_ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def import_model(ref, framework):
    for name in [m for m in sys.modules if m.split(".")[0] in STUB_ROOTS]:
        del sys.modules[name]
    path = os.path.join(ref, "src/gs_compress", framework, "scene/gaussian_model.py")
    finder = _StubFinder()
    sys.meta_path.insert(0, finder)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = importlib.util.spec_from_file_location("ref_densify_" + framework.replace("-", "_").lower(), path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
    finally:
        sys.meta_path.remove(finder)
    mod.torch = _CpuTorch()
    return mod.GaussianModel


def run_case(GM, case, dtype, none_visible_mask=False):
    """The reference's methods on a namespace -> dict of numpy results"""
    N, K, appended, ci = case["N"], case["K"], case["appended"], case["check_interval"]
    rec = {}

    def anchor_growing(grads, threshold, offset_mask):
        rec.update(grads_norm=grads.clone(), threshold=threshold, offset_mask=offset_mask.clone())
        for name in ("opacity_accum", "anchor_demon"):
            setattr(m, name, torch.cat([getattr(m, name), torch.zeros([appended, 1]).float()], dim=0))   # float32 zeros, as the reference appends
        m.get_anchor = torch.zeros(N + appended, 3)

    def prune_anchor(mask):
        rec.update(prune_mask=mask.clone())
        m.get_anchor = m.get_anchor[~mask]

    _CpuTorch.run_dtype = dtype
    m = dr.model(N, K, dtype, lib="torch")
    m.get_anchor = torch.zeros(N, 3)
    m.anchor_growing, m.prune_anchor = anchor_growing, prune_anchor
    for it in case["iters"]:
        vp = types.SimpleNamespace(grad=torch.from_numpy(it["grad"]).to(dtype))
        vis = None if none_visible_mask else torch.from_numpy(it["visible"])
        GM.training_statis(m, vp, torch.from_numpy(it["opacity"]).to(dtype).view(-1, 1), torch.from_numpy(it["update_filter"]),
                           torch.from_numpy(it["selection"]), vis)
    np64 = lambda t: t.detach().numpy().astype(np.float64).reshape(-1)
    res = {"stats_" + k: np64(getattr(m, k)) for k in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")}
    GM.adjust_anchor(m, check_interval=ci, success_threshold=dr.SUCCESS_THRESHOLD, grad_threshold=dr.GRAD_THRESHOLD, min_opacity=dr.MIN_OPACITY)
    assert rec["threshold"] == dr.GRAD_THRESHOLD
    res.update({"after_" + k: np64(getattr(m, k)) for k in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")})
    res.update(grads_norm=np64(rec["grads_norm"]), offset_mask=rec["offset_mask"].numpy().copy(),
               prune_mask=rec["prune_mask"].numpy().copy() if "prune_mask" in rec else np.zeros(0, bool), max_radii2D_len=np.int64(m.max_radii2D.shape[0]))
    return res


MASKS = ("offset_mask", "prune_mask", "max_radii2D_len", "stats_anchor_demon", "stats_offset_denom", "after_anchor_demon", "after_offset_denom")
SUMS = ("stats_opacity_accum", "stats_offset_gradient_accum", "grads_norm", "after_opacity_accum", "after_offset_gradient_accum")


def main(ref):
    models = {f: import_model(ref, f) for f in FRAMEWORKS}
    arrays = {}
    for name in dr.CASES:
        for attempt in range(50):
            case = dr.make_case(name, attempt)
            r64 = run_case(models["HAC"], case, torch.float64)
            if dr.margins_ok(r64["stats_opacity_accum"], r64["stats_anchor_demon"], r64["grads_norm"], dr.MIN_OPACITY, dr.GRAD_THRESHOLD):
                break
        else:
            raise AssertionError(f"{name}: no seed meets the input conditions")
        r32 = run_case(models["HAC"], case, torch.float32)
        for f in FRAMEWORKS[1:]:
            for dt, want in ((torch.float64, r64), (torch.float32, r32)):
                got = run_case(models[f], case, dt)
                assert all(np.array_equal(got[k], want[k], equal_nan=True) for k in want), (name, f, dt)
        if _all_visible(case):
            got = run_case(models["TC-GS"], case, torch.float64, none_visible_mask=True)
            assert all(np.array_equal(got[k], r64[k]) for k in r64), (name, "TC-GS, anchor_visible_mask=None")
        for k in MASKS:   # the counts sit on their thresholds only as integers: both precisions decide alike
            assert np.array_equal(r32[k], r64[k]), (name, k)
        pre = name + "/"
        arrays.update({pre + "attempt": np.int64(attempt), pre + "N": np.int64(case["N"]), pre + "K": np.int64(case["K"]),
                       pre + "appended": np.int64(case["appended"]), pre + "check_interval": np.int64(case["check_interval"])})
        for i, it in enumerate(case["iters"]):
            arrays.update({f"{pre}it{i}/{k}": v for k, v in it.items()})
        for k in MASKS:
            arrays[pre + k] = r64[k].astype(np.uint16) if r64[k].dtype == np.float64 else r64[k]
        for k in SUMS:
            arrays[pre + k] = r64[k]
            arrays[pre + k + "/f32_vs_f64"] = np.float64(np.max(np.abs(r32[k] - r64[k]), initial=0.0))
        n_prune, n_off = int(r64["prune_mask"].sum()), int(r64["offset_mask"].sum())
        print(f"{name}: attempt {attempt}, pruned {n_prune} of {len(r64['prune_mask'])}, offsets passing {n_off} of {len(r64['offset_mask'])}, " +
              ", ".join(f"{k} {arrays[pre + k + '/f32_vs_f64']:.2e}" for k in SUMS))
    arrays["min_opacity"], arrays["grad_threshold"], arrays["success_threshold"] = np.float64(dr.MIN_OPACITY), np.float64(dr.GRAD_THRESHOLD), np.float64(dr.SUCCESS_THRESHOLD)
    out = os.path.join(HERE, "densify.npz")
    save_npz(out, arrays)
    size = os.path.getsize(out)
    assert size <= MAX_FIXTURE_BYTES, size
    print(f"wrote {out}: {size} bytes")


def _all_visible(case):
    return all(it["visible"].all() for it in case["iters"])


if __name__ == "__main__":
    main(sys.argv[1])
