"""Generate tests/golden/attr_b_<variant>.npz and ng_<variant>.npz (variant: hac, hac_plus) by RUNNING the reference's own attribute-side
Python from a checkout of the reference project (not part of this repository):

    python tests/golden/make_attr_pins.py <reference checkout>

Only inputs' hashes, inputs of the neural-Gaussian models and what the reference's programs computed or wrote are stored -- no reference
source text.  Inputs come from tests/attr_pin_cases.py, which the tests share.

(a) `.b` files: src/gs_compress/HAC/utils/encodings_cuda.py (38-175, 317-492) and HAC-plus/utils/encodings_cuda.py (the same functions
and 177-317, the mixture), each imported under its own module name with a stand-in `arithmetic` module, this project's own code:

  calculate_cdf(mean, scale, Q, min, max)           oracle.gaussian_cdf
  arithmetic_encode(sym, lower, chunk, n, Lp)       oracle.hac_encode, returned as CPU tensors
  arithmetic_decode(lower, data, cnt, chunk, n, Lp) oracle.hac_decode

Every call's arguments are recorded.  Each module's `torch` is a proxy that drops device='cuda' (the decoders create their tensors
there).  Per case the reference's own encoder_gaussian_chunk / decoder_gaussian_chunk, encoder / decoder, encoder_factorized_chunk /
decoder_factorized_chunk and, for HAC++, encoder_gaussian_mixed_chunk / decoder_gaussian_mixed_chunk run; stored are the files written
(names and bytes), the returned bit count, the decoded tensor with dtype and shape, per file the int16 symbols and min / max the
stand-in saw and, up to 600 symbols, the float32 table the reference's Python handed to the coder (the mixture: after its own multiply,
sum and clamp).  Asserted here: every stored table is within 2e-7 of the same expression in float64 (scipy.special.erfc; the measured
maximum is stored), and the reference's decoder returns round(x / Q) * Q exactly.

(b) Neural Gaussians: HAC/gaussian_renderer/__init__.py:25-172 and HAC-plus/gaussian_renderer/__init__.py:25-205, imported under stubs
for diff_gaussian_rasterization, scene.gaussian_model and _gridencoder and a torch proxy whose cuda.synchronize does nothing.  The
reference's own generate_neural_gaussians(cam, pc, visible_mask) runs on CPU models (attr_pin_cases.ng_model) once in float64 -- the
expectation -- and once in float32, which measures the reference's own rounding.  Stored: the model tensors and weights (float32),
the float64 outputs cast to float32, the kept candidate indices in order, per output f32_vs_f64 and the tolerance in force,
max(project tolerance, 4 x f32_vs_f64).  Asserted: the inputs are unambiguous in what the reference computed (|opacity| >= 1e-3 for
every candidate the mask leaves; |frac(x / Q) - 0.5| >= max(1e-3, 10 x the reference's float32-vs-float64 difference in x / Q)), both
runs keep the same candidates, the kept Gaussians lie at least 100 x the xyz tolerance apart (so a position names its candidate),
and each mutation of attr_pin_cases.NG_MUTATIONS, run through the reference, moves some float64 output
by at least 100 x that output's tolerance.

LIMIT.  The CUDA `arithmetic` extension's own erfc and coder and torch's GEMM rounding are not pinned: the stand-ins are this
project's oracle.  What these fixtures pin is the reference's Python around the native calls.
"""
import importlib.util
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_wiring import _module, _TorchProxy, save_npz      # noqa: E402
from tests import attr_pin_cases as apc                      # noqa: E402

MAX_FIXTURE_BYTES = 200 * 1024


class _CpuTorch(_TorchProxy):
    """torch with device='cuda' dropped from the factory calls the reference's decoders and renderer make, and a cuda.synchronize that returns."""

    cuda = types.SimpleNamespace(synchronize=lambda *a, **kw: None)

    @staticmethod
    def zeros(*a, **kw):
        kw.pop("device", None)
        return torch.zeros(*a, **kw)

    @staticmethod
    def ones(*a, **kw):
        if kw.get("device") == "cuda":
            kw.pop("device")
        return torch.ones(*a, **kw)


class Recorder:
    def reset(self):
        self.cdf, self.enc, self.dec = [], [], []


REC = Recorder()


def _arithmetic_module():
    from oracle import oracle as orc

    orc.build()
    np32 = lambda t: t.detach().cpu().numpy()

    def calculate_cdf(mean, scale, Q, min_value, max_value):
        assert mean.dtype == scale.dtype == torch.float32 and mean.shape == scale.shape == Q.shape and mean.dim() == 1
        mn, mx = float(min_value), float(max_value)
        assert mn == int(mn) and mx == int(mx)
        REC.cdf.append(dict(min=mn, max=mx, q_dtype=str(Q.dtype), min_dtype=str(min_value.dtype)))
        return torch.from_numpy(orc.gaussian_cdf(np32(mean), np32(scale), np32(Q), int(mn), int(mx)))

    def arithmetic_encode(sym, lower, chunk, n, Lp):
        assert sym.dtype == torch.int16 and sym.dim() == 1 and lower.dtype == torch.float32 and tuple(lower.shape) == (n, Lp) and sym.shape[0] == n
        assert chunk == apc.CHUNK
        REC.enc.append(dict(sym=np32(sym).copy(), table=np32(lower).copy()))
        data, cnt = orc.hac_encode(np32(sym), np32(lower), chunk)
        return torch.from_numpy(data.copy()), torch.from_numpy(cnt.copy())

    def arithmetic_decode(lower, data, cnt, chunk, n, Lp):
        assert lower.dtype == torch.float32 and tuple(lower.shape) == (n, Lp) and data.dtype == torch.uint8 and cnt.dtype == torch.int32
        REC.dec.append(dict(table=np32(lower).copy()))
        return torch.from_numpy(orc.hac_decode(np32(lower), np32(data), np32(cnt), chunk))

    return _module("arithmetic", calculate_cdf=calculate_cdf, arithmetic_encode=arithmetic_encode, arithmetic_decode=arithmetic_decode)


def _import_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_encodings(ref, variant):
    _arithmetic_module()
    sub = "HAC" if variant == "hac" else "HAC-plus"
    mod = _import_file(f"ref_{variant}_encodings_cuda", os.path.join(ref, "src/gs_compress", sub, "utils/encodings_cuda.py"))
    mod.torch = _CpuTorch()
    assert mod.chunk_size_cuda == apc.CHUNK
    return mod


def import_renderer(ref, variant):
    sub = os.path.join(ref, "src/gs_compress", "HAC" if variant == "hac" else "HAC-plus")
    for name in [m for m in sys.modules if m == "utils" or m.startswith("utils.") or m == "scene" or m.startswith("scene.")]:
        del sys.modules[name]
    _module("diff_gaussian_rasterization", GaussianRasterizationSettings=object, GaussianRasterizer=object)
    _module("scene", gaussian_model=_module("scene.gaussian_model", GaussianModel=object))
    _module("_gridencoder")
    sys.path.insert(0, sub)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mod = _import_file(f"ref_{variant}_renderer", os.path.join(sub, "gaussian_renderer/__init__.py"))
    finally:
        sys.path.remove(sub)
    mod.torch = _CpuTorch()
    return mod


# ------------------------------------------------------------------------------------------------------------ (a) `.b` files
def _table_f64(case, arrays, lo, hi, mn, mx):
    """The table of elements [lo, hi) in float64: 0.5 erfc(-((min + t - 0.5) Q - mean) / (max(scale, 1e-9) sqrt 2)); the mixture: the weighted sum, clamped."""
    from scipy.special import erfc

    n = hi - lo
    q = (arrays["q"][lo:hi] if "q" in arrays else np.full(n, np.float32(case["q"]))).astype(np.float64)
    samples = (np.arange(int(mn), int(mx) + 2, dtype=np.float64) - 0.5)[None, :] * q[:, None]
    acc = np.zeros_like(samples)
    for c in range(case.get("comps", 1)):
        mean, scale = arrays[f"mean{c}"][lo:hi].astype(np.float64), np.maximum(arrays[f"scale{c}"][lo:hi].astype(np.float64), 1e-9)
        w = arrays[f"prob{c}"][lo:hi].astype(np.float64)[:, None] if case["kind"] == "mix" else 1.0
        acc += w * 0.5 * erfc(-(samples - mean[:, None]) / (scale[:, None] * np.sqrt(2.0)))
    return np.clip(acc, 0.0, 1.0) if case["kind"] == "mix" else acc


def _fact_table_f64(case, rows, mn, mx):
    a, b, q = np.array(apc.FACT_A)[:, None], np.array(apc.FACT_B)[:, None], float(case["q"])
    s = np.arange(int(mn), int(mx) + 1, dtype=np.float64)[None, :]
    lower, upper = a * ((s - 0.5) * q) + b, a * ((s + 0.5) * q) + b
    sign = -np.sign(lower + upper)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    cdf = np.cumsum(np.abs(sig(sign * upper) - sig(sign * lower)), axis=1)
    t = np.clip(np.concatenate([np.zeros((len(a), 1)), cdf], 1), 0.0, 1.0)
    return np.tile(t, (rows, 1))


def run_b_case(mod, case, tmp):
    arrays = apc.b_inputs(case)
    kind, name = case["kind"], case["name"]
    fn = os.path.join(tmp, f"{name}.b")
    kw = dict(chunk_size=case["chunk_size"]) if case.get("chunk_size") else {}
    REC.reset()
    out = {f"{name}/inputs_sha256": np.array(apc.sha256_of(arrays))}
    if kind == "bern":
        x = torch.tensor(arrays["x"])
        bits = mod.encoder(x, file_name=fn)
        dec = mod.decoder(x.numel(), file_name=fn)
        assert np.array_equal(dec.numpy(), arrays["x"].reshape(-1).astype(np.int16))
        want = None
    elif kind == "fact":
        x = torch.tensor(arrays["x"])
        bits = mod.encoder_factorized_chunk(x, apc.lower_func, case["q"], file_name=fn, **kw)
        dec = mod.decoder_factorized_chunk(apc.lower_func, case["q"], x.shape[0], x.shape[1], file_name=fn, device="cpu", **kw)
        want = torch.round(x / case["q"]) * case["q"]
    elif kind == "gauss":
        x, mean, scale, Q = apc.b_torch_args(case, arrays, torch)
        bits = mod.encoder_gaussian_chunk(x, mean, scale, Q, file_name=fn, **kw)
        dec = mod.decoder_gaussian_chunk(mean, scale, Q, file_name=fn, **kw)
        want = torch.round(x / Q) * Q
    else:
        x, means, scales, probs, Q = apc.b_torch_args(case, arrays, torch)
        bits = mod.encoder_gaussian_mixed_chunk(x, means, scales, probs, Q, file_name=fn, **kw)
        dec = mod.decoder_gaussian_mixed_chunk(means, scales, probs, Q, file_name=fn, **kw)
        want = torch.round(x / Q) * Q
    if want is not None:
        assert dec.dtype == want.dtype and torch.equal(dec, want), f"{name}: the reference's decoder does not return round(x / Q) * Q"
    files = sorted((f for f in os.listdir(tmp) if f.startswith(name + "_") or f == name + ".b"), key=lambda f: (len(f), f))
    assert len(files) == len(REC.enc) == len(REC.dec)
    assert all(np.array_equal(e["table"], d["table"]) for e, d in zip(REC.enc, REC.dec)), f"{name}: the decoder's table is not the encoder's"
    if kind in ("gauss", "mix"):
        comps = case.get("comps", 1)
        assert len(REC.cdf) == 2 * comps * len(files)
        out[f"{name}/q_dtype"] = np.array(REC.cdf[0]["q_dtype"])
    bounds = [0, arrays["x"].size] if kind == "bern" else apc.b_chunk_bounds(case, arrays["x"].shape[0])
    assert len(bounds) == len(files) + 1
    out[f"{name}/files"] = np.array(files)
    out[f"{name}/bounds"] = np.array(bounds, np.int64)
    out[f"{name}/bits"] = np.int64(bits)
    out[f"{name}/dec"] = dec.numpy()
    out[f"{name}/dec_dtype"] = np.array(str(dec.dtype))
    worst = 0.0
    total = 0
    for i, f in enumerate(files):
        with open(os.path.join(tmp, f), "rb") as fh:
            blob = fh.read()
        total += len(blob)
        sym, table = REC.enc[i]["sym"], REC.enc[i]["table"]
        out[f"{name}/f{i}/bytes"] = np.frombuffer(blob, np.uint8)
        out[f"{name}/f{i}/sym"] = sym
        lo, hi = bounds[i], bounds[i + 1]
        if kind == "bern":
            p1 = np.frombuffer(blob[:4], np.float32)[0]
            assert np.array_equal(table, np.tile(np.array([0.0, np.float32(1) - p1, 1.0], np.float32), (len(sym), 1)))
            continue
        mn, mx = (float(v) for v in np.frombuffer(blob[:8], np.float32))
        if kind != "fact":
            per = case.get("comps", 1)
            assert all(c["min"] == mn and c["max"] == mx for c in REC.cdf[i * per:(i + 1) * per])
        out[f"{name}/f{i}/min"], out[f"{name}/f{i}/max"] = np.float32(mn), np.float32(mx)
        assert table.shape[1] == int(mx - mn) + 2
        if len(sym) <= apc.TABLE_ROWS_MAX:
            f64 = _fact_table_f64(case, hi - lo, mn, mx) if kind == "fact" else _table_f64(case, arrays, lo, hi, mn, mx)
            worst = max(worst, float(np.abs(table.astype(np.float64) - f64).max()))
            out[f"{name}/f{i}/table"] = table
    assert worst <= apc.TABLE_TOL, f"{name}: the table differs from float64 by {worst:.3g}"
    out[f"{name}/table_vs_f64"] = np.float64(worst)
    print(f"  {name:<14} {len(files)} file(s), {total} B, {int(bits)} bits, decoded {tuple(dec.shape)} {dec.dtype}, table vs float64 {worst:.2e}")
    return out


def make_b(ref, variant, tmp):
    mod = import_encodings(ref, variant)
    out = {"cases": np.array([c["name"] for c in apc.b_cases(variant)])}
    print(f"attr_b_{variant}:")
    for case in apc.b_cases(variant):
        sub = os.path.join(tmp, f"{variant}_{case['name']}")
        os.mkdir(sub)
        out.update(run_b_case(mod, case, sub))
    return _save(f"attr_b_{variant}.npz", out)


# ------------------------------------------------------------------------------------------------------------ (b) neural Gaussians
class _Tap(torch.nn.Module):
    """Records what a module of the model returned to the reference."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, x):
        y = self.inner(x)
        self.seen.append(y.detach().clone())
        return y


def run_ng(mod, case, arrays, dtype, masked=True):
    """The reference's generate_neural_gaussians -> (outputs {name: float64 numpy}, kept candidate indices, opacity MLP output, context MLP output)."""
    pc, cam, vis = apc.ng_model(case, arrays, torch, "cpu", dtype)
    pc.get_opacity_mlp = _Tap(pc.get_opacity_mlp)
    if not case["decoded"]:
        pc.get_grid_mlp = _Tap(pc.get_grid_mlp)
        pc.ng_rows = vis if masked else None
    with torch.no_grad():
        res = mod.generate_neural_gaussians(cam, pc, vis if masked else None)
    assert len(res) == 6
    outs = {k: v.double().numpy() for k, v in zip(apc.NG_OUTPUTS, res[:5])}
    nopa = pc.get_opacity_mlp.seen[0].double().numpy()                         # (visible anchors, K)
    m = arrays["mask"][arrays["vis"] if masked else slice(None)][:, :, 0]
    kept = np.nonzero((nopa.reshape(-1) > 0) & (m.reshape(-1) != 0))[0]
    assert len(kept) == len(outs["xyz"]), (case["name"], len(kept), len(outs["xyz"]))
    grid = None if case["decoded"] else pc.get_grid_mlp.seen[0].double().numpy()
    return outs, kept, nopa, grid, res[5]


def _ng_moves(a, kept_a, b, kept_b):
    if not np.array_equal(kept_a, kept_b):
        return {k: np.inf for k in apc.NG_OUTPUTS}
    return {k: float(np.abs(a[k] - b[k]).max()) for k in apc.NG_OUTPUTS}


def run_ng_case(mod, case):
    name = case["name"]
    arrays = apc.ng_inputs(case)
    out = {f"{name}/inputs_sha256": np.array(apc.sha256_of(arrays))}
    out[f"{name}/in/f32"], out[f"{name}/in/index"] = apc.pack(arrays)
    out[f"{name}/in/vis"] = arrays["vis"]
    runs = [("masked", True)] + ([("all", False)] if case.get("also_without_mask") else [])
    for tag, masked in runs:
        o64, kept, nopa64, grid64, tsub = run_ng(mod, case, arrays, torch.float64, masked)
        o32, kept32, _, grid32, _ = run_ng(mod, case, arrays, torch.float32, masked)
        assert (tsub == 0) == bool(case["decoded"])
        m = arrays["mask"][arrays["vis"] if masked else slice(None)][:, :, 0]
        margin = float(np.abs(nopa64[m != 0]).min())
        assert margin >= apc.OPACITY_MARGIN, f"{name}: a candidate with |opacity| {margin:.2e}"
        assert np.array_equal(kept, kept32) and len(kept) > 0
        if not case["decoded"]:
            rows = arrays["vis"] if masked else slice(None)
            worst_frac, worst_diff = 1.0, 0.0
            for j, (q0, key) in enumerate(((apc.Q_FEAT, "feat"), (apc.Q_SCALING, "scaling"), (apc.Q_OFFSETS, "offset"))):
                x = arrays[key][rows].reshape(len(grid64), -1)
                r64 = x.astype(np.float64) / (q0 * (1.0 + np.tanh(grid64[:, -3 + j:grid64.shape[1] - 2 + j])))
                q32 = (np.float32(q0) * (np.float32(1) + np.tanh(grid32[:, -3 + j:grid32.shape[1] - 2 + j].astype(np.float32)))).astype(np.float32)
                r32 = (x / q32).astype(np.float64)
                diff = float(np.abs(r32 - r64).max())
                frac = float(np.abs(np.abs(r64 - np.floor(r64) - 0.5)).min())
                need = max(apc.FRAC_MARGIN, 10 * diff)
                assert frac >= need, f"{name}: {key} comes within {frac:.2e} of a rounding boundary (needs {need:.2e})"
                worst_frac, worst_diff = min(worst_frac, frac), max(worst_diff, diff)
            out[f"{name}/{tag}/round_margin"] = np.float64(worst_frac)
            out[f"{name}/{tag}/xq_f32_vs_f64"] = np.float64(worst_diff)
        diffs = _ng_moves(o64, kept, o32, kept32)
        tol = {k: max(apc.NG_TOL[k], 4 * diffs[k]) for k in apc.NG_OUTPUTS}
        out[f"{name}/{tag}/out"] = np.concatenate([o64[k] for k in apc.NG_OUTPUTS], axis=1).astype(np.float32)      # (kept, 3 + 3 + 1 + 3 + 4)
        out[f"{name}/{tag}/kept"] = kept.astype(np.int32)
        sep = float((np.linalg.norm(o64["xyz"][:, None] - o64["xyz"][None], axis=-1) + 1e9 * np.eye(len(kept))).min())
        assert sep >= apc.SEPARATION * tol["xyz"], f"{name}: two kept Gaussians {sep:.2e} apart"
        out[f"{name}/{tag}/separation"] = np.float64(sep)
        out[f"{name}/{tag}/f32_vs_f64"] = np.array([diffs[k] for k in apc.NG_OUTPUTS])
        out[f"{name}/{tag}/tol"] = np.array([tol[k] for k in apc.NG_OUTPUTS])
        out[f"{name}/{tag}/opacity_margin"] = np.float64(margin)
        print(f"  {name:<30} {tag:<6} {len(kept)} of {nopa64.size} candidates kept, min |opacity| {margin:.2e}, nearest two {sep:.2e} apart")
        print("    reference float32 vs float64: " + " ".join(f"{k} {diffs[k]:.2e}" for k in apc.NG_OUTPUTS))
        print("    tolerance in force:           " + " ".join(f"{k} {tol[k]:.2e}" for k in apc.NG_OUTPUTS))
        if tag != "masked":
            continue
        for mname in apc.NG_MUTATIONS:
            if mname == "exchange_bank_first_last" and not case["bank"]:
                continue
            m64, mkept, _, _, _ = run_ng(mod, case, apc.ng_mutate(case, arrays, mname, int(kept[0]) % case["K"]), torch.float64, True)
            mv = _ng_moves(o64, kept, m64, mkept)
            ratio = max(mv[k] / tol[k] for k in apc.NG_OUTPUTS)
            assert ratio >= 100, f"{name}: mutation {mname} moves the outputs by only {ratio:.1f} x the tolerance"
            out[f"{name}/mutation_{mname}"] = np.array([min(mv[k], 1e30) for k in apc.NG_OUTPUTS])
            print(f"    mutation {mname}: " + ("another set of Gaussians" if np.isinf(ratio) else " ".join(f"{k} {mv[k]:.2e}" for k in apc.NG_OUTPUTS)))
    return out


def make_ng(ref, variant):
    mod = import_renderer(ref, variant)
    out = {"cases": np.array([c["name"] for c in apc.ng_cases(variant)])}
    print(f"ng_{variant}:")
    for case in apc.ng_cases(variant):
        out.update(run_ng_case(mod, case))
    return _save(f"ng_{variant}.npz", out)


def _save(name, arrays):
    path = os.path.join(HERE, name)
    save_npz(path, arrays)
    size = os.path.getsize(path)
    assert size <= MAX_FIXTURE_BYTES, f"{name}: {size} bytes"
    print(f"{name}: {size} bytes")
    return path


def main(ref):
    torch.manual_seed(0)
    torch.set_num_threads(1)          # one summation order, whatever the machine
    with tempfile.TemporaryDirectory() as tmp:
        for variant in ("hac", "hac_plus"):
            make_b(ref, variant, tmp)
    for variant in ("hac", "hac_plus"):
        make_ng(ref, variant)
    print("attribute pins written to", HERE)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
