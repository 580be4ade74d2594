"""Access to tests/golden/attr_b_<variant>.npz and ng_<variant>.npz, what the reference's own attribute-side Python computed and wrote
(tests/golden/make_attr_pins.py), for tests/test_attr_pins_cpu.py and tests/test_gpu_attr_pins.py."""
import os

import numpy as np

from . import attr_pin_cases as apc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("hac", "hac_plus")
B_IDS = [(v, c["name"]) for v in VARIANTS for c in apc.b_cases(v)]
NG_IDS = [(v, c["name"]) for v in VARIANTS for c in apc.ng_cases(v)]
_files, _cases = {}, {}


def _npz(name):
    if name not in _files:
        z = np.load(os.path.join(GOLDEN, name))
        _files[name] = {k: z[k] for k in z.files}
    return _files[name]


class BFile:
    """One file the reference wrote: name, bytes, element bounds [lo, hi), the int16 symbols and (Gaussian family) min / max and table the coder was given."""

    def __init__(self, z, prefix, name, lo, hi):
        self.name, self.lo, self.hi = name, int(lo), int(hi)
        self.blob = z[f"{prefix}/bytes"].tobytes()
        self.sym = z[f"{prefix}/sym"]
        self.min = float(z[f"{prefix}/min"]) if f"{prefix}/min" in z else None
        self.max = float(z[f"{prefix}/max"]) if f"{prefix}/max" in z else None
        self.table = z.get(f"{prefix}/table")


class BCase:
    def __init__(self, variant, name):
        z = _npz(f"attr_b_{variant}.npz")
        assert name in z["cases"].tolist()
        self.variant, self.name, self.spec = variant, name, apc.b_case(name)
        self.kind = self.spec["kind"]
        self.arrays = apc.b_inputs(self.spec)
        self.sha256 = str(z[f"{name}/inputs_sha256"])
        bounds = z[f"{name}/bounds"]
        self.bounds = [int(b) for b in bounds]
        self.files = [BFile(z, f"{name}/f{i}", str(f), bounds[i], bounds[i + 1]) for i, f in enumerate(z[f"{name}/files"].tolist())]
        self.bits = int(z[f"{name}/bits"])
        self.dec, self.dec_dtype = z[f"{name}/dec"], str(z[f"{name}/dec_dtype"])
        self.table_vs_f64 = float(z[f"{name}/table_vs_f64"])

    def part(self, f):
        """The input arrays of the elements file `f` holds (and Q as an array, the scalar expanded in float32)."""
        a = {k: v[f.lo:f.hi] for k, v in self.arrays.items()}
        if self.kind in ("gauss", "mix") and "q" not in a:
            a["q"] = np.full(f.hi - f.lo, np.float32(self.spec["q"]))
        return a

    def oracle_table(self, orc, f):
        """The table the oracle builds for file `f` from the case's inputs and the stored min / max (Bernoulli: the exact row)."""
        from . import b_assembly as ba

        a = self.part(f)
        if self.kind == "bern":
            return np.tile(ba.bernoulli_row(ba.parse_bernoulli(f.blob)[0]), (len(f.sym), 1))
        if self.kind == "gauss":
            return orc.gaussian_cdf(a["mean0"], a["scale0"], a["q"], int(f.min), int(f.max))
        if self.kind == "mix":
            comps = range(self.spec["comps"])
            return orc.gaussian_mixed_cdf([a[f"mean{c}"] for c in comps], [a[f"scale{c}"] for c in comps], [a[f"prob{c}"] for c in comps], a["q"], int(f.min), int(f.max))
        raise KeyError(self.kind)


class NGRun:
    def __init__(self, z, prefix):
        out = z[f"{prefix}/out"]
        self.out = dict(zip(apc.NG_OUTPUTS, np.split(out, [3, 6, 7, 10], axis=1)))
        self.kept = z[f"{prefix}/kept"].astype(np.int64)
        self.f32_vs_f64 = dict(zip(apc.NG_OUTPUTS, z[f"{prefix}/f32_vs_f64"].tolist()))
        self.tol = dict(zip(apc.NG_OUTPUTS, z[f"{prefix}/tol"].tolist()))
        self.separation = float(z[f"{prefix}/separation"])


class NGCase:
    def __init__(self, variant, name):
        z = _npz(f"ng_{variant}.npz")
        assert name in z["cases"].tolist()
        self.variant, self.name = variant, name
        self.spec = next(c for c in apc.NG_CASES if c["name"] == name)
        self.sha256 = str(z[f"{name}/inputs_sha256"])
        self.arrays = apc.unpack(z[f"{name}/in/f32"], z[f"{name}/in/index"])
        self.arrays["vis"] = z[f"{name}/in/vis"]
        self.runs = {tag: NGRun(z, f"{name}/{tag}") for tag in ("masked", "all") if f"{name}/{tag}/out" in z}


def b_case(variant, name) -> BCase:
    key = ("b", variant, name)
    if key not in _cases:
        _cases[key] = BCase(variant, name)
    return _cases[key]


def ng_case(variant, name) -> NGCase:
    key = ("ng", variant, name)
    if key not in _cases:
        _cases[key] = NGCase(variant, name)
    return _cases[key]
