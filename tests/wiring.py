"""Access to tests/golden/wiring_<case>.npz, the fixtures the reference's own GausPcgc Python computed (tests/golden/make_wiring.py):
the cases, their weights (checked against the stored sha256), per-level records, tolerances and the generator's mutations."""
import importlib.util
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_wiring", os.path.join(GOLDEN, "make_wiring.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)      # the generator's own weights(), mutate() and case table; it touches the reference only in main()

CASES = tuple(c["name"] for c in gen.CASES)
GRAD_CASE = next(c["name"] for c in gen.CASES if c["grad"])
MUTATIONS = gen.MUTATIONS
PROB_TOL = 1e-5
_cache = {}


class Case:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, f"wiring_{name}.npz"))
        self.name, self.z = name, {k: z[k] for k in z.files}
        self.k, self.posQ, self.points = int(self.z["k"]), float(self.z["posQ"]), self.z["points"]
        self.levels = int(self.z["levels"])
        spec = next(c for c in gen.CASES if c["name"] == name)
        assert float(self.z["emb_scale"]) == gen.EMB_SCALE and int(self.z["weight_seed"]) == spec["wseed"]
        self.sd = gen.weights(self.k, spec["wseed"])
        # a change in synth.py must not silently detach the fixture from the weights the tests load
        assert gen.weights_sha256(self.sd) == str(self.z["weights_sha256"]), "synthetic weights no longer those of the fixture: regenerate"
        self.bits_f64 = float(self.z["bpp_f64"]) * len(self.points)

    def xyz(self, d):
        return self.z[f"l{d}_xyz"]

    def sym(self, d, s):
        return self.z[f"l{d}_s{s}_sym"]

    def cdf(self, d, s):
        return self.z[f"l{d}_s{s}_cdf"]

    def prob(self, d, s):
        return self.z[f"l{d}_s{s}_prob"].astype(np.float64)

    def tol(self, s):
        """max(1e-5, 4 x the reference's own float32-vs-float64 difference on this stage's probabilities)."""
        return max(PROB_TOL, 4.0 * float(self.z["f32_vs_f64"][s]))

    def grad(self):
        z = np.load(os.path.join(GOLDEN, f"wiring_{self.name}_grad.npz"))
        assert str(z["weights_sha256"]) == str(self.z["weights_sha256"])
        return {k: z[k] for k in z.files}


def case(name) -> Case:
    if name not in _cache:
        _cache[name] = Case(name)
    return _cache[name]


def sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort((a[:, 0], a[:, 1], a[:, 2]))]
