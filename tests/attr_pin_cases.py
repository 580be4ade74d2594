"""Inputs of the attribute-side pins, shared by the generator (tests/golden/make_attr_pins.py, which feeds them to the reference's own
Python) and the tests (tests/test_attr_pins_cpu.py, tests/test_gpu_attr_pins.py): the case tables and the seeded numpy.random.RandomState
builders.  Every fixture stores inputs_sha256 of what its builder returned, so drift in a builder is caught.

`.b` cases (B_CASES).  Every x is k * q with an integer k: q is a float32 of few mantissa bits (QS) or the scalar the case names, so
round(x / q) == k in float32 whichever way the last bit of the division falls.  Scales are wide enough against |sample| that the float32
table stays within the project's 2e-7 of the float64 expression (the generator asserts it).

Neural-Gaussian cases (NG_CASES).  Inputs are UNAMBIGUOUS in float64: every candidate the offset mask leaves has |neural opacity| >= 1e-3
(anchors that violate it are redrawn), and for un-decoded models every attribute is (integer + u) * Q with |u| <= 0.4 and Q the step the
context MLP gives in float64, so round(x / Q) has a margin of 0.1 against everybody's rounding; the kept Gaussians lie 100 tolerances apart.  The generator asserts both on what the
reference itself computed; the forward pass below only steers the redraw.  Weights are multiples of 1/16 in [-0.5, 0.5] (the context MLP's
second layer: of 1/128), which is what lets a fixture hold them in full.
"""
import hashlib
import types

import numpy as np

CHUNK = 10000                                         # chunk_size_cuda of both reference files and of gauspcc_amd.encodings_cuda
QS = np.array([0.5, 1.0, 2.0, 0.75, 1.25], np.float32)
TABLE_ROWS_MAX = 600                                  # the float32 table the reference handed to the coder is stored up to this many symbols
TABLE_TOL = 2e-7                                      # tests/test_gpu_attributes.py::test_calculate_cdf_matches_oracle: two erfc libraries

# kind 'gauss': encoder_gaussian_chunk;  'mix': encoder_gaussian_mixed_chunk (HAC++ file only);  'bern': encoder;  'fact': encoder_factorized_chunk.
# levels: inclusive range of round(x / Q), both ends present when n >= 2.  q: 'tensor' (per element from QS) or the Python scalar handed over.
# scale: (low, high) factors of Q;  scale_abs: absolute values instead.  chunk_size: the wrappers' argument (None: their default).
# only: the one fixture that holds the case (the large ones run through one of the two reference files: both fixtures stay under 200 KB).
B_CASES = (
    dict(name="g_n1", kind="gauss", n=1, seed=11, levels=(2, 2), q="tensor", scale=(0.6, 2.0)),
    dict(name="g_10000", kind="gauss", only="hac", n=10000, seed=12, levels=(-3, 4), q=1.0, scale=(0.7, 2.5)),
    dict(name="g_10001", kind="gauss", only="hac", n=10001, seed=13, levels=(-3, 4), q=0.5, scale=(0.7, 2.5)),
    dict(name="g_chunk23", kind="gauss", n=23, seed=14, levels=(-4, 6), q="tensor", scale=(0.6, 2.0), chunk_size=10),
    dict(name="g_scalar_q", kind="gauss", n=57, seed=15, levels=(-5, 5), q=0.75, scale=(0.6, 2.0)),
    dict(name="g_tensor_q", kind="gauss", n=57, seed=16, levels=(-5, 5), q="tensor", scale=(0.6, 2.0)),
    dict(name="g_const", kind="gauss", n=40, seed=17, levels=(3, 3), q="tensor", scale=(0.6, 2.0)),
    dict(name="g_negative", kind="gauss", n=45, seed=18, levels=(-9, -2), q="tensor", scale=(0.6, 2.0)),
    dict(name="g_wide", kind="gauss", only="hac", n=64, seed=19, levels=(-150, 150), q=0.001, scale=(0.05, 0.2), scale_abs=True),
    dict(name="g_clamp", kind="gauss", n=30, seed=20, levels=(-3, 3), q="tensor", scale=(0.6, 2.0), clamp_rows=(0, 7, 8, 29)),
    dict(name="b_zeros", kind="bern", shape=(37,), seed=21, p=0.0),
    dict(name="b_ones", kind="bern", shape=(37,), seed=22, p=1.0),
    dict(name="b_n1", kind="bern", shape=(1,), seed=23, p=0.0),
    dict(name="b_mask3", kind="bern", only="hac", shape=(2345, 10, 1), seed=24, p=0.27),
    dict(name="f_chunk23", kind="fact", n=23, dim=3, seed=25, levels=(-4, 4), q=0.5, chunk_size=10),
    dict(name="m_two", kind="mix", n=200, seed=31, levels=(-5, 6), q="tensor", scale=(0.6, 2.0), comps=2),
    dict(name="m_zero_weight", kind="mix", n=90, seed=32, levels=(-4, 4), q="tensor", scale=(0.6, 2.0), comps=2, zero_weight=True),
    dict(name="m_one", kind="mix", n=90, seed=33, levels=(-4, 4), q=1.25, scale=(0.6, 2.0), comps=1),
    dict(name="m_chunk23", kind="mix", n=23, seed=34, levels=(-4, 6), q="tensor", scale=(0.6, 2.0), comps=2, chunk_size=10),
    dict(name="m_10000", kind="mix", n=10000, seed=35, levels=(-3, 4), q=1.0, scale=(0.7, 2.5), comps=2),
    dict(name="m_10001", kind="mix", n=10001, seed=36, levels=(-3, 4), q=2.0, scale=(0.7, 2.5), comps=2),
)
B_VARIANTS = {"hac": ("gauss", "bern", "fact"), "hac_plus": ("gauss", "bern", "fact", "mix")}

FACT_A = (0.6, 1.1, 1.7)
FACT_B = (-0.4, 0.2, 0.9)


def b_cases(variant):
    return tuple(c for c in B_CASES if c["kind"] in B_VARIANTS[variant] and c.get("only", variant) == variant)


def b_case(name):
    return next(c for c in B_CASES if c["name"] == name)


def lower_func(v, stop_gradient=False):
    """The factorized pair's cumulative logits: a_c * v + b_c per channel (monotone, like an entropy bottleneck's), on a [C, 1, L] tensor."""
    import torch

    a = torch.tensor(FACT_A, dtype=v.dtype, device=v.device).view(-1, 1, 1)
    b = torch.tensor(FACT_B, dtype=v.dtype, device=v.device).view(-1, 1, 1)
    return a * v + b


def _levels(rng, n, lo, hi):
    k = rng.randint(lo, hi + 1, size=n)
    if n >= 2:
        k[0], k[-1] = lo, hi
    return k


def b_inputs(case):
    """{name: numpy array} of a `.b` case.  Q is an array under 'q' (tensor Q) or absent (the scalar case['q'] is handed over as it is)."""
    rng = np.random.RandomState(case["seed"])
    kind = case["kind"]
    if kind == "bern":
        x = (rng.rand(*case["shape"]) < case["p"]).astype(np.float32)
        return dict(x=x)
    if kind == "fact":
        k = _levels(rng, case["n"] * case["dim"], *case["levels"]).reshape(case["n"], case["dim"])
        return dict(x=(k * np.float32(case["q"])).astype(np.float32))
    n = case["n"]
    k = _levels(rng, n, *case["levels"])
    out = {}
    if case["q"] == "tensor":
        q = QS[rng.randint(len(QS), size=n)]
        out["q"] = q
    else:
        q = np.full(n, np.float32(case["q"]))
    x = (k * q).astype(np.float32)
    out["x"] = x
    lo, hi = case["scale"]
    for c in range(case.get("comps", 1)):
        scale = (rng.rand(n) * (hi - lo) + lo).astype(np.float32)
        if not case.get("scale_abs"):
            scale = (scale * q).astype(np.float32)
        mean = (x + rng.randn(n) * scale * 0.7).astype(np.float32)
        for j, r in enumerate(case.get("clamp_rows", ())):
            scale[r] = (0.0, 1e-12, 5e-10, 9.9e-10)[j % 4]       # below the 1e-9 clamp; the value lies in the bin that holds the mean
            mean[r] = np.float32((k[r] + (0.2, -0.3, 0.1, 0.0)[j % 4]) * q[r])
        out[f"mean{c}"], out[f"scale{c}"] = mean, scale
    if kind == "mix":
        comps = case["comps"]
        if comps == 1:
            out["prob0"] = np.ones(n, np.float32)
        else:
            z = rng.randn(n, comps).astype(np.float32)
            w = np.exp(z - z.max(1, keepdims=True))
            w = (w / w.sum(1, keepdims=True)).astype(np.float32)
            if case.get("zero_weight"):
                w[::3] = (1.0, 0.0)
                w[1::7] = (0.0, 1.0)
            for c in range(comps):
                out[f"prob{c}"] = np.ascontiguousarray(w[:, c])
    return out


def sha256_of(arrays):
    h = hashlib.sha256()
    for key in sorted(arrays):
        a = np.ascontiguousarray(arrays[key])
        h.update(key.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def pack(arrays):
    """The float32 arrays of a dict as one flat vector and an index of 'key:d0,d1,...' strings (a fixture member per array costs more than most arrays)."""
    keys = [k for k in sorted(arrays) if arrays[k].dtype == np.float32]
    flat = np.concatenate([arrays[k].reshape(-1) for k in keys])
    return flat, np.array([f"{k}:{','.join(map(str, arrays[k].shape))}" for k in keys])


def unpack(flat, index):
    out, at = {}, 0
    for item in index:
        key, dims = str(item).split(":")
        shape = tuple(int(d) for d in dims.split(",")) if dims else ()
        size = int(np.prod(shape, dtype=np.int64))
        out[key] = flat[at:at + size].reshape(shape)
        at += size
    assert at == flat.size
    return out


def b_chunk_bounds(case, n):
    """Element bounds of the files the `_chunk` wrappers write: [0, chunk_size, 2 chunk_size, ..., n]."""
    cs = case.get("chunk_size") or 1000_0000
    return list(range(0, n, cs)) + [n]


def b_torch_args(case, arrays, torch, device="cpu"):
    """The case's inputs as the wrappers take them: (x, mean, scale, Q) / (x, [mean], [scale], [prob], Q) with Q a tensor or the scalar."""
    t = lambda a: torch.tensor(a, device=device)
    Q = t(arrays["q"]) if "q" in arrays else case["q"]
    if case["kind"] == "gauss":
        return t(arrays["x"]), t(arrays["mean0"]), t(arrays["scale0"]), Q
    comps = range(case["comps"])
    return t(arrays["x"]), [t(arrays[f"mean{c}"]) for c in comps], [t(arrays[f"scale{c}"]) for c in comps], [t(arrays[f"prob{c}"]) for c in comps], Q


# ------------------------------------------------------------------------------------------------------------ neural Gaussians
Q_FEAT, Q_SCALING, Q_OFFSETS = 1.0, 0.001, 0.2
OPACITY_MARGIN = 1e-3
FRAC_MARGIN = 1e-3
SEPARATION = 100            # kept Gaussians lie at least this many xyz tolerances apart, so a position names its candidate
CTX_DIM = 16
NG_TOL = dict(xyz=2e-5, color=2e-5, opacity=2e-5, scaling=2e-5, rot=5e-5)       # tests/test_gpu_neural_gaussians.py
NG_OUTPUTS = ("xyz", "color", "opacity", "scaling", "rot")

NG_CASES = (
    dict(name="hac_f32_k10_bank", variant="hac", F=32, K=10, bank=True, n=17, decoded=True, seed=41),
    dict(name="hac_f50_k10_undecoded", variant="hac", F=50, K=10, bank=False, n=33, decoded=False, seed=42),
    dict(name="hac_f32_k5", variant="hac", F=32, K=5, bank=False, n=15, decoded=True, seed=43, also_without_mask=True),
    dict(name="hac_f50_k17", variant="hac", F=50, K=17, bank=False, n=40, decoded=True, seed=44),              # K > 16: the one-lane-per-anchor kernel
    dict(name="hac_f32_k16_bank_undecoded", variant="hac", F=32, K=16, bank=True, n=64, decoded=False, seed=45),
    dict(name="hacpp_f50_k10", variant="hac_plus", F=50, K=10, bank=False, n=33, decoded=True, seed=46),
    # the feature bank folds feat[:, ::4] four times over (HAC/gaussian_renderer/__init__.py:126-129): feat_dim must divide by 4, so the bank
    # case of HAC++ has feat_dim 32 -- with 50 the reference's own expression cannot be evaluated
    dict(name="hacpp_f32_k10_bank_undecoded", variant="hac_plus", F=32, K=10, bank=True, n=48, decoded=False, seed=47),
)
MLPS = ("opacity", "cov", "color", "bank", "grid")


def ng_cases(variant):
    return tuple(c for c in NG_CASES if c["variant"] == variant)


def grid_width(case):
    F, K = case["F"], case["K"]
    return (3 if case["variant"] == "hac_plus" else 2) * F + 12 + 6 * K + 3


def _w(rng, shape, unit=16):
    return (rng.randint(-8, 9, size=shape) / float(unit)).astype(np.float32)


def _mlp_np(a, name, x):
    h = np.maximum(x @ a[f"{name}_w1"].astype(np.float64).T + a[f"{name}_b1"].astype(np.float64), 0.0)
    return h @ a[f"{name}_w2"].astype(np.float64).T + a[f"{name}_b2"].astype(np.float64)


def _steps_np(case, a):
    """(Q_feat, Q_scaling, Q_offsets), each (n, 1), in float64 from the context MLP's last three columns."""
    adj = _mlp_np(a, "grid", a["ctx"].astype(np.float64))[:, -3:]
    return [q0 * (1.0 + np.tanh(adj[:, j:j + 1])) for j, q0 in enumerate((Q_FEAT, Q_SCALING, Q_OFFSETS))]


def _opacity_np(case, a, feat):
    """Neural opacity (n, K) in float64 from `feat` (n, F): only steers the redraw of borderline anchors."""
    view = a["anchor"].astype(np.float64) - a["cam"].astype(np.float64)
    dist = np.linalg.norm(view, axis=1, keepdims=True)
    view = view / dist
    if case["bank"]:
        z = _mlp_np(a, "bank", np.concatenate([view, dist], 1))
        w = np.exp(z - z.max(1, keepdims=True)); w /= w.sum(1, keepdims=True)
        feat = np.tile(feat[:, ::4], (1, 4)) * w[:, :1] + np.tile(feat[:, ::2], (1, 2)) * w[:, 1:2] + feat * w[:, 2:]
    return np.tanh(_mlp_np(a, "opacity", np.concatenate([feat, view, dist], 1)))


def ng_inputs(case):
    """{name: numpy array}: the model tensors (float32), the visible mask (bool), the camera centre and the weights of the MLPs."""
    rng = np.random.RandomState(case["seed"])
    F, K, n = case["F"], case["K"], case["n"]
    a = dict(cam=np.array([0.3, -4.0, 1.1], np.float32))
    a["anchor"] = (rng.rand(n, 3) * 4 - 2).astype(np.float32)
    a["mask"] = (rng.rand(n, K, 1) > 0.35).astype(np.float32)
    vis = rng.rand(n) > 0.2
    vis[1], vis[2] = False, True
    a["vis"] = vis
    for name, cin, cout in (("opacity", F + 4, K), ("cov", F + 4, 7 * K), ("color", F + 4, 3 * K)):
        a[f"{name}_w1"], a[f"{name}_b1"], a[f"{name}_w2"], a[f"{name}_b2"] = _w(rng, (F, cin)), _w(rng, F), _w(rng, (cout, F)), _w(rng, cout)
    if case["bank"]:
        a["bank_w1"], a["bank_b1"], a["bank_w2"], a["bank_b2"] = _w(rng, (F, 4)), _w(rng, F), _w(rng, (3, F)), _w(rng, 3)
    if not case["decoded"]:
        a["ctx"] = (rng.randn(n, CTX_DIM) * 0.5).astype(np.float32)
        a["grid_w1"], a["grid_b1"] = _w(rng, (2 * F, CTX_DIM)), _w(rng, 2 * F)
        # the heads in front of the three step columns are not read at inference: three-valued rows keep the fixture small
        a["grid_w2"], a["grid_b2"] = (rng.randint(-1, 2, size=(grid_width(case), 2 * F)) / 16.0).astype(np.float32), _w(rng, grid_width(case), 128)
        a["grid_w2"][-3:] = _w(rng, (3, 2 * F), 128)
        qf, qs, qo = _steps_np(case, a)

    def draw(rows):
        m = len(rows)
        if case["decoded"]:
            return ((rng.randn(m, F) * 0.8).astype(np.float32), np.exp(rng.randn(m, 6) * 0.4 - 2.5).astype(np.float32),
                    (rng.randn(m, K, 3) * 0.3).astype(np.float32))
        part = lambda lo, hi, shape: rng.randint(lo, hi + 1, size=shape) + rng.uniform(-0.4, 0.4, size=shape)
        # an anchor's K offsets round to K different integer triples of [-3, 3]^3: no two candidates share a position after quantisation
        combo = np.stack([rng.choice(343, size=K, replace=False) for _ in range(m)])
        triples = np.stack([combo % 7 - 3, (combo // 7) % 7 - 3, combo // 49 - 3], axis=-1) + rng.uniform(-0.4, 0.4, size=(m, K, 3))
        return ((part(-3, 3, (m, F)) * qf[rows]).astype(np.float32), (part(20, 200, (m, 6)) * qs[rows]).astype(np.float32),
                (triples * qo[rows][:, None, :]).astype(np.float32))

    a["feat"], a["scaling"], a["offset"] = draw(np.arange(n))
    for _ in range(200):
        feat = a["feat"].astype(np.float64)
        if not case["decoded"]:
            feat = np.rint(feat / qf) * qf
        op = _opacity_np(case, a, feat)
        bad = np.nonzero(((np.abs(op) < 4 * OPACITY_MARGIN) & (a["mask"][:, :, 0] != 0)).any(1))[0]
        if bad.size == 0:
            break
        a["feat"][bad], a["scaling"][bad], a["offset"][bad] = draw(bad)
    else:
        raise AssertionError(f"{case['name']}: could not clear the borderline opacities")
    return a


def _sequential(torch, a, name, act, device, dtype):
    nn = torch.nn
    w1, w2 = a[f"{name}_w1"], a[f"{name}_w2"]
    mods = [nn.Linear(w1.shape[1], w1.shape[0]), nn.ReLU(True), nn.Linear(w2.shape[1], w2.shape[0])] + ([act] if act is not None else [])
    seq = nn.Sequential(*mods)
    with torch.no_grad():
        for lin, tag in ((seq[0], "1"), (seq[2], "2")):
            lin.weight.copy_(torch.tensor(a[f"{name}_w{tag}"])); lin.bias.copy_(torch.tensor(a[f"{name}_b{tag}"]))
    return seq.to(device=device, dtype=dtype).eval()


def ng_model(case, a, torch, device="cpu", dtype=None):
    """(pc, cam, visible_mask): a SimpleNamespace with the attributes generate_neural_gaussians touches, built from the arrays of ng_inputs
    (or of a fixture).  For an un-decoded model calc_interp_feat is a stand-in that returns the stored context features of the anchors it is
    given (the rows `visible_mask` selects, in order; all rows without a mask)."""
    dtype = dtype or torch.float32
    nn = torch.nn
    t = lambda x: torch.tensor(np.asarray(x)).to(device=device, dtype=dtype)
    pc = types.SimpleNamespace(feat_dim=case["F"], n_offsets=case["K"], decoded_version=bool(case["decoded"]), use_feat_bank=bool(case["bank"]))
    pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc.get_mask = t(a["anchor"]), t(a["feat"]), t(a["offset"]), t(a["scaling"]), t(a["mask"])
    pc.get_mask_anchor = (pc.get_mask.sum(dim=1) > 0).to(dtype)
    pc.rotation_activation = torch.nn.functional.normalize
    pc.get_opacity_mlp = _sequential(torch, a, "opacity", nn.Tanh(), device, dtype)
    pc.get_cov_mlp = _sequential(torch, a, "cov", None, device, dtype)
    pc.get_color_mlp = _sequential(torch, a, "color", nn.Sigmoid(), device, dtype)
    if case["bank"]:
        pc.get_featurebank_mlp = _sequential(torch, a, "bank", nn.Softmax(dim=1), device, dtype)
    vis = torch.tensor(np.asarray(a["vis"]), device=device)
    if not case["decoded"]:
        pc.get_grid_mlp = _sequential(torch, a, "grid", None, device, dtype)
        ctx = t(a["ctx"])
        pc.ng_rows = None                 # set by the caller to the mask in force (None: every anchor)

        def calc_interp_feat(anchor):
            out = ctx if pc.ng_rows is None else ctx[pc.ng_rows]
            assert out.shape[0] == anchor.shape[0]
            return out

        pc.calc_interp_feat = calc_interp_feat
    cam = types.SimpleNamespace(camera_center=t(a["cam"]))
    return pc, cam, vis


def ng_mutate(case, a, name, offset=0):
    """The generator's mutations of the weights (each must move the reference's float64 outputs by >= 100 x the tolerance).  offset: the
    offset whose rows are exchanged -- the generator names one that has a kept Gaussian."""
    a = {k: v.copy() for k, v in a.items()}
    F, K = case["F"], case["K"]
    if name == "exchange_ob_view_ob_dist":                       # the MLPs read [feat, ob_dist, ob_view] instead of [feat, ob_view, ob_dist]
        for mlp in ("opacity", "cov", "color"):
            a[f"{mlp}_w1"][:, F:F + 4] = a[f"{mlp}_w1"][:, [F + 1, F + 2, F + 3, F]]
    elif name == "exchange_cov_scale_rot_rows":                  # one offset: its first scale column with its first rotation column
        r = 7 * offset
        for key in ("cov_w2", "cov_b2"):
            a[key][[r, r + 3]] = a[key][[r + 3, r]]
    elif name == "exchange_bank_first_last":
        for key in ("bank_w2", "bank_b2"):
            a[key][[0, 2]] = a[key][[2, 0]]
    elif name == "exchange_opacity_offsets":                     # the offset and the next one
        o, p = offset, (offset + 1) % K
        for key in ("opacity_w2", "opacity_b2"):
            a[key][[o, p]] = a[key][[p, o]]
    else:
        raise KeyError(name)
    return a


NG_MUTATIONS = ("exchange_ob_view_ob_dist", "exchange_cov_scale_rot_rows", "exchange_bank_first_last", "exchange_opacity_offsets")
