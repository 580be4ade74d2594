"""Generate tests/golden/wiring_<case>.npz by RUNNING the reference's own GausPcgc Python -- `Network.forward`
(src/ai_pcc/GausPcgc/network_ue_4stage_conv.py:100-182, kit/nn.py:9-117), `compress_point_cloud` and `decompress_point_cloud`
(src/gs_compress/HAC/utils/pcc_utils.py:24-217, 230-400) -- from a checkout of the reference project (not part of this repository):

    python tests/golden/make_wiring.py <reference checkout>

Only inputs and what the reference's programs computed or wrote are stored -- no reference source text.

torchsparse and torchac are absent from the reference tree, so the reference runs on a CPU under small functional
stand-ins, this project's own code, installed in sys.modules before the reference modules are imported:

  torchsparse   SparseTensor (coords / feats, C / F, to(), + on feats), nn.ReLU on feats, nn.Conv3d with the parameter `kernel`
                (k^3, Cin, Cout).  Stride 1: a gather - matmul - sum over a coordinate dictionary, in the dtype of its input, the k^3
                offsets enumerated x fastest, o = (dx + r) + k (dy + r) + k^2 (dz + r) (gauspcc_amd.model.conv_offset_layout).
                Stride 2, k = 2 (FOG): output coordinates unique(coords // 2) in (batch, z, y, x) order, features summed over the children.
  torchac       encode / decode_int16_normalized_cdf on the oracle's restatement of torchac's coder; every (cdf rows, symbols) pair recorded.
  kit.nn.torch  a forwarding proxy that drops device='cuda' from tensor() and arange() (kit/nn.py:36,73,75).

LIMIT.  torchsparse's own offset order and its own output row order are not in the reference tree and stay unpinned: the
stand-in uses this project's reading of both.  GAUSPCC_OFFSET_ORDER / GAUSPCC_FLIP_OFFSETS remain the answer for those.  Likewise
torchac's arithmetic.  What these fixtures pin is the reference's Python: data flow, stage split, orderings, the stopping rule, the
container header, the key names, the loss and its gradient.

Cases (weights: gauspcc_amd.synth.synthetic_state_dict(32, k, seed), saved with torch.save and loaded by the reference's own
load_state_dict; their sha256 is stored).  Clouds are grown top-down from a seeded set of nodes, a seeded non-empty child set per
node, so that a few hundred points give three coded levels with every stage alphabet fully used and all eight octants present:
  k3_exact64   k = 3; one level has exactly 64 nodes (the `< 64` stopping rule, :108); carries the float64 gradient of bpp
               (wiring_k3_exact64_grad.npz: with 18 x 512 kernel samples in float64 it is kept in a file of its own)
  k5_negative  k = 5; negative coordinates (the reference's loop takes them as they are: floor halving, non-negative remainders)
  k3_posq      k = 3; posQ = 2.5
Duplicate input rows are not a case: the reference's loop sums the duplicate children's occupancy bits (kit/nn.py:53-54), which
is no occupancy code any more, and this library refuses them.

The run ends with a mutation self-check through the reference itself (see MUTATIONS): each must move the float64 probabilities by
at least 100 x the tolerance the tests use.
"""
import hashlib
import importlib
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGE_M = (2, 2, 4, 16)
PROB_TOL = 1e-5          # the project's tolerance on probabilities (tests/test_oracle_independent.py)
GRAD_SAMPLES = 512
EMB_SCALE = 1.0          # factor on the embedding tables, should the synthetic weights be too tame for the mutation check
CASES = (
    # name, k, weight seed, cloud seed, top level, origin of the top level, coded levels, posQ, gradient
    dict(name="k3_exact64", k=3, wseed=5, cseed=101, top="cube4", origin=(2, 6, 4), depth=2, posQ=1, grad=True),
    dict(name="k5_negative", k=5, wseed=7, cseed=102, top="blob", origin=(-9, -3, -14), depth=2, posQ=1, grad=False),
    dict(name="k3_posq", k=3, wseed=11, cseed=103, top="blob", origin=(40, 1, 17), depth=2, posQ=2.5, grad=False),
)
MUTATIONS = ("swap_target_embedding_rows_1_2", "swap_s2_emb_rows_1_2", "exchange_spatial_conv_s1_s2", "exchange_target_resnet_blocks")


# ---------------------------------------------------------------------------------------------------------------- stand-ins
class SparseTensor:
    def __init__(self, feats=None, coords=None, stride=1, **kw):
        self.coords, self.feats, self.stride = coords, feats, stride

    C = property(lambda self: self.coords, lambda self, v: setattr(self, "coords", v))
    F = property(lambda self: self.feats, lambda self, v: setattr(self, "feats", v))

    def to(self, *a, **kw):
        return self

    def __add__(self, other):
        return SparseTensor(coords=self.coords, feats=self.feats + other.feats)


class SpReLU(nn.Module):
    def __init__(self, inplace=True):
        super().__init__()

    def forward(self, x):
        return SparseTensor(coords=x.coords, feats=torch.relu(x.feats))


_PAIRS = {}


def _pairs(coords, k):
    """[(rows out, rows in)] per offset o = (dx + r) + k (dy + r) + k^2 (dz + r): the rows whose neighbour at +d exists."""
    c = coords.detach().cpu().numpy().astype(np.int64)
    key = (c.tobytes(), k)
    if key not in _PAIRS:
        r = k // 2
        row = {tuple(v): i for i, v in enumerate(c.tolist())}
        assert len(row) == len(c), "duplicate coordinates"
        out = []
        for o in range(k ** 3):
            dx, dy, dz = o % k - r, (o // k) % k - r, o // (k * k) - r
            dst, src = [], []
            for i, (b, x, y, z) in enumerate(c.tolist()):
                j = row.get((b, x + dx, y + dy, z + dz))
                if j is not None:
                    dst.append(i)
                    src.append(j)
            out.append((torch.tensor(dst, dtype=torch.long), torch.tensor(src, dtype=torch.long)))
        _PAIRS[key] = out
    return _PAIRS[key]


class SpConv3d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, bias=False, **kw):
        super().__init__()
        assert not bias and (stride, kernel_size) in ((1, 3), (1, 5), (1, 7), (2, 2))
        self.k, self.stride = kernel_size, stride
        bound = 1.0 / np.sqrt(in_channels * kernel_size ** 3)
        self.kernel = nn.Parameter(torch.empty(kernel_size ** 3, in_channels, out_channels).uniform_(-bound, bound))

    def forward(self, x):
        w = self.kernel.to(x.feats.dtype)
        if self.stride == 1:
            out = x.feats.new_zeros(x.feats.shape[0], w.shape[2])
            for o, (dst, src) in enumerate(_pairs(x.coords, self.k)):
                if len(dst):
                    out = out.index_add(0, dst, x.feats[src] @ w[o])
            return SparseTensor(coords=x.coords, feats=out)
        c = x.coords
        par = torch.cat((c[:, :1], torch.div(c[:, 1:], 2, rounding_mode="floor")), dim=1)
        child = (c[:, 1] % 2 + 2 * (c[:, 2] % 2) + 4 * (c[:, 3] % 2)).long()
        up, inv = torch.unique(par, dim=0, return_inverse=True)
        u = up.cpu().numpy()
        order = np.lexsort((u[:, 1], u[:, 2], u[:, 3], u[:, 0]))     # (batch, z, y, x)
        rank = torch.empty(len(order), dtype=torch.long)
        rank[torch.as_tensor(order)] = torch.arange(len(order))
        feats = x.feats.new_zeros(up.shape[0], w.shape[2]).index_add(0, rank[inv], torch.bmm(x.feats.unsqueeze(1), w[child]).squeeze(1))
        return SparseTensor(coords=up[torch.as_tensor(order)].to(c.dtype), feats=feats)


class Recorder:
    def reset(self, dtype=torch.float32):
        self.dtype = dtype
        self.cdf_float, self.enc, self.dec, self.coords = [], [], [], []


REC = Recorder()


def _ac_encode(cdf, sym):
    from oracle import oracle as orc

    assert cdf.dtype == torch.int16 and sym.dtype == torch.int16
    REC.enc.append((cdf.numpy().copy(), sym.numpy().copy()))
    return orc.rc_encode(cdf.numpy().view(np.uint16), sym.numpy().astype(np.uint8))


def _ac_decode(cdf, data):
    from oracle import oracle as orc

    assert cdf.dtype == torch.int16
    sym = orc.rc_decode(cdf.numpy().view(np.uint16), data)
    REC.dec.append((cdf.numpy().copy(), sym.copy()))
    return torch.from_numpy(sym.astype(np.int16))


class _TorchProxy:
    """torch, with device='cuda' dropped from tensor() and arange()."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def tensor(*a, **kw):
        kw.pop("device", None)
        return torch.tensor(*a, **kw)

    @staticmethod
    def arange(*a, **kw):
        kw.pop("device", None)
        return torch.arange(*a, **kw)


def _module(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def import_reference(ref):
    from oracle import oracle as orc

    orc.build()
    _module("torchac", encode_int16_normalized_cdf=_ac_encode, decode_int16_normalized_cdf=_ac_decode)
    cfg = types.SimpleNamespace(get_default_conv_config=lambda: types.SimpleNamespace(), set_global_conv_config=lambda c: None)
    fn = _module("torchsparse.nn.functional", conv_config=cfg)
    spnn = _module("torchsparse.nn", Conv3d=SpConv3d, ReLU=SpReLU, functional=fn)
    _module("torchsparse", SparseTensor=SparseTensor, nn=spnn)
    sys.path.insert(0, os.path.join(ref, "src/ai_pcc/GausPcgc"))
    sys.path.insert(0, os.path.join(ref, "src/gs_compress/HAC"))
    knn = importlib.import_module("kit.nn")
    knn.torch = _TorchProxy()
    op = importlib.import_module("kit.op")
    net = importlib.import_module("network_ue_4stage_conv")
    pcc_utils = importlib.import_module("utils.pcc_utils")
    convert = op._convert_to_int_and_normalize

    def recording_convert(cdf_float, needs_normalization):
        REC.cdf_float.append(cdf_float.detach().clone())
        return convert(cdf_float, needs_normalization)

    op._convert_to_int_and_normalize = recording_convert
    TargetEmbedding = knn.TargetEmbedding

    def coded_coordinates(module, args, output):
        if isinstance(module, TargetEmbedding):     # called once per coded level with the coordinates in coded order
            REC.coords.append(args[1].detach().clone())

    nn.modules.module.register_module_forward_hook(coded_coordinates)
    return pcc_utils, net.Network


# ---------------------------------------------------------------------------------------------------------------- clouds
def grow_cloud(seed, top, origin, depth):
    """Seeded top-down cloud: `top` nodes, then depth + 1 times a non-empty child set per node (4 in 5 nodes: one or two children,
    the others: each child with probability 1/2), so the last expansion gives the points: depth + 1 coded levels (the top nodes are the first coded level)."""
    rng = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(4 if top == "cube4" else 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    if top == "blob":
        g = g[rng.permutation(len(g))[:72]]
    c = g.astype(np.int64) + np.asarray(origin, dtype=np.int64)
    for _ in range(depth + 1):
        nxt = []
        for node in c:
            if rng.rand() < 0.8:
                occ = np.zeros(8, bool)
                occ[rng.permutation(8)[: 1 + (rng.rand() < 0.3)]] = True
            else:
                occ = rng.rand(8) < 0.5
                if not occ.any():
                    occ[rng.randint(8)] = True
            for j in np.nonzero(occ)[0]:
                nxt.append(node * 2 + np.array([j & 1, (j >> 1) & 1, j >> 2]))
        c = np.asarray(nxt, dtype=np.int64)
    return np.ascontiguousarray(c[rng.permutation(len(c))].astype(np.int32))


def weights(k, seed):
    from gauspcc_amd.synth import synthetic_state_dict

    sd = synthetic_state_dict(32, k, seed)
    if EMB_SCALE != 1.0:
        for key in sd:
            if "emb" in key:
                sd[key] = (sd[key] * np.float32(EMB_SCALE)).astype(np.float32)
    return sd


def weights_sha256(sd):
    h = hashlib.sha256()
    for key in sorted(sd):
        h.update(key.encode())
        h.update(np.ascontiguousarray(sd[key], dtype=np.float32).tobytes())
    return h.hexdigest()


def mutate(sd, name):
    sd = {k: v.copy() for k, v in sd.items()}
    if name == "swap_target_embedding_rows_1_2":
        sd["target_embedding.target_res_embedding.weight"][[1, 2]] = sd["target_embedding.target_res_embedding.weight"][[2, 1]]
    elif name == "swap_s2_emb_rows_1_2":
        sd["pred_head_s2_emb.weight"][[1, 2]] = sd["pred_head_s2_emb.weight"][[2, 1]]
    elif name == "exchange_spatial_conv_s1_s2":
        for j in (0, 2):
            a, b = f"spatial_conv_s1.{j}.kernel", f"spatial_conv_s2.{j}.kernel"
            sd[a], sd[b] = sd[b], sd[a]
    elif name == "exchange_target_resnet_blocks":
        for j in ("conv0", "conv1"):
            a, b = f"target_resnet.2.{j}.kernel", f"target_resnet.3.{j}.kernel"
            sd[a], sd[b] = sd[b], sd[a]
    else:
        raise KeyError(name)
    return sd


# ---------------------------------------------------------------------------------------------------------------- runs
def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member, so that a rerun reproduces the file bit for bit."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def save_ckpt(sd, path):
    torch.save({k: torch.tensor(v) for k, v in sd.items()}, path)


def run_compress(pcc_utils, pts, ckpt, k, posQ, dtype, out_path):
    """The reference's compress_point_cloud -> (its dict, per level: coords, per (level, stage): float CDF rows, int16 rows, symbols)."""
    REC.reset(dtype)
    torch.set_default_dtype(dtype)      # the network compress_point_cloud constructs, and so the whole run, in this dtype
    try:
        res = pcc_utils.compress_point_cloud(pts, ckpt, out_path, channels=32, kernel_size=k, posQ=posQ)
    finally:
        torch.set_default_dtype(torch.float32)
    L = len(REC.coords)
    assert L >= 1 and len(REC.cdf_float) == 4 * L == len(REC.enc)
    return res, list(REC.coords), list(REC.cdf_float), list(REC.enc)


def probs_of(cdf_float):
    return [(c[:, 1:] - c[:, :-1]).double().numpy() for c in cdf_float]


def run_forward(Network, sd_path, pts, k, dtype, grad=False):
    net = Network(channels=32, kernel_size=k)
    net.load_state_dict(torch.load(sd_path))
    if dtype == torch.float64:
        net = net.double()
    xyz = torch.tensor(pts)
    coords = torch.cat((xyz[:, 0:1] * 0, xyz), dim=-1).int()
    x = SparseTensor(coords=coords, feats=torch.ones((coords.shape[0], 1), dtype=torch.float))
    bpp = net(x)
    grads = None
    if grad:
        bpp.backward()
        grads = {n: p.grad.detach().numpy().copy() for n, p in net.named_parameters() if p.requires_grad}
    return float(bpp.detach()), grads, {n: tuple(v.shape) for n, v in net.state_dict().items()}


def stage_diffs(a, b):
    """max |a - b| per stage over the levels of two per-(level, stage) probability lists."""
    return [max(float(np.abs(a[i] - b[i]).max()) for i in range(s, len(a), 4)) for s in range(4)]


def make_case(pcc_utils, Network, case, tmp):
    name, k, posQ = case["name"], case["k"], case["posQ"]
    pts = grow_cloud(case["cseed"], case["top"], case["origin"], case["depth"])
    assert len(np.unique(pts, axis=0)) == len(pts)
    sd = weights(k, case["wseed"])
    ckpt = os.path.join(tmp, f"{name}.pt")
    save_ckpt(sd, ckpt)
    bin_path = os.path.join(tmp, f"{name}.bin")

    res, coords, cdf32, enc = run_compress(pcc_utils, pts, ckpt, k, posQ, torch.float32, bin_path)
    with open(bin_path, "rb") as f:
        blob = f.read()
    _, coords64, cdf64, _ = run_compress(pcc_utils, pts, ckpt, k, posQ, torch.float64, os.path.join(tmp, f"{name}_f64.bin"))
    assert len(coords) == len(coords64) == case["depth"] + 1 and all(torch.equal(a, b) for a, b in zip(coords, coords64))
    p32, p64 = probs_of(cdf32), probs_of(cdf64)
    f32_vs_f64 = stage_diffs(p32, p64)
    tol = [max(PROB_TOL, 4 * d) for d in f32_vs_f64]

    out = dict(points=pts, k=np.int32(k), posQ=np.float64(posQ), weight_seed=np.int32(case["wseed"]), cloud_seed=np.int32(case["cseed"]),
               emb_scale=np.float64(EMB_SCALE), weights_sha256=np.array(weights_sha256(sd)), levels=np.int32(len(coords)),
               f32_vs_f64=np.array(f32_vs_f64), bin=np.frombuffer(blob, np.uint8), file_size_bits=np.int64(res["file_size_bits"]),
               compress_num_points=np.int64(res["num_points"]))
    octants = set()
    for d, c in enumerate(coords):
        c = c.numpy()
        assert not c[:, 0].any()
        out[f"l{d}_xyz"] = c[:, 1:].astype(np.int32)
        octants |= set(((c[:, 1] & 1) + 2 * (c[:, 2] & 1) + 4 * (c[:, 3] & 1)).tolist())
        for s in range(4):
            cdf, sym = enc[4 * d + s]
            out[f"l{d}_s{s}_sym"] = sym.astype(np.uint8)
            out[f"l{d}_s{s}_cdf"] = cdf
            out[f"l{d}_s{s}_prob"] = p64[4 * d + s].astype(np.float32)
            out[f"l{d}_s{s}_f32_vs_f64"] = np.float64(np.abs(p32[4 * d + s] - p64[4 * d + s]).max())
    for s, m in enumerate(STAGE_M):
        used = set(np.concatenate([enc[4 * d + s][1] for d in range(len(coords))]).tolist())
        assert used == set(range(m)), (name, s, sorted(used))
    assert octants == set(range(8)), name

    for flag in (True, False):
        REC.reset(torch.float32)
        dec = pcc_utils.decompress_point_cloud(bin_path, ckpt, None, channels=32, kernel_size=k, is_data_pre_quantized=flag)
        assert all(torch.equal(a, b) for a, b in zip(coords, REC.coords)) and all(np.array_equal(e[1], d_[1]) for e, d_ in zip(enc, REC.dec))
        pc = dec["point_cloud"]
        tag = "preq" if flag else "raw"
        out[f"dec_{tag}"] = pc.numpy()
        out[f"dec_{tag}_dtype"] = np.array(str(pc.dtype))
        out[f"dec_{tag}_num_points"] = np.int64(dec["num_points"])
        if flag:
            srt = lambda a: a[np.lexsort((a[:, 0], a[:, 1], a[:, 2]))]
            assert np.array_equal(srt(np.round(pc.numpy() / np.float16(posQ)).astype(np.int64)), srt(pts.astype(np.int64)))

    bpp64, grads, shapes = run_forward(Network, ckpt, pts, k, torch.float64, grad=case["grad"])
    bpp32, _, _ = run_forward(Network, ckpt, pts, k, torch.float32)
    out["bpp_f64"], out["bpp_f32"] = np.float64(bpp64), np.float32(bpp32)
    out["keys"] = np.array(sorted(shapes))
    out["key_shapes"] = np.array([" ".join(map(str, shapes[n])) for n in sorted(shapes)])

    moves = {}
    for mname in MUTATIONS:
        mck = os.path.join(tmp, f"{name}_{mname}.pt")
        save_ckpt(mutate(sd, mname), mck)
        _, _, mcdf, _ = run_compress(pcc_utils, pts, mck, k, posQ, torch.float64, os.path.join(tmp, "mut.bin"))
        mv = stage_diffs(probs_of(mcdf), p64)
        moves[mname] = mv
        ratio = max(m / t for m, t in zip(mv, tol))
        assert ratio >= 100, f"{name}: mutation {mname} moves the probabilities by only {ratio:.1f} x the tolerance: raise EMB_SCALE"
        out[f"mutation_{mname}"] = np.array(mv)
    save_npz(os.path.join(HERE, f"wiring_{name}.npz"), out)

    if case["grad"]:
        from gauspcc_amd.synth import CONV_KEYS

        g = {"bpp_f64": np.float64(bpp64), "weights_sha256": out["weights_sha256"]}
        rng = np.random.RandomState(case["cseed"] + 1)
        for n, v in grads.items():
            if n in CONV_KEYS:
                pos = np.sort(rng.choice(v.size, GRAD_SAMPLES, replace=False))
                g[f"pos/{n}"] = pos.astype(np.uint16 if v.size <= 65536 else np.int32)
                g[f"val/{n}"] = v.reshape(-1)[pos]
                g[f"sum/{n}"] = np.float64(v.sum())
                g[f"norm/{n}"] = np.float64(np.sqrt((v * v).sum()))
            else:
                g[f"full/{n}"] = v
        save_npz(os.path.join(HERE, f"wiring_{name}_grad.npz"), g)

    n_nodes = [len(c) for c in coords]
    print(f"{name}: {len(pts)} points, coded levels {n_nodes}, base {int(np.frombuffer(blob[2:6], np.int32)[0])} nodes, {len(blob)} B, "
          f"bpp f64 {bpp64:.9f} f32 {bpp32:.7f}")
    print(f"  reference float32 vs float64, max |dp| per stage: " + " ".join(f"{d:.2e}" for d in f32_vs_f64))
    for mname, mv in moves.items():
        print(f"  mutation {mname}: max |dp| per stage " + " ".join(f"{d:.2e}" for d in mv))


def main(ref):
    torch.manual_seed(0)
    torch.set_num_threads(1)          # one summation order, whatever the machine
    pcc_utils, Network = import_reference(ref)
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            make_case(pcc_utils, Network, case, tmp)
    print("wiring fixtures written to", HERE)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
