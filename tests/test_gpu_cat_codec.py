"""GPU tests of CAT-3DGS's attribute loop (gauspcc_amd.cat_codec): conduct_encoding -> conduct_decoding on the slice of GaussianModel the
reference's methods touch (src/gs_compress/CAT-3DGS/scene/gaussian_model.py:1056-1616; gauspcc_amd.synth.SyntheticGaussianModelCAT), the pipelined
chain decoder gsac_decode_normal_chain against the staged path (gshac_mlp2 + decoder_gaussian_slices, stage after stage), and estimate_final_bits.

The round trip is EXACT: the expectation is computed outside cat_codec -- the tri-plane sampler's public call, the context head by the ORACLE on
the host (gshac_mlp2 == orc.mlp2 bit for bit, tests/test_gpu_tcgs_codec.py), the step sizes Q0 * (1.1 + tanh(adj)), STE_multistep with the
global means -- and compared with torch.equal.  The context and one chained stage's mean / scale are held to a float64 evaluation by the
project's usual rule: no further from it than 4 x what torch's float32 modules are."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FACTOR = 4.0
F = 50
TRI_FILES = {f"{p}_bitstream_{j}.bin" for p in ("xy", "yz", "zx") for j in range(2)}
GPCC_ERR_ARG, GPCC_ERR_FORMAT = -2, -5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch


def _model(torch, N, seed, groups=(12, 12, 13, 13), on_s=False, on_o=False, n_offsets=10, kept="random"):
    """A synthetic model of which exactly N anchors are kept: the first N rows keep offset 0 (and, `random`, whatever their seeded logits say; `all`:
    every offset), the others keep none.  Tri-plane resolution 32; scaling spread 0.05 (alphabets of the scaling attribute wider than a wave)."""
    from gauspcc_amd.synth import SyntheticGaussianModelCAT

    m = SyntheticGaussianModelCAT(N + 24, seed=seed, chcm_slices_list=groups, chcm_for_scaling=on_s, chcm_for_offsets=on_o, n_offsets=n_offsets,
                                  resolution=32, scaling_spread=0.05, device="cuda:0")
    with torch.no_grad():
        m._mask[N:] = -20.0
        m._mask[:N, 0] = 5.0
        if kept == "all":
            m._mask[:N] = 5.0
    assert int(m.get_mask_anchor(None).sum()) == N
    return m


def _decoder_model(torch, enc, seed):
    """a fresh model that shares only the networks (a COPY of the feature net, its tri-plane grids zeroed: the decoder must take the planes from the files)"""
    dec = _model(torch, 40, seed + 50, groups=tuple(enc.chcm_slices_list), on_s=enc.chcm_for_scaling, on_o=enc.chcm_for_offsets, n_offsets=enc.n_offsets)
    dec.feature_net = copy.deepcopy(enc.feature_net)
    with torch.no_grad():
        for level in dec.feature_net.attribute_net.grid.grids:
            for p in level:
                p.zero_()
    dec.mlp_chcm_list = enc.mlp_chcm_list
    for name in ("mlp_chcm_scaling", "mlp_chcm_offsets"):
        if hasattr(enc, name):
            setattr(dec, name, getattr(enc, name))
    dec._anchor_feat = torch.zeros(1, enc.feat_dim, device="cuda")
    return dec


def _encode(torch, tmp, enc):
    from gauspcc_amd import cat_codec

    patched, log, rate_set = cat_codec.conduct_encoding(enc, str(tmp), None, ckpt_path="synthetic")
    return patched, log, rate_set


def _decode(torch, tmp, enc, patched, seed, chain):
    from gauspcc_amd import cat_codec

    dec = _decoder_model(torch, enc, seed)
    msg = cat_codec.conduct_decoding(dec, str(tmp), patched, None, ckpt_path="synthetic", chain=chain)
    assert msg.startswith("\nDecTime") and dec.decoded_version is True
    return dec


def _ste(torch, x, Q, mean):
    """STE_multistep.forward (CAT-3DGS/utils/encodings.py:268-280) with the GLOBAL mean, as the reference's loop calls it"""
    x = torch.clamp(x, min=(mean - 15_000 * Q), max=(mean + 15_000 * Q))
    return torch.round(x / Q) * Q


def _grid_features(torch, enc, anchor):
    from gauspcc_amd.cat_triplane import ms_triplane_sample

    grid = enc.feature_net.attribute_net.grid
    return ms_triplane_sample(anchor, [list(g) for g in grid.grids], level=2, quantise=True, aabb=grid.aabb)


def _expected(torch, orc, enc):
    """anchors in the decoder's order, the source attributes in that order, the oracle's context row and the quantised attributes"""
    net = enc.feature_net.attribute_net
    K = enc.n_offsets
    with torch.no_grad():
        keep = enc.get_mask_anchor(None)
        a_int = torch.round(enc.get_anchor[keep] / enc.voxel_size)
        key = (a_int - a_int.min(dim=0, keepdim=True).values).to(torch.int64)
        M = key.max() + 1
        order = torch.argsort(key[:, 0] + key[:, 1] * M + key[:, 2] * M * M)       # calculate_morton_order (pcc_utils.py:12-22)
        anchor = a_int[order] * enc.voxel_size
        src = dict(feat=enc._anchor_feat[keep][order], scaling=enc.get_scaling[keep][order], mask=enc.get_mask(None)[keep][order], offs=enc._offset[keep][order])
        w1, b1, w2, b2 = (t.detach().cpu().numpy() for t in (net.feature_out[0].weight, net.feature_out[0].bias, net.net[1].weight, net.net[1].bias))
        ctx = torch.tensor(orc.mlp2(_grid_features(torch, enc, anchor).cpu().numpy(), w1, b1, w2, b2), device="cuda")
        c = 2 * F + 12 + 6 * K
        Q = dict(feat=1 * (1.1 + torch.tanh(ctx[:, c:c + 1])), scaling=0.001 * (1.1 + torch.tanh(ctx[:, c + 1:c + 2])), offsets=0.2 * (1.1 + torch.tanh(ctx[:, c + 2:c + 3])))
        m3 = src["mask"].repeat(1, 1, 3).view(-1, 3 * K)
        want = {"_anchor_feat": _ste(torch, src["feat"], Q["feat"], src["feat"].mean()),
                "_scaling": _ste(torch, src["scaling"], Q["scaling"], enc.get_scaling.mean()),
                "_offset": (_ste(torch, src["offs"].reshape(-1, 3 * K), Q["offsets"], enc._offset.mean()) * m3).view(-1, K, 3)}   # offsets[~mask] = 0 (:1346)
    return anchor, src, ctx, Q, want


def _check_exact(torch, enc, dec, N, anchor, src, want, rows=None):
    K = enc.n_offsets
    assert torch.equal(dec._anchor.data, anchor) and torch.equal(dec._mask.data, src["mask"])
    for name, shape in (("_anchor", (N, 3)), ("_anchor_feat", (N, F)), ("_scaling", (N, 6)), ("_offset", (N, K, 3)), ("_mask", (N, K, 1))):
        assert isinstance(getattr(dec, name), torch.nn.Parameter) and tuple(getattr(dec, name).shape) == shape, name
    sl = slice(None) if rows is None else rows
    for name, w in want.items():
        got = getattr(dec, name).data
        assert torch.equal(got[sl], w[sl]), (name, int((got[sl] != w[sl]).sum()), float((got[sl] - w[sl]).abs().max()))
    assert float(dec._offset.data[src["mask"].expand(-1, -1, 3) == 0].abs().max() if (src["mask"] == 0).any() else 0.0) == 0.0


def _check_contract(torch, tmp, enc, patched, log, rate_set, N):
    G, K = enc.num_feat_slices, enc.n_offsets
    steps = -(-N // 500)
    assert len(patched) == 12
    n_full, n_kept, mb, infos, min_f, max_f, min_s, max_s, min_o, max_o, prob_masks, tri = patched
    assert mb == 500 and n_full == enc._anchor.shape[0] and n_kept == N and infos == [None] * steps and 0.0 < prob_masks <= 1.0
    for lists in (min_f, max_f):                         # [group][slice] of 0-d tensors
        assert isinstance(lists, list) and len(lists) == G
        assert all(isinstance(l, list) and len(l) == steps and all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in l) for l in lists)
    for l in (min_s, max_s, min_o, max_o):
        assert isinstance(l, list) and len(l) == steps and all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in l)
    assert isinstance(tri, list) and len(tri) == 3 and all(len(t) == 2 for t in tri)          # AC_MAX_VAL per plane and level
    stems = [f"feat{i}" for i in range(G)] + ["scaling", "offsets"]
    assert set(os.listdir(tmp)) == {"xyz_pcc.bin", "masks.b"} | TRI_FILES | {f"{a}_{s}.b" for a in stems for s in range(steps)}
    assert len(rate_set) == 7 + G and all(isinstance(v, float) for v in rate_set)
    assert log.startswith("\nEncoded sizes in MB: anchor ") and ", total_feat " in log and all(f"feat{i} " in log for i in range(G))
    assert ", Triplane_f " in log and ",Total " in log and ", EncTime " in log
    assert log.index("scaling ") < log.index("offsets ") < log.index("masks ") < log.index("MLPs ") < log.index("Triplane_f ")


# ---------------------------------------------------------------- the shared case: 1 037 anchors, the default groups, both MLP flags on
@pytest.fixture(scope="module")
def full_case(torch_cuda, orc, tmp_path_factory):
    """slices of 500, 500 and 37 (37 is prime: a last block that is partial for every B, a slice shorter than one block for B > 37); six stages, the
    longest pipeline of the default groups.  Decoded once per path."""
    torch = torch_cuda
    tmp = tmp_path_factory.mktemp("cat_1037")
    enc = _model(torch, 1037, 11, on_s=True, on_o=True)
    patched, log, rate_set = _encode(torch, tmp, enc)
    exp = _expected(torch, orc, enc)
    dec_chain = _decode(torch, tmp, enc, patched, 11, True)
    dec_staged = _decode(torch, tmp, enc, patched, 12, False)
    return dict(tmp=tmp, enc=enc, patched=patched, log=log, rate_set=rate_set, exp=exp, chain=dec_chain, staged=dec_staged, N=1037)


def test_roundtrip_three_slices_exact_and_contract(torch_cuda, full_case):
    c = full_case
    anchor, src, ctx, Q, want = c["exp"]
    _check_contract(torch_cuda, c["tmp"], c["enc"], c["patched"], c["log"], c["rate_set"], c["N"])
    _check_exact(torch_cuda, c["enc"], c["chain"], c["N"], anchor, src, want)
    _check_exact(torch_cuda, c["enc"], c["staged"], c["N"], anchor, src, want)
    for name in ("_anchor_feat", "_scaling", "_offset"):
        assert torch_cuda.equal(getattr(c["chain"], name).data, getattr(c["staged"], name).data), name


def test_wide_alphabets_are_present(torch_cuda, full_case):
    """scaling spread 0.05 over Q ~ 0.001: the 64-wide window and the binary-search tiers run on rows that depend on decoded values"""
    p = full_case["patched"]
    widths = [float(mx - mn) for mn, mx in zip(p[6], p[7])]
    print("scaling alphabets (max - min per slice):", widths)
    assert max(widths) > 64


@pytest.mark.parametrize("N", [1, 499, 500, 501])
def test_sizes_exact(torch_cuda, orc, tmp_path, N):
    """501: a one-anchor slice, whose pipeline is all lag; 1: a single anchor"""
    torch = torch_cuda
    enc = _model(torch, N, 20 + N, on_s=True, on_o=True)
    patched, log, rate_set = _encode(torch, tmp_path, enc)
    _check_contract(torch, tmp_path, enc, patched, log, rate_set, N)
    anchor, src, ctx, Q, want = _expected(torch, orc, enc)
    dec = _decode(torch, tmp_path, enc, patched, N, True)
    _check_exact(torch, enc, dec, N, anchor, src, want)
    dec2 = _decode(torch, tmp_path, enc, patched, N + 1, False)
    for name in ("_anchor_feat", "_scaling", "_offset"):
        assert torch.equal(getattr(dec, name).data, getattr(dec2, name).data), name


@pytest.mark.parametrize("groups,on_s,on_o,n_offsets,kept", [
    ((12, 12, 13, 13), False, False, 10, "random"),
    ((5, 10, 15, 20), True, False, 10, "all"),
    ((25, 25), False, True, 5, "random"),
    ((50,), False, False, 10, "random"),          # no MLP stage at all
    ((50,), True, True, 5, "all"),
])
def test_configurations_exact(torch_cuda, orc, tmp_path, groups, on_s, on_o, n_offsets, kept):
    torch = torch_cuda
    N = 1037
    enc = _model(torch, N, 31 + len(groups) + n_offsets, groups=groups, on_s=on_s, on_o=on_o, n_offsets=n_offsets, kept=kept)
    if kept == "all":
        assert bool((enc.get_mask(None)[enc.get_mask_anchor(None)] == 1).all())
    patched, log, rate_set = _encode(torch, tmp_path, enc)
    _check_contract(torch, tmp_path, enc, patched, log, rate_set, N)
    anchor, src, ctx, Q, want = _expected(torch, orc, enc)
    dec = _decode(torch, tmp_path, enc, patched, 3, True)
    _check_exact(torch, enc, dec, N, anchor, src, want)
    dec2 = _decode(torch, tmp_path, enc, patched, 4, False)
    _check_exact(torch, enc, dec2, N, anchor, src, want)


def test_second_encode_writes_identical_files(torch_cuda, full_case, tmp_path):
    c = full_case
    patched2, _, _ = _encode(torch_cuda, tmp_path, c["enc"])
    assert sorted(os.listdir(tmp_path)) == sorted(os.listdir(c["tmp"]))
    for f in os.listdir(c["tmp"]):
        assert open(c["tmp"] / f, "rb").read() == open(tmp_path / f, "rb").read(), f
    for a, b in zip(c["patched"][4:6], patched2[4:6]):
        assert all(torch_cuda.equal(u, v) for la, lb in zip(a, b) for u, v in zip(la, lb))
    for a, b in zip(c["patched"][6:10], patched2[6:10]):
        assert all(torch_cuda.equal(u, v) for u, v in zip(a, b))


# ---------------------------------------------------------------- the kernel through its own entry: block sizes, an empty offsets stream, errors
@pytest.fixture(scope="module")
def stage_case(torch_cuda, full_case, tmp_path_factory):
    """The stages of the shared model coded with keep flags of the test's own: random, but NOTHING kept in slice 1 (anchors 500 .. 999) -- through
    the model an anchor without offsets is not coded at all, so this comes in below conduct_encoding.  Decoded once by the staged path."""
    torch = torch_cuda
    from gauspcc_amd import cat_codec

    tmp = tmp_path_factory.mktemp("cat_stages")
    enc = full_case["enc"]
    anchor, src, _, _, _ = full_case["exp"]
    N, K = 1037, enc.n_offsets
    with torch.no_grad():
        stages = cat_codec.stage_table(enc)
        ctx = cat_codec._context(enc, anchor)
        Q = cat_codec._step_sizes(enc, ctx)
        g = torch.Generator().manual_seed(5)
        keep = (torch.rand(N, K, generator=g) < 0.5).cuda()
        keep[500:1000] = False
        mask = keep.unsqueeze(-1).repeat(1, 1, 3).view(N, 3 * K)
        x = {"feat": _ste(torch, src["feat"], Q["feat"], src["feat"].mean()), "scaling": _ste(torch, src["scaling"], Q["scaling"], src["scaling"].mean()),
             "offsets": _ste(torch, src["offs"].reshape(N, 3 * K), Q["offsets"], src["offs"].mean()) * mask}
        bounds = cat_codec.slice_bounds(N)
        bits, mins, maxs = cat_codec.encode_stages(stages, ctx, Q, x, mask, bounds, str(tmp), 3)
        staged = cat_codec.decode_staged(stages, ctx, Q, mask, bounds, str(tmp), 3, mins, maxs, N, F, K)
    return dict(tmp=tmp, stages=stages, ctx=ctx, Q=Q, keep=keep, x=x, mins=mins, maxs=maxs, staged=staged, bits=bits, N=N, K=K)


def test_empty_offsets_stream(torch_cuda, stage_case):
    c = stage_case
    assert os.path.getsize(c["tmp"] / "offsets_1.b") == 0 and c["bits"]["offsets"][1] == 0
    assert float(c["mins"]["offsets"][1]) == 0.0 and float(c["maxs"]["offsets"][1]) == 0.0
    assert os.path.getsize(c["tmp"] / "offsets_0.b") > 0 and os.path.getsize(c["tmp"] / "offsets_2.b") > 0
    for k, v in c["x"].items():                           # the staged path gives back what was coded
        assert torch_cuda.equal(c["staged"][k], v), k


@pytest.mark.parametrize("block", [0, 1, 7, 16, 64])
def test_block_sizes_equal_staged(torch_cuda, stage_case, block):
    """through the C ABI: every block size (0: the default) gives the staged result, offsets 0 where not kept"""
    from gauspcc_amd import cat_codec

    c = stage_case
    outs = cat_codec.decode_chain(c["stages"], c["ctx"], c["Q"], c["keep"], str(c["tmp"]), 3, c["mins"], c["maxs"], c["N"], F, c["K"], block_anchors=block)
    for k in ("feat", "scaling", "offsets"):
        assert torch_cuda.equal(outs[k], c["staged"][k]), (k, block, int((outs[k] != c["staged"][k]).sum()))
    assert float(outs["offsets"][500:1000].abs().max()) == 0.0


def _records(torch, n, nstages, **over):
    """minimal valid records of `nstages` independent stages of one channel on n anchors in one slice"""
    from gauspcc_amd import _lib

    recs = (_lib.ChainStage * nstages)()
    keep = dict(q=torch.ones(n, device="cuda"), out=torch.zeros(n, nstages, device="cuda"), w=torch.zeros(4096, device="cuda"),
                cnt=np.zeros(1, dtype=np.int32), mn=np.zeros(1, dtype=np.float32), mx=np.ones(1, dtype=np.float32))
    for k, r in enumerate(recs):
        r.ch, r.dep_ch, r.dh, r.lag, r.mean_col, r.scale_col, r.feat_col, r.out_col, r.out_pitch, r.keep_group = 1, 0, 0, 0, 0, 1, -1, k, nstages, 1
        r.q_dev, r.out_dev = keep["q"].data_ptr(), keep["out"].data_ptr()
        r.bytes, r.nbytes, r.cnt, r.min_value, r.max_value = None, 0, keep["cnt"].ctypes.data, keep["mn"].ctypes.data, keep["mx"].ctypes.data
    for key, val in over.items():
        if key in ("w1", "b1", "w2", "b2"):
            val = keep["w"].data_ptr()
        setattr(recs[0], key, val)
    return recs, keep


@pytest.mark.parametrize("nstages,over,code", [
    (9, {}, GPCC_ERR_ARG),                                                               # S > 8
    (2, dict(ch=65, out_pitch=80), GPCC_ERR_ARG),                                        # ch > 64
    (2, dict(dep_ch=65, dh=16, lag=1, w1=1, b1=1, w2=1, b2=1), GPCC_ERR_ARG),            # dep_ch > 64
    (2, dict(feat_col=0, dep_ch=1, dh=129, lag=1, w1=1, b1=1, w2=1, b2=1), GPCC_ERR_ARG),   # dh > 128
    (2, dict(feat_col=0, dep_ch=1, dh=16, lag=0, w1=1, b1=1, w2=1, b2=1), GPCC_ERR_ARG),    # reads its own channel in the step that decodes it
    (2, dict(min_value="nan"), GPCC_ERR_FORMAT),
    (2, dict(min_value="wide"), GPCC_ERR_FORMAT),
    (1, {}, 0),                                                                          # the minimal records themselves are accepted
])
def test_entry_point_errors(torch_cuda, nstages, over, code):
    torch = torch_cuda
    from gauspcc_amd import _lib, runtime

    n = 3
    over = dict(over)
    bad = over.pop("min_value", None)
    recs, keep = _records(torch, n, nstages, **over)
    if bad == "nan":
        keep["mn"][0] = np.nan
    elif bad == "wide":
        keep["mn"][0], keep["mx"][0] = -40000.0, 40000.0            # more than int16 symbols
    ctx = torch.ones(n, 2, device="cuda")
    dev = ctx.device
    rc = _lib.lib().gsac_decode_normal_chain(runtime.context(dev), recs, nstages, ctx.data_ptr(), 2, n, 500, 1, 0, runtime.stream_ptr(dev))
    assert rc == code, (rc, _lib.lib().gpcc_last_error())
    if code == 0:                                                   # an empty stream reads as zeros: some value inside the alphabet, finite
        v = keep["out"][:, 0]
        assert bool(torch.isfinite(v).all()) and bool(((v == 0) | (v == 1)).all())


# ---------------------------------------------------------------- a short file
def test_short_file_gives_finite_values_inside_the_alphabet(torch_cuda, full_case, tmp_path):
    """feat1 of slice 1 cut to half its length: the decode returns, every value of that stage is finite and within [min, max] * Q of its slice, and
    the other slices are unchanged (the later stages of slice 1 depend on the damaged channels: finite is all that is asked of them)"""
    torch = torch_cuda
    import shutil

    c = full_case
    for f in os.listdir(c["tmp"]):
        shutil.copy(c["tmp"] / f, tmp_path / f)
    data = open(tmp_path / "feat1_1.b", "rb").read()
    assert len(data) > 8
    open(tmp_path / "feat1_1.b", "wb").write(data[:len(data) // 2])
    dec = _decode(torch, tmp_path, c["enc"], c["patched"], 77, True)
    anchor, src, ctx, Q, want = c["exp"]
    for name in ("_anchor_feat", "_scaling", "_offset"):
        got = getattr(dec, name).data
        assert bool(torch.isfinite(got).all()), name
        for rows in (slice(0, 500), slice(1000, 1037)):
            assert torch.equal(got[rows], want[name][rows]), (name, rows)
    assert torch.equal(dec._anchor_feat.data[500:1000, :12], want["_anchor_feat"][500:1000, :12])      # feat0 of slice 1: before the damage
    mn, mx = float(c["patched"][4][1][1]), float(c["patched"][5][1][1])
    k = torch.round(dec._anchor_feat.data[500:1000, 12:24] / Q["feat"][500:1000])
    print("damaged stage: symbols", float(k.min()), "..", float(k.max()), "alphabet", mn, "..", mx)
    assert float(k.min()) >= mn and float(k.max()) <= mx
    assert not torch.equal(dec._anchor_feat.data[500:1000, 12:24], want["_anchor_feat"][500:1000, 12:24])   # (the cut did reach the decoder)


# ---------------------------------------------------------------- accuracy of the context and of a chained stage
def _m64(torch, seq):
    m = torch.nn.Sequential(*[torch.nn.Linear(l.in_features, l.out_features) if isinstance(l, torch.nn.Linear) else torch.nn.ReLU() for l in seq])
    m.load_state_dict(seq.state_dict())
    return m.double().cuda()


def test_context_and_chained_stage_close_to_float64(torch_cuda, full_case):
    torch = torch_cuda
    from gauspcc_amd import cat_codec

    c = full_case
    enc = c["enc"]
    anchor, src, _, _, want = c["exp"]
    net = enc.feature_net.attribute_net
    K = enc.n_offsets
    with torch.no_grad():
        x = _grid_features(torch, enc, anchor)
        got = cat_codec._context(enc, anchor)
        t32 = net.net(net.feature_out(x))
        head = torch.nn.Sequential(net.feature_out[0], net.net[0], net.net[1])
        w64 = _m64(torch, head)(x.double())
        assert got.shape == (1037, 175)
        bad = []
        names = ("scale", "mean", "mean_scaling", "scale_scaling", "mean_offsets", "scale_offsets", "Q_adj")
        for name, g_, t_, w_ in zip(names, *(torch.split(t, [F, F, 6, 6, 3 * K, 3 * K, 3], dim=-1) for t in (got, t32, w64))):
            e_dev, e_t32 = float((g_.double() - w_).abs().max()), float((t_.double() - w_).abs().max())
            print(f"{name}: e_dev {e_dev:.3e}  e_t32 {e_t32:.3e}")
            if not e_dev <= FACTOR * e_t32:
                bad.append((name, e_dev, e_t32))
        # one chained stage: feat3 reads the 37 decoded channels before it
        st = cat_codec.stage_table(enc)[3]
        assert st["name"] == "feat3" and st["dep_ch"] == 37
        xq = want["_anchor_feat"]
        mean, scale = cat_codec._stage_params(st, got, xq)
        m = st["mlp"]
        d32, d64 = m(xq[:, :37]), _m64(torch, m)(xq[:, :37].double())
        ch = st["ch"]
        cols = lambda t, c0: t[:, c0:c0 + ch]                                                         # noqa: E731
        ref = dict(mean=(cols(t32, st["mean_col"]) + d32[:, :ch], cols(w64, st["mean_col"]) + d64[:, :ch]),
                   scale=(torch.clamp(cols(t32, st["scale_col"]) + d32[:, ch:], min=1e-9), torch.clamp(cols(w64, st["scale_col"]) + d64[:, ch:], min=1e-9)))
        for name, g_ in (("mean", mean), ("scale", scale)):
            t_, w_ = ref[name]
            e_dev, e_t32 = float((g_.double() - w_).abs().max()), float((t_.double() - w_).abs().max())      # by value: a zero's sign may differ
            print(f"feat3 {name}: e_dev {e_dev:.3e}  e_t32 {e_t32:.3e}")
            if not e_dev <= FACTOR * e_t32:
                bad.append(("feat3 " + name, e_dev, e_t32))
    assert not bad, bad


# ---------------------------------------------------------------- estimate_final_bits
def test_estimate_final_bits_matches_torch_restatement(torch_cuda, full_case):
    """The numbers of the returned string against (:1056-1137) restated with the model's own torch modules.  Every number is round(bits / 2^23, 4), a
    float32 sum of n terms: two correct evaluations differ by at most n 2^-24 of the sum (summation order) plus one unit of the rounding, 1e-4."""
    torch = torch_cuda
    from gauspcc_amd import cat_codec

    enc = full_case["enc"]
    K = enc.n_offsets
    log = cat_codec.estimate_final_bits(enc, None)
    assert log.startswith("\nEstimated sizes in MB: anchor ")
    nums = dict(re.findall(r"(anchor|total feat|scaling|offsets|masks|MLPs|Triplane_f|Total) ([-0-9.e]+)", log))
    assert len(nums) == 8, log
    MB = 8 * 1024 * 1024

    def bits(x, mean, scale, Q):                                                        # Entropy_gaussian.forward (utils/entropy_models.py:34-51)
        Q = torch.clamp(Q, min=1e-9)
        xm = x.mean()
        x = torch.clamp(x, min=xm - 15_000 * Q, max=xm + 15_000 * Q)
        m1 = torch.distributions.normal.Normal(mean, torch.clamp(scale, min=1e-9))
        return -torch.log2(torch.clamp(torch.abs(m1.cdf(x + 0.5 * Q) - m1.cdf(x - 0.5 * Q)), min=1e-6))

    def ste(x, Q):
        m = x.mean()
        return torch.round(torch.clamp(x, min=m - 15_000 * Q, max=m + 15_000 * Q) / Q) * Q

    with torch.no_grad():
        keep = enc.get_mask_anchor(None)
        _anchor, _feat, _offs, _scaling, _mask = enc.get_anchor[keep], enc._anchor_feat[keep], enc._offset[keep], enc.get_scaling[keep], enc.get_mask(None)[keep]
        ctx, feat_rate = enc.feature_net(_anchor, itr=-1)
        scales, means, mean_s, scale_s, mean_o, scale_o, qf, qs, qo = torch.split(ctx, [F, F, 6, 6, 3 * K, 3 * K, 1, 1, 1], dim=-1)
        groups = enc.chcm_slices_list
        lm, ls = torch.split(means, groups, dim=-1), torch.split(scales, groups, dim=-1)
        Qf, Qs, Qo = 1 * (1.1 + torch.tanh(qf)), 0.001 * (1.1 + torch.tanh(qs)), 0.2 * (1.1 + torch.tanh(qo))
        fq = ste(_feat, Qf)
        fl = torch.split(fq, groups, dim=-1)
        bit_feat, dec_feat = [], None
        for i in range(len(groups)):
            mean, scale = lm[i], ls[i]
            if i:
                d = enc.mlp_chcm_list[i - 1](dec_feat)
                mean, scale = mean + d[:, :groups[i]], scale + d[:, groups[i]:]
            bit_feat.append(torch.sum(bits(fl[i], mean, scale, Qf)).item())
            dec_feat = fl[i] if dec_feat is None else torch.cat([dec_feat, fl[i]], dim=-1)
        d = enc.mlp_chcm_scaling(dec_feat)
        mean_s, scale_s = mean_s + d[:, :6], scale_s + d[:, 6:]
        d = enc.mlp_chcm_offsets(dec_feat)
        mean_o, scale_o = mean_o + d[:, :3 * K], scale_o + d[:, 3 * K:]
        b_s = torch.sum(bits(ste(_scaling, Qs), mean_s, scale_s, Qs)).item()
        offs = ste(_offs, Qo.unsqueeze(1)).view(-1, 3 * K)
        b_o = torch.sum(bits(offs, mean_o, scale_o, Qo) * _mask.repeat(1, 1, 3).view(-1, 3 * K)).item()
        n = _anchor.shape[0]
        pos = torch.sum(_mask)
        Pg = torch.clamp(pos / _mask.numel(), min=1e-6, max=1 - 1e-6)
        b_m = (pos * (-torch.log2(Pg)) + (_mask.numel() - pos) * (-torch.log2(1 - Pg)) + 32).item()
        mlp = enc.get_mlp_size()[0]
        tri = (feat_rate / MB).item()
        b_a = n * 3 * 16
    want = {"anchor": (b_a / MB, 1), "total feat": (sum(bit_feat) / MB, n * F), "scaling": (b_s / MB, n * 6), "offsets": (b_o / MB, n * 3 * K),
            "masks": (b_m / MB, 1), "MLPs": (mlp / MB, 1), "Triplane_f": (tri, sum(p.numel() for lv in enc.feature_net.attribute_net.grid.grids for p in lv)),
            "Total": ((b_a + sum(bit_feat) + b_s + b_o + b_m + mlp) / MB + tri, n * (F + 6 + 3 * K))}
    bad = []
    for name, (val, count) in want.items():
        tol = 1e-4 + count * 2.0 ** -24 * abs(val)
        got = float(nums[name])
        print(f"{name}: got {got}  torch {val:.6f}  tol {tol:.2e}")
        if not abs(got - val) <= tol:
            bad.append((name, got, val, tol))
    assert not bad, bad
