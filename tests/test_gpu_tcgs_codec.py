"""GPU tests of TC-GS's attribute loop (gauspcc_amd.tcgs_codec): conduct_encoding -> conduct_decoding on the slice of GaussianModel the reference's
methods touch (src/gs_compress/TC-GS/scene/gaussian_model.py:1135-1465; gauspcc_amd.synth.SyntheticGaussianModelTC).

The round trip is EXACT: the expectation is computed outside tcgs_codec -- per 1 000-anchor slice the sampler in the reference's
`anchor.unsqueeze(1).repeat(1, K, 1)` form, the Linear-ReLU-Linear chain by the ORACLE on the host (gshac_mlp2 == orc.mlp2 bit for bit, checked
below at TC-GS's own layer sizes), the STE with the global means -- and compared with torch.equal.  Separately the context itself is held to a
float64 evaluation by the project's usual rule: no further from it than 4 x what torch's float32 nn.Sequential is."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 4
FACTOR = 4.0
FILES_FIXED = {"xyz_pcc.bin", "masks.b"}            # ste_binary is False (TC-GS's default): no hash.b


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch


def _model(n, seed):
    from gauspcc_amd.synth import SyntheticGaussianModelTC

    return SyntheticGaussianModelTC(n, seed=seed, resolution=64, device="cuda:0")


def _roundtrip(torch, tmp, n, seed):
    """conduct_encoding -> conduct_decoding into a fresh model that shares only the networks and the bounds: (enc, dec, patched, N, anchor, src)"""
    from gauspcc_amd import tcgs_codec

    enc = _model(n, seed)
    assert enc.ste_binary is False and enc.get_encoding_params() is enc.triplane.get_encode()
    patched, log = tcgs_codec.conduct_encoding(enc, str(tmp), ckpt_path="synthetic")
    assert len(patched) == 12
    n_full, N, mb, infos, *bounds, prob_hash, prob_masks = patched
    steps = -(-N // mb)
    assert mb == 1000 and n_full == enc._anchor.shape[0] and N == int(enc.get_mask_anchor.sum()) and infos == [None] * steps
    assert len(bounds) == 6 and prob_hash == 0 and 0.0 < prob_masks <= 1.0
    for lst in bounds:                                   # min_feat, max_feat, min_scaling, max_scaling, min_offsets, max_offsets: one 0-d tensor per slice
        assert isinstance(lst, list) and len(lst) == steps and all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in lst)
    assert set(os.listdir(tmp)) == FILES_FIXED | {f"{a}_{s}.b" for a in ("feat", "scaling", "offsets") for s in range(steps)}
    assert log.startswith("\nEncoded sizes in MB: anchor ") and "triplane 0.0, masks " in log and ", EncTime " in log

    dec = _model(64, seed + 50)
    dec.triplane, dec.mlp_triplane = enc.triplane, enc.mlp_triplane
    dec.x_bound_min, dec.x_bound_max = enc.x_bound_min, enc.x_bound_max
    dec._anchor_feat = torch.zeros(1, enc.feat_dim, device="cuda")
    msg = tcgs_codec.conduct_decoding(dec, str(tmp), patched, ckpt_path="synthetic")
    assert msg.startswith("\nDecTime") and dec.decoded_version is True

    # the decoder's anchors in the reference's order (calculate_morton_order, pcc_utils.py:12-22) and the encoder-side attributes in that order
    keep = enc.get_mask_anchor
    a_int = torch.round(enc.get_anchor[keep] / enc.voxel_size)
    key = (a_int - a_int.min(dim=0, keepdim=True).values).to(torch.int64)
    M = key.max() + 1
    order = torch.argsort(key[:, 0] + key[:, 1] * M + key[:, 2] * M * M)
    anchor = a_int[order] * enc.voxel_size
    assert torch.equal(dec._anchor.data, anchor)
    src = dict(feat=enc._anchor_feat[keep][order], scaling=enc.get_scaling[keep][order], mask=enc.get_mask[keep][order], offs=enc._offset[keep][order])
    assert torch.equal(dec._mask.data, src["mask"])
    for name, shape in (("_anchor_feat", (N, enc.feat_dim)), ("_scaling", (N, 6)), ("_offset", (N, enc.n_offsets, 3)), ("_mask", (N, enc.n_offsets, 1))):
        assert isinstance(getattr(dec, name), torch.nn.Parameter) and tuple(getattr(dec, name).shape) == shape
    return enc, dec, patched, N, anchor, src


@pytest.fixture(scope="module")
def three_slices(torch_cuda, tmp_path_factory):
    """2 300 anchors: three slices, the last partial.  Shared by the exact comparison, the context check and the second encode."""
    tmp = tmp_path_factory.mktemp("tcgs_2300")
    return (tmp,) + _roundtrip(torch_cuda, tmp, 2300, 5)


def _ste(torch, x, Q, mean):
    """STE_multistep.forward (TC-GS/utils/encodings.py:318-330) with the GLOBAL mean, as the reference's loop calls it"""
    x = torch.clamp(x, min=(mean - 15_000 * Q), max=(mean + 15_000 * Q))
    return torch.round(x / Q) * Q


def _split(torch, enc, out):
    """(:1222-1236) the nine outputs of mlp_triplane -> mean / scale per attribute and the three step sizes, (rows, channels) each"""
    fd, no = enc.feat_dim, enc.n_offsets
    mean, scale, mean_s, scale_s, mean_o, scale_o, qf, qs, qo = torch.split(out, [fd, fd, 6, 6, 3 * no, 3 * no, 1, 1, 1], dim=-1)
    Qf = 1 * (1 + torch.tanh(qf.contiguous().repeat(1, fd)))
    Qs = 0.001 * (1 + torch.tanh(qs.contiguous().repeat(1, 6)))
    Qo = 0.2 * (1 + torch.tanh(qo.contiguous().repeat(1, 3 * no)))
    return dict(mean=torch.cat([mean, mean_s, mean_o], dim=1), scale=torch.clamp(torch.cat([scale, scale_s, scale_o], dim=1), min=1e-9), Qf=Qf, Qs=Qs, Qo=Qo)


def _features(torch, enc, rows):
    """(:1215-1219) the sampler in the reference's form, K identical samples per anchor, and the anchor behind them"""
    ctx = enc.triplane(rows.unsqueeze(1).repeat(1, K, 1), enc.x_bound_max, enc.x_bound_min)
    return torch.cat([ctx, rows], dim=1)


def _check_exact(torch, orc, enc, dec, N, anchor, src, mb=1000):
    m = enc.get_tri_mlp
    w1, b1, w2, b2 = (t.detach().cpu().numpy() for t in (m[0].weight, m[0].bias, m[2].weight, m[2].bias))
    no = enc.n_offsets
    with torch.no_grad():
        for s0 in range(0, N, mb):
            sl = slice(s0, min(s0 + mb, N))
            out = torch.tensor(orc.mlp2(_features(torch, enc, anchor[sl]).cpu().numpy(), w1, b1, w2, b2), device="cuda")
            c = _split(torch, enc, out)
            m3 = src["mask"][sl].repeat(1, 1, 3).view(-1, 3 * no)
            want = {"_anchor_feat": _ste(torch, src["feat"][sl], c["Qf"], src["feat"].mean()),
                    "_scaling": _ste(torch, src["scaling"][sl], c["Qs"], src["scaling"].mean()),
                    "_offset": _ste(torch, src["offs"][sl].reshape(-1, 3 * no), c["Qo"], src["offs"].mean()) * m3}      # offsets[~mask] = 0 (:1262, :1415)
            for name, w in want.items():
                got = getattr(dec, name).data[sl].reshape(w.shape)
                assert torch.equal(got, w), (name, sl, int((got != w).sum()), float((got - w).abs().max()))


def test_roundtrip_three_slices_exact(torch_cuda, orc, three_slices):
    tmp, enc, dec, patched, N, anchor, src = three_slices
    assert -(-N // 1000) == 3 and N % 1000 != 0
    _check_exact(torch_cuda, orc, enc, dec, N, anchor, src)


@pytest.mark.parametrize("n", [1000, 700])
def test_roundtrip_single_slice_exact(torch_cuda, orc, tmp_path, n, monkeypatch):
    from gauspcc_amd import tcgs_codec

    if n == 700:                                         # the context in several passes of 256 anchors: rows are independent, the same bits
        monkeypatch.setattr(tcgs_codec, "_CONTEXT_ROWS", 256)
    enc, dec, patched, N, anchor, src = _roundtrip(torch_cuda, tmp_path, n, 7 + n)
    assert N <= 1000 and (n != 1000 or N == 1000)
    _check_exact(torch_cuda, orc, enc, dec, N, anchor, src)


def test_second_encode_writes_identical_files(torch_cuda, three_slices, tmp_path):
    from gauspcc_amd import tcgs_codec

    tmp, enc = three_slices[0], three_slices[1]
    patched2, _ = tcgs_codec.conduct_encoding(enc, str(tmp_path), ckpt_path="synthetic")
    assert sorted(os.listdir(tmp_path)) == sorted(os.listdir(tmp))
    for f in os.listdir(tmp):
        assert open(tmp / f, "rb").read() == open(tmp_path / f, "rb").read(), f
    for a, b in zip(three_slices[3][4:10], patched2[4:10]):
        assert all(torch_cuda.equal(u, v) for u, v in zip(a, b))


def test_context_close_to_float64(torch_cuda, three_slices):
    """mean, scale and the three step sizes as tcgs_codec computes them (one pass over all anchors, the sampler's repeat form, gshac_mlp2) against
    mlp_triplane evaluated in float64 on the same features: no further from it than 4 x what torch's float32 nn.Sequential is."""
    torch = torch_cuda
    from gauspcc_amd import tcgs_codec

    tmp, enc, dec, patched, N, anchor, src = three_slices
    fd, no = enc.feat_dim, enc.n_offsets
    with torch.no_grad():
        c = tcgs_codec._context(enc, anchor)
        got = dict(mean=torch.cat([c["mean"].view(N, fd), c["mean_scaling"].view(N, 6), c["mean_offsets"].view(N, 3 * no)], dim=1),
                   scale=torch.cat([c["scale"].view(N, fd), c["scale_scaling"].view(N, 6), c["scale_offsets"].view(N, 3 * no)], dim=1),
                   Qf=c["Q_feat"].view(N, fd), Qs=c["Q_scaling"].view(N, 6), Qo=c["Q_offsets"].view(N, 3 * no))
        x = _features(torch, enc, anchor)
        t32 = _split(torch, enc, enc.get_tri_mlp(x))
        m64 = torch.nn.Sequential(*[torch.nn.Linear(l.in_features, l.out_features) if isinstance(l, torch.nn.Linear) else torch.nn.ReLU() for l in enc.get_tri_mlp])
        m64.load_state_dict(enc.get_tri_mlp.state_dict())
        want = _split(torch, enc, m64.double().cuda()(x.double()))
    bad = []
    for name in ("mean", "scale", "Qf", "Qs", "Qo"):
        e_dev = float((got[name].double() - want[name]).abs().max())
        e_t32 = float((t32[name].double() - want[name]).abs().max())
        print(f"{name}: e_dev {e_dev:.3e}  e_t32 {e_t32:.3e}")
        if not e_dev <= FACTOR * e_t32:
            bad.append((name, e_dev, e_t32))
    assert not bad, bad


@pytest.mark.parametrize("din,dh,dout", [(603, 100, 175), (600, 100, 175), (100, 64, 20)])
def test_mlp2_at_tcgs_sizes_matches_oracle_bit_for_bit(torch_cuda, orc, din, dh, dout):
    """TC-GS's mlp_triplane (K * 3 * 50 + 3 = 603 inputs), the same without the anchor columns and a narrower layer inside the class of the wide
    matrix-pipe kernel (k_mlp2_mfma_wide: din <= 608, dh <= 100, dout <= 176): the exact comparison above rests on this."""
    torch = torch_cuda
    from gauspcc_amd import hac_codec

    rng = np.random.RandomState(din)
    w1 = (rng.randn(dh, din) / np.sqrt(din)).astype(np.float32); b1 = rng.randn(dh).astype(np.float32) * 0.1
    w2 = (rng.randn(dout, dh) / np.sqrt(dh)).astype(np.float32); b2 = rng.randn(dout).astype(np.float32) * 0.1
    for n in (1, 15, 16, 17, 1000):
        x = rng.randn(n, din).astype(np.float32)
        y = hac_codec.mlp2(*(torch.tensor(a).cuda() for a in (x, w1, b1, w2, b2))).cpu().numpy()
        assert np.array_equal(y, orc.mlp2(x, w1, b1, w2, b2)), n
