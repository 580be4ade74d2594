"""gsac_arm_encode / gsac_arm_decode / gsac_arm_cdf_rows (gauspcc_amd.arm_codec) on the device: the bitstream of CAT-3DGS's tri-plane
latents.  Lossless round trips over every path of the decoder (one lane, narrow last strip, more than one wave, both kernels, several
levels, the alphabet's edges, scales on both clamp ends, probabilities on the one-count floor), the integer rows against float64,
every chunk's bytes against the library's host coder, the stream's size against the ideal code length, and the file-level calls."""
import functools
import os

import numpy as np
import pytest
import torch

from gauspcc_amd import _lib, arm_codec as AC, runtime
from gauspcc_amd.arm import arm_rate
from tests import arm_codec_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [((1, 1, 1), None), ((2, 1, 5), None), ((2, 5, 1), None), ((3, 5, 2), None), ((3, 9, 37), 4), ((1, 4, 260), 4), ((2, 40, 24), None),
          ((2, 6, 334), None), ((8, 64, 96), None), ((1, 2, 1030), 4)]
ARMS = {"spec": dict(layers=[16, 16, 16, 16], seed=1), "any": dict(layers=[8, 24], seed=2), "res": dict(layers=[12, 12], seed=3)}


@functools.lru_cache(maxsize=None)
def _arm(name):
    if name in ARMS:
        return R.make_arm(**ARMS[name]).to(DEV)
    if name == "wide":        # ls pinned below the clamp: s = exp(5) = 148.4
        return R.make_arm([16, 16, 16, 16], 4, ls_pin=-20.0).to(DEV)
    if name == "narrow":      # ls pinned above the clamp: s = 1e-3, quantised to 1 / 16
        return R.make_arm([8, 24], 5, ls_pin=20.0).to(DEV)
    if name == "far":         # mu tens of symbols from the latents, a narrow scale: every latent sits on the one-count floor
        return R.make_arm([16, 16, 16, 16], 6, mu_bias=40.0, ls_pin=2.0).to(DEV)
    if name == "size":
        return R.make_arm([16, 16, 16, 16], 5, spread=0.15).to(DEV)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _latent(shape, seed=0):
    C, H, W = shape
    return torch.as_tensor(R.smooth_latent(C, H, W, 100 + seed + C + 7 * H + 13 * W)).to(DEV).reshape(1, C, H, W)


def _round_trip(y, arm, strip=None):
    data = AC.encode_latents(y, arm, strip)
    assert AC.encode_latents(y, arm, strip) == data
    back = AC.decode_latents(data, arm)
    assert back.shape == (1,) + tuple(y.shape[-3:]) and back.dtype == torch.float32 and back.is_cuda
    assert torch.equal(back.reshape(y.shape), y)
    return data


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("shape,strip", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, _ in SHAPES])
def test_round_trip(shape, strip, arm):
    data = _round_trip(_latent(shape), _arm(arm), strip)
    h = AC.parse_header(data)
    assert (h["C"], h["H"], h["W"]) == shape and h["S"] == (strip or AC.default_strip(shape[2]))
    assert h["A"] == R.ac_max_val(_latent(shape).cpu().numpy())


@pytest.mark.parametrize("arm", ["wide", "narrow", "far"])
@pytest.mark.parametrize("shape,strip", [((3, 9, 37), 4), ((2, 40, 24), None)], ids=["3x9x37", "2x40x24"])
def test_round_trip_extreme_models(shape, strip, arm):
    y = _latent(shape)
    _, _, scale = arm_rate(y, _arm(arm), reduce="none", return_params=True)
    s = scale[0]
    if arm == "wide":
        assert float(s.min()) > 140.0
    if arm == "narrow":
        assert float(s.max()) < 2e-3
    _round_trip(y, _arm(arm), strip)


@pytest.mark.parametrize("arm", ["spec", "any"])
def test_round_trip_two_levels_in_one_call(arm):
    ys = [_latent((3, 8, 12)), _latent((3, 16, 24))]
    datas = AC.encode_levels(ys, _arm(arm))
    assert datas == AC.encode_levels(ys, _arm(arm))
    assert datas == [AC.encode_latents(y, _arm(arm)) for y in ys]      # a level's stream does not depend on its company
    for y, back in zip(ys, AC.decode_levels(datas, _arm(arm))):
        assert torch.equal(back, y)


def test_alphabet_edges():
    arm = _arm("spec")
    zero = torch.zeros(1, 2, 6, 10, device=DEV)
    assert AC.parse_header(_round_trip(zero, arm))["A"] == 2
    edge = _latent((2, 6, 10)).clone()
    edge[0, 0, 2, 3], edge[0, 1, 4, 7] = 1022.0, -1022.0
    assert AC.parse_header(_round_trip(edge, arm))["A"] == 1024
    over = edge.clone()
    over[0, 0, 0, 0] = 1023.0
    with pytest.raises(ValueError):
        AC.encode_latents(over, arm)
    frac = zero.clone()
    frac[0, 1, 3, 3] = 0.5
    with pytest.raises(ValueError):
        AC.encode_latents(frac, arm)


def test_checks():
    arm, y = _arm("spec"), _latent((3, 5, 2))
    with pytest.raises(ValueError):
        AC.encode_latents(y, arm, strip=3)
    with pytest.raises(TypeError):
        AC.encode_latents(y.double(), arm)
    with pytest.raises(RuntimeError):
        AC.encode_latents(y.cpu(), arm)
    with pytest.raises(ValueError):
        AC.decode_latents(AC.encode_latents(y, arm), _arm("any"))          # another ARM's widths
    nan_arm = R.make_arm([8, 24], 9).to(DEV)
    with torch.no_grad():
        nan_arm.linears()[-1].b[0] = float("nan")
    with pytest.raises(ValueError):
        AC.encode_latents(y, nan_arm)                                      # a mu that is not finite: no stream


def _device_rows(mu_q, s_q, A):
    n = mu_q.numel()
    rows = torch.empty((n, 2 * A + 2), dtype=torch.int16, device=DEV)
    _lib.check(_lib.lib().gsac_arm_cdf_rows(runtime.context(DEV), mu_q.data_ptr(), s_q.data_ptr(), n, A, rows.data_ptr(), runtime.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(np.uint16)


def _quantised(ys, arm):
    """(mu_q, s_q) per level, flat, float32 on the device: arm_rate's maps quantised by the format's rule"""
    _, mu, scale = arm_rate(ys, arm, reduce="none", return_params=True)
    return [(torch.round(m.reshape(-1) * 16) / 16, torch.clamp(torch.round(s.reshape(-1) * 16) / 16, min=1 / 16)) for m, s in zip(mu, scale)]


@pytest.mark.parametrize("arm,A", [("spec", 9), ("any", 2), ("wide", 40), ("narrow", 5), ("far", 1024)])
def test_rows_against_float64(arm, A):
    """every entry within one count of rint(F64 (65536 - L)) + j on the same float32 (mu_q, s_q), at most 5 % differ (the float32
    evaluation is within ~0.011 count of float64: only near-ties of rint move), rows strictly increasing"""
    y = _latent((3, 9, 37))
    (mu_q, s_q), = _quantised([y], _arm(arm))
    if A == 1024:
        mu_q, s_q = mu_q[:64].contiguous(), s_q[:64].contiguous()
    L = 2 * A + 1
    got = _device_rows(mu_q, s_q, A).astype(np.int64)
    want = R.rows_ref(mu_q.cpu().numpy(), s_q.cpu().numpy(), A)
    assert np.all(got[:, L] == 0) and np.all(got[:, 0] == 0)
    got[:, L] = 65536
    diff = np.abs(got - want)
    print(f"rows {arm} A={A}: max |diff| {diff.max()}, differing {100 * (diff > 0).mean():.3f} %")
    assert diff.max() <= 1
    assert (diff > 0).mean() <= 0.05
    assert np.all(np.diff(got, axis=1) > 0)


@pytest.mark.parametrize("case", ["strips", "levels"])
def test_bytes_equal_the_host_coder(case):
    arm = _arm("spec")
    ys, strips = ([_latent((3, 9, 37))], [4]) if case == "strips" else ([_latent((3, 8, 12)), _latent((3, 16, 24))], [None, None])
    datas = AC.encode_levels(ys, arm, strips)
    for y, data, (mu_q, s_q) in zip(ys, datas, _quantised(ys, arm)):
        h = AC.parse_header(data)
        rows = _device_rows(mu_q, s_q, h["A"])
        want = R.chunk_payloads(y[0].cpu().numpy(), rows, h["S"])
        assert len(want) == len(h["counts"])
        for k, (w, off, cnt) in enumerate(zip(want, h["offsets"], h["counts"])):
            assert data[off:off + cnt] == w, (case, k)


def test_size():
    """8 len(data) <= 1.01 ideal + n 2 L / 65536 + 96 n_chunks + 8 header_bytes (tests/arm_codec_ref.py: size_bound_bits)"""
    y, arm = _latent((8, 64, 96), seed=0), _arm("size")
    data = _round_trip(y, arm)
    h = AC.parse_header(data)
    (mu_q, s_q), = _quantised([y], arm)
    ideal = R.ideal_bits(y.cpu().numpy(), mu_q.cpu().numpy(), s_q.cpu().numpy())
    bound = R.size_bound_bits(ideal, y.numel(), h["A"], len(h["counts"]), h["header_bytes"])
    print(f"size: {8 * len(data)} bits, ideal {ideal:.0f}, bound {bound:.0f}, payload excess {100 * (8 * sum(h['counts']) / ideal - 1):.3f} %")
    assert 8 * len(data) <= bound


class _Grid:
    def __init__(self):
        g = torch.Generator().manual_seed(7)
        self.grids = [[(torch.randn(1, 4, H, W, generator=g) * 0.4).to(DEV) for _ in range(3)] for H, W in ((6, 10), (12, 20))]
        self.arm, self.arm2, self.arm3 = (R.make_arm(layers, 20 + i).to(DEV) for i, layers in enumerate(([16, 16, 16, 16], [8, 24], [12, 12])))


def test_files(tmp_path):
    grid = _Grid()
    info, real_rate_byte = AC.encode_triplane(grid, str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f"{p}_bitstream_{j}.bin" for p in ("xy", "yz", "zx") for j in range(2))
    assert real_rate_byte == sum(os.path.getsize(tmp_path / n) for n in names)
    assert info == [[int(torch.ceil(torch.round(grid.grids[j][p] * 16).abs().max())) + 2 for j in range(2)] for p in range(3)]
    planes = AC.decode_triplane(grid, str(tmp_path), info)
    assert len(planes) == 2 and all(isinstance(p, torch.nn.ParameterList) and len(p) == 3 for p in planes)
    for j in range(2):
        for p in range(3):
            assert planes[j][p].is_cuda and planes[j][p].shape == grid.grids[j][p].shape
            assert torch.equal(planes[j][p].detach(), torch.round(grid.grids[j][p] * 16) / 16)
