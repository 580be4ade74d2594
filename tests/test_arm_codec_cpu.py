"""The tri-plane latent bitstream without a GPU: the header parser, and the size bound of tests/test_gpu_arm_codec.py on the restatement
of tests/arm_codec_ref.py (float64 rows, the library's host coder) -- the inputs and the bound are consistent before any device runs."""
import re
import os
import struct

import numpy as np
import pytest

from gauspcc_amd import arm_codec as AC
from tests import arm_codec_ref as R

DIMS = [12, 16, 16, 16, 16, 2]
SIZE_SHAPE, SIZE_SEED = (8, 64, 96), 11


def _stream(C=2, H=3, W=9, S=4, A=5, counts=None, payload=None):
    K = -(-W // S)
    counts = [1] * (C * K) if counts is None else counts
    return R.build_header(C, H, W, A, S, DIMS, counts) + (b"\x00" * sum(counts) if payload is None else payload)


def test_parse_header_accepts_the_restatement():
    data = _stream(counts=[3, 0, 2, 1, 1, 0])
    h = AC.parse_header(data)
    assert (h["C"], h["H"], h["W"], h["S"], h["A"], h["quant"]) == (2, 3, 9, 4, 5, 16)
    assert h["dims"] == DIMS and h["counts"] == [3, 0, 2, 1, 1, 0]
    assert h["header_bytes"] == len(data) - 7
    assert h["offsets"] == [h["header_bytes"] + o for o in (0, 3, 3, 5, 6, 7)]
    assert AC.build_header(2, 3, 9, 5, 4, DIMS, h["counts"]) == data[:h["header_bytes"]]


@pytest.mark.parametrize("what", ["magic", "version", "quant", "short_fixed", "short_dims", "short_counts", "sum_low", "sum_high",
                                   "strip", "alphabet", "empty_c", "empty_h", "empty_w", "chunks"])
def test_parse_header_rejects(what):
    good = bytearray(_stream())
    AC.parse_header(bytes(good))
    bad = bytearray(good)
    if what == "magic":
        bad[0:4] = b"GSAX"
    elif what == "version":
        struct.pack_into("<H", bad, 4, 2)
    elif what == "quant":
        struct.pack_into("<H", bad, 6, 8)
    elif what == "short_fixed":
        bad = bad[:20]
    elif what == "short_dims":
        bad = bad[:30]
    elif what == "short_counts":
        bad = bad[:AC.parse_header(bytes(good))["header_bytes"] - 3]
    elif what == "sum_low":
        bad = bad + b"\x00"
    elif what == "sum_high":
        bad = bad[:-1]
    elif what == "strip":
        bad = bytearray(_stream(S=3, counts=[1] * 6))
    elif what == "alphabet":
        bad = bytearray(_stream(A=1025))
    elif what == "empty_c":
        struct.pack_into("<I", bad, 8, 0)
    elif what == "empty_h":
        struct.pack_into("<I", bad, 12, 0)
    elif what == "empty_w":
        struct.pack_into("<I", bad, 16, 0)
    elif what == "chunks":
        bad = bytearray(_stream(counts=[1] * 5))
    with pytest.raises(ValueError):
        AC.parse_header(bytes(bad))


def test_default_strip_rule():
    for W in (1, 5, 37, 96, 334, 512, 513, 4096):
        S = AC.default_strip(W)
        assert S % 8 == 0 and -(-W // S) <= 64
        assert S == 8 or -(-W // (S - 8)) > 64


def test_chunk_order_covers_the_grid_once():
    C, H, W, S = 3, 9, 37, 4
    order = R.chunk_order(C, H, W, S)
    assert len(order) == C * 10 and len(order[9]) == H * 1
    assert sorted(np.concatenate(order).tolist()) == list(range(C * H * W))
    assert order[1][:5].tolist() == [4, 5, 6, 7, W + 4]


def test_size_bound_holds_for_the_restatement():
    """smooth latents under the [16, 16, 16, 16] ARM, parameters from ArmMLP.forward on the CPU, rows in float64, the host coder: the
    stream decodes on the host and meets the bound the device test asserts"""
    C, H, W = SIZE_SHAPE
    y = R.smooth_latent(C, H, W, SIZE_SEED)
    arm = R.make_arm([16, 16, 16, 16], 5, spread=0.15)
    mu, s = R.params_cpu(y, arm)
    S = AC.default_strip(W)
    data = R.encode_ref(y, mu, s, S, DIMS)
    h = AC.parse_header(data)
    A = R.ac_max_val(y)
    assert h["A"] == A and len(h["counts"]) == C * -(-W // S)
    mu_q, s_q = R.quantise(mu, s)
    ideal = R.ideal_bits(y, mu_q, s_q)
    bound = R.size_bound_bits(ideal, y.size, A, len(h["counts"]), h["header_bytes"])
    print(f"size (host restatement): {8 * len(data)} bits, ideal {ideal:.0f}, bound {bound:.0f}, payload excess "
          f"{100 * (8 * sum(h['counts']) / ideal - 1):.3f} %")
    assert 8 * len(data) <= bound
    # and the first chunk decodes back on the host
    rows = (R.rows_ref(mu_q, s_q, A) & 0xFFFF).astype(np.uint16)
    ix = R.chunk_order(C, H, W, S)[0]
    got = R.host_decode(data[h["offsets"][0]:h["offsets"][0] + h["counts"][0]], rows[ix])
    assert np.array_equal(got.astype(np.float32) - A, y.reshape(-1)[ix])


def test_entry_points_are_declared_and_exported():
    from gauspcc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gauspcc.h")).read()
    names = {"gsac_arm_encode", "gsac_arm_decode", "gsac_arm_cdf_rows"}
    assert names <= set(re.findall(r"GPCC_API int (\w+)\(", header)) and names <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert len(L.gsac_arm_encode.argtypes) == 16 and len(L.gsac_arm_decode.argtypes) == 16 and len(L.gsac_arm_cdf_rows.argtypes) == 7
