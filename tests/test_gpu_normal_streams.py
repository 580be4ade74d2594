"""The TC-GS / CAT-3DGS stream coder on the device (gsac_normal_cdf_rows, gsac_encode_normal_streams, gsac_decode_normal_streams; gauspcc_amd/csrc/
attributes.hip): one carry-less torchac stream per slice, CDF entries of `Normal(mean, scale).cdf((samples - 0.5) * Q)` evaluated inside the coder.

What is held to what:
  rows     strictly increasing; against the torch-built table integerised on the same device (torchac_encodings._int_rows) no entry differs by
           more than 1 -- a few ulp of a float32 CDF times at most 65 535 cannot move rint further; the share that differs is printed, not asserted;
  bytes    every stream equals torchac's coder (gsac_host_encode_u16) on the slice's rows from gsac_normal_cdf_rows, and gsac_host_decode_u16 on
           those rows decodes it;
  decode   gsac_decode_normal_streams returns round(x / Q) * Q exactly, over slice lengths 0, 1, 63, 64, 65, 2 049 and 50 000 in one call and over
           alphabets that take every tier of the decoder (16-wide window, 64-wide window, binary search).
"""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RANGE = -3                                                     # GPCC_ERR_RANGE (include/gauspcc.h)
CLAMP = 1e-9                                                   # TC-GS clamps its scales there (scene/gaussian_model.py:1231-1233)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch


class Slices:
    """Slices of one call: float32 arrays x, mean, scale, q and the slice starts."""

    def __init__(self, parts):
        self.start = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)
        cat = lambda k: np.concatenate([p[k] for p in parts]).astype(np.float32)
        self.x, self.mean, self.scale, self.q = cat(0), cat(1), cat(2), cat(3)

    def dev(self, torch):
        return tuple(torch.tensor(a).cuda() for a in (self.x, self.mean, self.scale, self.q))


def _small(rng, n, lo=-12, hi=12):
    """integer levels lo .. hi at Q = 1: alphabets of at most hi - lo + 2 entries"""
    mean = rng.randn(n) * 2.0
    scale = rng.rand(n) * 2.0 + 0.3
    x = np.clip(np.rint(mean + scale * rng.randn(n)), lo, hi)
    if n >= 2:
        x[0], x[1] = lo, hi
    return x, mean, scale, np.ones(n)


def lengths_case():
    rng = np.random.RandomState(5)
    return Slices([_small(rng, n) for n in (0, 1, 63, 64, 65, 2049, 50_000)])


def alphabets_case():
    """One slice per decoder tier; scales at the clamp and means outside [min, max] * Q are mixed in."""
    rng = np.random.RandomState(6)
    parts = []
    n = 700
    # lp = 2: min == max
    parts.append((np.full(n, 1.5), rng.randn(n), rng.rand(n) + 0.1, np.full(n, 0.5)))
    # lp <= 17: the whole row is one 16-wide window; every fourth scale at the clamp
    x, mean, scale, q = _small(rng, n, -7, 7)
    scale[::4] = CLAMP
    parts.append((x, mean, scale, q))
    # 18 .. 65 entries: a 64-wide window holds the row; means far outside the levels
    x, mean, scale, q = _small(rng, n, -25, 25)
    mean[::5] = 400.0
    mean[1::5] = -400.0
    parts.append((x, mean, scale, q))
    # the scaling attribute: Q = 0.001, sigma / Q about 50, a few thousand levels
    mean = -4.0 + rng.randn(n) * 0.3
    scale = np.full(n, 0.05) * (0.8 + 0.4 * rng.rand(n))
    x = mean + scale * rng.randn(n)
    x[0], x[1] = x.min() - 1.0, x.max() + 1.0
    parts.append((x, mean, scale, np.full(n, 0.001)))
    # sigma / Q below 1 and the value far in a tail: the windows around the mean and around the quantile miss, the binary search runs
    mean = rng.rand(n) * 20.0 - 10.0
    mean[::7] = 40.0                                          # outside [min, max] * Q
    mean[3::7] = -40.0
    scale = np.full(n, 0.005)
    scale[::3] = CLAMP
    x = rng.rand(n) * 30.0 - 15.0
    parts.append((x, mean, scale, np.full(n, 0.01)))
    return Slices(parts)


def _encode(torch, s):
    from gauspcc_amd import arithmetic

    return arithmetic.encode_normal_streams(*s.dev(torch), s.start)


def _host_coder(sym, rows):
    """torchac's coder on host arrays: (bytes of gsac_host_encode_u16, symbols of gsac_host_decode_u16 on those bytes)"""
    from gauspcc_amd import _lib

    n, lp = rows.shape
    sym = np.ascontiguousarray(sym, dtype=np.int16)
    rows = np.ascontiguousarray(rows)
    out = np.empty(4 * n + 64, dtype=np.uint8)
    nb = C.c_int64()
    _lib.check(_lib.lib().gsac_host_encode_u16(sym.ctypes.data, rows.ctypes.data, n, lp, out.ctypes.data, out.size, C.byref(nb)))
    data = np.ascontiguousarray(out[:nb.value])
    back = np.zeros(n, dtype=np.int16)
    _lib.check(_lib.lib().gsac_host_decode_u16(rows.ctypes.data, data.ctypes.data, data.size, n, lp, back.ctypes.data))
    return data, back


def _rows_checks(torch, s, a, b, mn, mx):
    """rows of slice [a, b) from the library: strictly increasing, within 1 of the torch-built table; returns (rows uint16 host, entries, differing)"""
    from gauspcc_amd import arithmetic
    from gauspcc_amd import torchac_encodings as te

    mean, scale, q = (torch.tensor(v[a:b]).cuda() for v in (s.mean, s.scale, s.q))
    rows = arithmetic.normal_cdf_rows(mean, scale, q, mn, mx)
    lp = mx - mn + 2
    assert rows.shape == (b - a, lp) and rows.dtype == torch.int16
    r = rows.to(torch.int32) & 0xFFFF
    r[:, -1] = torch.where(r[:, -1] == 0, torch.full_like(r[:, -1], 65536), r[:, -1])     # the last entry is 2^16 modulo 2^16 when the row ends at 1.0
    assert bool((r[:, 1:] > r[:, :-1]).all()), "rows are not strictly increasing"
    ref = te._int_rows(mean, scale, q, mn, mx).to(torch.int32) & 0xFFFF
    ref[:, -1] = torch.where(ref[:, -1] == 0, torch.full_like(ref[:, -1], 65536), ref[:, -1])
    d = (r - ref).abs()
    assert int(d.max()) <= 1, f"an entry differs from the torch-built table by {int(d.max())}"
    return rows.cpu().numpy().view(np.uint16), d.numel(), int((d != 0).sum())


@pytest.fixture(scope="module")
def coded(torch_cuda):
    """Both cases encoded once: name -> (Slices, mins, maxs, bytes, cnt)."""
    out = {}
    for name, make in (("lengths", lengths_case), ("alphabets", alphabets_case)):
        s = make()
        out[name] = (s,) + tuple(_encode(torch_cuda, s))
    return out


@pytest.mark.parametrize("name", ["lengths", "alphabets"])
def test_rows_and_bytes_match_torchac(torch_cuda, coded, name):
    torch = torch_cuda
    s, mins, maxs, data, cnt = coded[name]
    ns = s.start.size - 1
    assert mins.shape == maxs.shape == cnt.shape == (ns,) and int(cnt.sum()) == data.size
    off = np.concatenate([[0], np.cumsum(cnt)])
    entries = differing = 0
    lps = []
    for i in range(ns):
        a, b = int(s.start[i]), int(s.start[i + 1])
        if b == a:
            assert cnt[i] == 0 and mins[i] == 0 and maxs[i] == 0
            continue
        xi = np.rint(s.x[a:b] / s.q[a:b])                       # float32 division, ties to even
        assert mins[i] == xi.min() and maxs[i] == xi.max()
        mn, mx = int(mins[i]), int(maxs[i])
        lps.append(mx - mn + 2)
        rows, e, d = _rows_checks(torch, s, a, b, mn, mx)
        entries += e; differing += d
        sym = (xi - mn).astype(np.int16)
        want, back = _host_coder(sym, rows)
        got = data[off[i]:off[i + 1]]
        assert got.size == want.size and np.array_equal(got, want), f"slice {i} (lp {lps[-1]}): stream differs from torchac's on the same rows"
        assert np.array_equal(back, sym)
    print(f"\n{name}: alphabets {lps}; {differing} of {entries} row entries differ from the torch-built table ({differing / max(entries, 1):.3e})")
    if name == "alphabets":      # the tiers the case is built for
        assert lps[0] == 2 and lps[1] <= 17 and 18 <= lps[2] <= 65 and lps[3] >= 2000 and lps[4] >= 2000


@pytest.mark.parametrize("name", ["lengths", "alphabets"])
def test_decode_round_trip_is_exact(torch_cuda, coded, name):
    torch = torch_cuda
    from gauspcc_amd import arithmetic

    s, mins, maxs, data, cnt = coded[name]
    x, mean, scale, q = s.dev(torch)
    got = arithmetic.decode_normal_streams(mean, scale, q, s.start, mins, maxs, data, cnt)
    want = torch.round(x / q) * q
    bad = torch.nonzero(got != want).flatten()
    assert bad.numel() == 0, f"{bad.numel()} values differ, the first at element {int(bad[0])} (slice {int(np.searchsorted(s.start, int(bad[0]), 'right')) - 1})"


def test_range_and_parameter_errors(torch_cuda):
    torch = torch_cuda
    from gauspcc_amd import _lib, arithmetic

    n = 64
    one = lambda v: torch.full((n,), float(v), device="cuda")
    x = one(0.0)
    x[1] = 32766.0                                               # levels 0 .. 32766: 32 767 of them, one more than int16 symbols index
    with pytest.raises(_lib.GpccError) as e:
        arithmetic.encode_normal_streams(x, one(0.0), one(1.0), one(1.0), [0, n])
    assert e.value.code == RANGE
    x[1] = 32765.0                                               # 32 766 levels: the widest alphabet
    mins, maxs, data, cnt = arithmetic.encode_normal_streams(x, one(0.0), one(1.0), one(1.0), [0, n])
    assert (mins[0], maxs[0]) == (0.0, 32765.0)
    assert torch.equal(arithmetic.decode_normal_streams(one(0.0), one(1.0), one(1.0), [0, n], mins, maxs, data, cnt), x)
    # (which of mean / scale / Q, the value put into one element): refused with an error, nothing computes with it
    for which, value in ((1, float("nan")), (0, float("inf")), (2, 0.0), (2, float("nan")), (1, 0.0)):
        params = [one(0.0), one(1.0), one(1.0)]
        params[which][n // 2] = value
        with pytest.raises(_lib.GpccError):
            arithmetic.encode_normal_streams(one(3.0), *params, [0, 10, n])
    # and the context still works
    mins, maxs, data, cnt = arithmetic.encode_normal_streams(one(3.0), one(0.0), one(1.0), one(1.0), [0, 10, n])
    assert mins.tolist() == [3.0, 3.0] and maxs.tolist() == [3.0, 3.0] and int(cnt.min()) > 0


def test_truncated_and_foreign_streams_stay_inside_the_alphabet(torch_cuda, coded):
    torch = torch_cuda
    from gauspcc_amd import arithmetic

    s, mins, maxs, data, cnt = coded["alphabets"]
    _, mean, scale, q = s.dev(torch)
    off = np.concatenate([[0], np.cumsum(cnt)])
    half = np.concatenate([data[off[i]:off[i] + cnt[i] // 2] for i in range(cnt.size)])
    zeros = np.zeros(int(cnt.sum()), dtype=np.uint8)
    lo = torch.tensor(np.repeat(mins, np.diff(s.start))).cuda() * q
    hi = torch.tensor(np.repeat(maxs, np.diff(s.start))).cuda() * q
    for blob, c in ((half, cnt // 2), (zeros, cnt), (np.empty(0, np.uint8), np.zeros_like(cnt))):
        got = arithmetic.decode_normal_streams(mean, scale, q, s.start, mins, maxs, blob, c)         # status OK: no exception
        assert bool(torch.isfinite(got).all()) and bool((got >= lo).all()) and bool((got <= hi).all())


def test_two_contexts_on_two_streams_give_the_solo_bytes(torch_cuda, coded):
    """Two host threads (a context each, runtime.context) on their own streams, at the same time."""
    torch = torch_cuda
    results, errors = {}, []

    def work(name):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                s = coded[name][0]
                for _ in range(3):
                    results[name] = _encode(torch, s)
        except BaseException as e:      # noqa: BLE001 -- reported on the test's thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(name,)) for name in ("lengths", "alphabets")]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for name in ("lengths", "alphabets"):
        for got, want in zip(results[name], coded[name][1:]):
            assert np.array_equal(got, want), name
