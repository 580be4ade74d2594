"""Every search tier and alphabet edge of the attribute decoder hac_decode_chunk (gauspcc_amd/csrc/attributes.hip) against the oracle coder.

The decoder finds a symbol in a 16-candidate window (tier 1), a 64-candidate window (tier 2) or a binary search (tier 3), with window positions
specialised for generic tables, GaussTable and MixTable rows; tests/hac_tier_ref.py says which tier a symbol MUST take and
tests/hac_tier_cases.py builds inputs with stated quotas of each (tests/test_hac_tier_ref_cpu.py proves the quotas for the oracle alone; they are
asserted again here).  Every comparison is exact.  The device and the oracle use different erfc libraries, so the expected bytes come from the
ORACLE CODER run on the TABLE THE DEVICE COMPUTED, and that table is held to the oracle's at 2e-7 absolute.

For every Gaussian / mixture case: the table-free fused encode and arithmetic_encode(sym, device_table) give the oracle's bytes and chunk counts;
the table-free fused decode, arithmetic_decode(device_table) and orc.hac_decode return the symbols; min / max are those of torch.round(x / q).
A mismatch message names the first differing row and its certain tier: that is the branch to read.
"""
import ctypes as C

import numpy as np
import pytest

from . import hac_tier_cases as hc

pytestmark = pytest.mark.gpu

RANGE = -3                                                     # GPCC_ERR_RANGE (include/gauspcc.h)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch


def _first_diff(got, want, tiers, what, case):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    if got.shape != want.shape:
        raise AssertionError(f"{case} {what}: shape {got.shape}, expected {want.shape}")
    r = int(np.nonzero(got != want)[0][0])
    raise AssertionError(f"{case} {what}: first difference at row {r} (row {r % case.chunk} of chunk {r // case.chunk}): got {got[r]}, expected {want[r]}; "
                         f"certain tier {int(tiers[r])} (0: unknown); {int((got != want).sum())} rows differ")


def _same_stream(b, cnt, rb, rcnt, what, case):
    cnt, b = cnt.cpu().numpy() if hasattr(cnt, "cpu") else cnt, b.cpu().numpy() if hasattr(b, "cpu") else b
    assert np.array_equal(cnt, rcnt), f"{case} {what}: chunk byte counts differ at chunks {np.nonzero(np.asarray(cnt) != rcnt)[0][:8]}"
    assert np.array_equal(b, rb), f"{case} {what}: payload differs from byte {int(np.nonzero(b != rb)[0][0])} of {rb.size}"


def _check_case(torch, orc, case):
    """The whole list of the module docstring for one Gaussian / mixture case.  Returns the oracle's chunk byte counts."""
    from gauspcc_amd import arithmetic

    tiers = hc.check_static(case)
    sym, mn, mx = hc.symbols(case)
    n, lp, chunk = case.n, mx - mn + 2, case.chunk
    dev = lambda a: torch.tensor(a).cuda()
    x, q = dev(case.x), dev(case.q)
    xi = torch.round(x / q)
    assert float(xi.min()) == mn and float(xi.max()) == mx
    if case.kind == "gauss":
        params = (dev(case.mean), dev(case.scale), q)
        table = arithmetic.calculate_cdf(*params, mn, mx)
        enc, dec = arithmetic.encode_gaussian, arithmetic.decode_gaussian
    else:
        params = ([dev(a) for a in case.mean], [dev(a) for a in case.scale], [dev(a) for a in case.prob], q)
        table = arithmetic.calculate_cdf_mixed(*params, mn, mx)
        enc, dec = arithmetic.encode_gaussian_mixed, arithmetic.decode_gaussian_mixed
        ref = arithmetic.calculate_cdf(params[0][0], params[1][0], q, mn, mx) * params[2][0].unsqueeze(-1)
        for i in range(1, len(case.mean)):                       # the reference's torch expression, op for op, in list order
            ref = ref + arithmetic.calculate_cdf(params[0][i], params[1][i], q, mn, mx) * params[2][i].unsqueeze(-1)
        assert torch.equal(table, torch.clamp(ref, min=0.0, max=1.0)), f"{case}: mixture table is not the clamped weighted sum of its components' tables"
        del ref
    tab = table.cpu().numpy()
    assert tab.shape == (n, lp)
    err = float(np.abs(tab - hc.oracle_table(orc, case)).max())
    assert err <= 2e-7, f"{case}: device table differs from the oracle's by {err:.3g}"
    rb, rcnt = orc.hac_encode(sym, tab, chunk)
    hc.check_cnt(case, rcnt)
    _first_diff(orc.hac_decode(tab, rb, rcnt, chunk), sym, tiers, "oracle decode", case)
    fmn, fmx, b, cnt = enc(x, *params, chunk)
    assert fmn == mn and fmx == mx
    _same_stream(b, cnt, rb, rcnt, "fused encode", case)
    b2, cnt2 = arithmetic.arithmetic_encode(dev(sym), table, chunk, n, lp)
    _same_stream(b2, cnt2, rb, rcnt, "arithmetic_encode", case)
    got = dec(*params, fmn, fmx, b, cnt, chunk)
    _first_diff(got.cpu().numpy(), (xi * q).cpu().numpy(), tiers, "fused decode", case)
    assert torch.equal(got, xi * q)
    _first_diff(arithmetic.arithmetic_decode(table, b, cnt, chunk, n, lp).cpu().numpy(), sym, tiers, "arithmetic_decode", case)
    return rcnt


# ------------------------------------------------------------------ a. GaussTable
@pytest.mark.parametrize("make", [lambda: hc.gauss_narrow(mn=-150), lambda: hc.gauss_clamped(mn=5000), lambda: hc.gauss_clamped(seed=22, mn=-5300),
                                  lambda: hc.gauss_wide()], ids=["narrow_tiers_1_2_3", "clamped_min5000", "clamped_min-5300", "wide_scale_over_q_50"])
def test_gaussian_rows_every_tier(torch_cuda, orc, make):
    """GaussTable, tiers 1, 2 and 3, >= 20 % of the symbols certain in each and mixed inside every pass of four rows: narrow rows (scale / q in
    {0, 0.25, 0.5, 1}; scale 0 is clamped to 1e-9) with x at |s - centre| <= 7, 8..25, >= 40 on both sides, at 0 and at max_symbol; the same with the mean far
    below and far above [min, max] (min = 5000 and -5300), which saturates both clamps of s0 and w0; and wide rows (scale / q about 50, >= 400
    symbols, tier 1 misses >= 50 %) where the quantile estimate carries the decode."""
    _check_case(torch_cuda, orc, make())


# ------------------------------------------------------------------ b. MixTable
@pytest.mark.parametrize("k", [2, 3, 4])
def test_mixture_rows_light_component(torch_cuda, orc, k):
    """MixTable, k = 2, 3, 4 (MIX_MAX): the symbol comes from a light, narrow component >= 100 symbols from the heaviest one's mean, so centre and
    estimate both point at the wrong component: >= 20 % of the symbols certain in tier 3; every fifth row has two exactly equal largest weights.
    calculate_cdf_mixed is bit-equal to clamp(sum_i calculate_cdf_i * prob_i, 0, 1) in list order."""
    _check_case(torch_cuda, orc, hc.mixture(k))


# ------------------------------------------------------------------ c. generic tables
def _u16(torch, sym, tab16, chunk, n, lp):
    """gsac_encode_u16 / gsac_decode_u16 on device tensors: (bytes, cnt, decoded symbols)."""
    from gauspcc_amd import _lib, arithmetic, runtime

    L, ctx, st = _lib.lib(), runtime.context(sym.device), runtime.stream_ptr(sym.device)
    pb, nb, pc, nc = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
    _lib.check(L.gsac_encode_u16(ctx, sym.data_ptr(), tab16.data_ptr(), chunk, n, lp, C.byref(pb), C.byref(nb), C.byref(pc), C.byref(nc), st))
    data, cnt = arithmetic._owned(pb, nb.value, np.uint8), arithmetic._owned(pc, nc.value, np.int32)
    out = torch.zeros(n, dtype=torch.int16, device=sym.device)
    _lib.check(L.gsac_decode_u16(ctx, tab16.data_ptr(), data.ctypes.data, data.size, cnt.ctypes.data, chunk, n, lp, out.data_ptr(), st))
    return data, cnt, out.cpu().numpy()


@pytest.mark.parametrize("lp", [100, 1000])
def test_generic_tables_skewed_rows(torch_cuda, orc, lp):
    """Generic float and uint16 tables, lp = 100 and 1000: rows with all mass in the last (first) three symbols code a mid-row symbol, so the
    estimate p * max_symbol is more than 40 symbols off: >= 20 % of the symbols certain in tier 3 (peaked and uniform rows give tiers 1 and 2).
    The uint16 coder on orc.cdf_to_int16 of the table writes the float path's bytes and decodes the same symbols."""
    torch = torch_cuda
    from gauspcc_amd import arithmetic

    case = hc.skewed_table(lp)
    tiers = hc.check_static(case)
    n, chunk, sym = case.n, case.chunk, case.sym
    rb, rcnt = orc.hac_encode(sym, case.cdf, chunk)
    hc.check_cnt(case, rcnt)
    table, dsym = torch.tensor(case.cdf).cuda(), torch.tensor(sym).cuda()
    b, cnt = arithmetic.arithmetic_encode(dsym, table, chunk, n, lp)
    _same_stream(b, cnt, rb, rcnt, "arithmetic_encode", case)
    _first_diff(arithmetic.arithmetic_decode(table, b, cnt, chunk, n, lp).cpu().numpy(), sym, tiers, "arithmetic_decode", case)
    _first_diff(orc.hac_decode(case.cdf, rb, rcnt, chunk), sym, tiers, "oracle decode", case)
    tab16 = torch.tensor(orc.cdf_to_int16(case.cdf)).cuda()
    b16, cnt16, dec16 = _u16(torch, dsym, tab16, chunk, n, lp)
    _same_stream(b16, cnt16, rb, rcnt, "uint16 encode", case)
    _first_diff(dec16, sym, tiers, "uint16 decode", case)


# ------------------------------------------------------------------ d. alphabet boundaries
@pytest.mark.parametrize("m", hc.BOUNDARY_M)
def test_alphabet_boundary_gaussian(torch_cuda, orc, m):
    """max_symbol = max - min in {0, 1, 14, 15, 16, 17, 62, 63, 64, 65, 200, 4000, 32765} (the last: lp = 32767, the largest the format takes), the range
    forced by one element at min and one at max; symbols 0, 1, max_symbol - 1, max_symbol, s0 + 14, s0 + 15, w0 + 62, w0 + 63 where the alphabet has
    them (scale-0 rows, where s0 and w0 are known), the rest uniform on wide rows."""
    _check_case(torch_cuda, orc, hc.boundary(m))


@pytest.mark.parametrize("m", hc.BOUNDARY_M_MIX)
def test_alphabet_boundary_mixture(torch_cuda, orc, m):
    """The same through MixTable (k = 2) for max_symbol in {15, 16, 63, 64, 4000}."""
    _check_case(torch_cuda, orc, hc.boundary(m, mixed=True))


# ------------------------------------------------------------------ e. the encoder's refusal
def test_encoders_refuse_32767_levels(torch_cuda):
    """Quantised values 32 766 apart need a row of 32 768 entries, one more than int16 symbols index: encode_gaussian, encode_gaussian_mixed and both
    slices encoders (only ONE slice is too wide there) return GPCC_ERR_RANGE "quantised values span ...".  The same context then encodes and
    decodes a valid stream exactly."""
    torch = torch_cuda
    from gauspcc_amd import _lib, arithmetic

    d = hc.too_wide()
    dev = lambda a: torch.tensor(a).cuda()
    x, q = dev(d["x"]), dev(d["q"])
    plain = (dev(d["mean"]), dev(d["scale"]), q)
    mixed = ([plain[0], dev(d["mean2"])], [plain[1], dev(d["scale2"])], [dev(p) for p in d["prob"]], q)
    bounds, chunk = list(hc.TOO_WIDE_BOUNDS), 128
    ok = x.clamp(-300.0, 300.0).contiguous()                            # the two outliers pulled in: 601 levels
    for params, enc, dec, encs, decs in ((plain, arithmetic.encode_gaussian, arithmetic.decode_gaussian, arithmetic.encode_gaussian_slices, arithmetic.decode_gaussian_slices),
                                         (mixed, arithmetic.encode_gaussian_mixed, arithmetic.decode_gaussian_mixed, arithmetic.encode_gaussian_mixed_slices,
                                          arithmetic.decode_gaussian_mixed_slices)):
        for call in (lambda: enc(x, *params, chunk), lambda: encs(x, *params, bounds, chunk)):
            with pytest.raises(_lib.GpccError) as e:
                call()
            assert e.value.code == RANGE and "quantised values span" in str(e.value), str(e.value)
        mn, mx, b, cnt = enc(ok, *params, chunk)
        assert (mn, mx) == (-300.0, 300.0)
        assert torch.equal(dec(*params, mn, mx, b, cnt, chunk), torch.round(ok / q) * q)
        mins, maxs, data, scnt = encs(ok, *params, bounds, chunk)
        assert torch.equal(decs(*params, bounds, mins, maxs, data, scnt, chunk), torch.round(ok / q) * q)


# ------------------------------------------------------------------ f. chunk shapes
@pytest.mark.parametrize("wide", [True, False], ids=["alphabet_over_64", "alphabet_15"])
@pytest.mark.parametrize("n,chunk", hc.CHUNK_SHAPES)
def test_chunk_shapes(torch_cuda, orc, n, chunk, wide):
    """Chunks of 1, 2, 3, 4, 5, 63, 64, 65, 67, 128 and 129 symbols (cn no multiple of 4 or 64, cn = 1, the min(j0 + lane, cn - 1) row clamp): chunk = 1
    makes one chunk per symbol, several shapes end on a chunk of one symbol, the last has chunk > n.  On wide Gaussian rows (alphabet > 64) and
    on an alphabet of 15 symbols (lp = 16)."""
    _check_case(torch_cuda, orc, hc.chunk_shape(n, chunk, wide))


# ------------------------------------------------------------------ g. bit reader
def test_bit_reader_block_crossings_and_partial_words(torch_cuda, orc):
    """WaveBits at high rate (about 10 bits per symbol, chunks of 700 and 2 000 symbols): every chunk is beyond 512 bytes, so the reader crosses its
    256-byte blocks more than once, and the byte counts take all four residues mod 4, so it ends on every length of partial word."""
    hc.check_residues([_check_case(torch_cuda, orc, case) for case in hc.high_rate_streams()])


def test_bit_reader_near_empty_chunks(torch_cuda, orc):
    """WaveBits on near-empty chunks: scale = 0 and every x on its mean in 10 000-symbol chunks, the alphabet (101 symbols) forced wider than 64 by two
    outliers in the middle chunk; the pure chunks have at most 8 bytes."""
    _check_case(torch_cuda, orc, hc.near_zero_rate())


# ------------------------------------------------------------------ h. worst legal rate
def test_worst_legal_rate_fills_the_scratch_bound(torch_cuda, orc):
    """One 10 000-symbol chunk in which every symbol has the smallest interval (hi == lo + 1; scale = 0, x >= 3 symbols off its mean): 16 bits per
    symbol, 16 n <= 8 cnt <= 16 n + 256, against the encoder's per-chunk scratch of 2 * symbols + 32 bytes.  Bytes equal the oracle's."""
    _check_case(torch_cuda, orc, hc.worst_rate())


# ------------------------------------------------------------------ i. slices in one launch
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mixture_k2"])
def test_slices_of_every_alphabet_in_one_launch(torch_cuda, tmp_path, mixed):
    """k_hac_decode_slices (per-slice min and lp): ONE call codes slices of max_symbol 0, 15, 16, 63, 64 and 3000 with ragged 10 000-symbol chunks (a
    slice of one symbol, two slices whose second chunk holds 1 and 64 symbols); the plain form also gets an empty slice, which the mixture's wrapper
    does not take.  Every file is byte-equal to the per-slice stream encoder's, the decode is exact, and >= 20 % of the widest slice's symbols
    are certain in tier 3."""
    torch = torch_cuda
    from gauspcc_amd import encodings_cuda as ec

    bounds, cases = hc.slices()
    if mixed:
        cases = [c for c in cases if c is not None]
        bounds = [0] + np.cumsum([c.n for c in cases]).tolist()
    live = [c for c in cases if c is not None]
    for c in live:
        hc.check_static(hc.as_mixture(c) if mixed else c)
    cat = lambda f: torch.tensor(np.concatenate([f(c) for c in live])).cuda()
    x, q = cat(lambda c: c.x), cat(lambda c: c.q)
    if mixed:
        params = ([cat(lambda c: c.mean), cat(lambda c: c.mean2)], [cat(lambda c: c.scale), cat(lambda c: c.scale2)],
                  [cat(lambda c: c.prob[0]), cat(lambda c: c.prob[1])], q)
        enc_all, dec_all, enc_one = ec.encoder_gaussian_mixed_slices, ec.decoder_gaussian_mixed_slices, ec.encoder_gaussian_mixed_chunk
        cut = lambda sl: ([t[sl] for t in params[0]], [t[sl] for t in params[1]], [t[sl] for t in params[2]], q[sl])
    else:
        params = (cat(lambda c: c.mean), cat(lambda c: c.scale), q)
        enc_all, dec_all, enc_one = ec.encoder_gaussian_slices, ec.decoder_gaussian_slices, ec.encoder_gaussian_chunk
        cut = lambda sl: (params[0][sl], params[1][sl], q[sl])
    ns = len(bounds) - 1
    a = [str(tmp_path / f"a_{s}.b") for s in range(ns)]
    b = [str(tmp_path / f"b_{s}.b") for s in range(ns)]
    file_of = lambda name: open(name.replace(".b", "_0.b"), "rb").read()
    bits = enc_all(x, *params, bounds, a)
    for s in range(ns):
        sl = slice(bounds[s], bounds[s + 1])
        if bounds[s + 1] == bounds[s]:
            assert bits[s] == 0
            continue
        assert bits[s] == enc_one(x[sl], *cut(sl), file_name=b[s])
        assert file_of(a[s]) == file_of(b[s]), f"slice {s} ({cases[s]}): the one-call file differs from the stream encoder's"
    want = (torch.round(x / q) * q).cpu().numpy()
    got = dec_all(*params, bounds, b).cpu().numpy()
    for c, lo in zip(live, [bounds[s] for s in range(ns) if bounds[s + 1] > bounds[s]]):
        _first_diff(got[lo:lo + c.n], want[lo:lo + c.n], hc.tiers(hc.as_mixture(c) if mixed else c), "slices decode", c)
