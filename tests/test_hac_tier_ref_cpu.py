"""The inputs of tests/test_gpu_attr_coder_tiers.py meet their stated conditions for the ORACLE alone: tier quotas (tests/hac_tier_ref.py: which
search tier of hac_decode_chunk a symbol must take), max_symbol, chunk byte-count residues and sizes, and the encoder's 2 * symbols + 32 scratch
bytes per chunk -- and every case round-trips exactly through orc.hac_encode / orc.hac_decode on orc.gaussian_cdf / orc.gaussian_mixed_cdf.
So the conditions are properties of the inputs and the reference, not of the code under test.  No GPU."""
import numpy as np
import pytest

from . import hac_tier_cases as hc
from . import hac_tier_ref as tr


def _roundtrip(orc, case):
    """Oracle table -> oracle coder -> oracle decoder; the static and byte-count conditions of the case.  Returns (tiers, cnt)."""
    t = hc.check_static(case)
    sym, _, _ = hc.symbols(case)
    table = hc.oracle_table(orc, case)
    assert table.shape == (case.n, int(sym.max()) + 2)
    data, cnt = orc.hac_encode(sym, table, case.chunk)
    assert int(cnt.sum()) == data.size
    assert np.array_equal(orc.hac_decode(table, data, cnt, case.chunk), sym), case
    hc.check_cnt(case, cnt)
    return t, cnt


# ------------------------------------------------------------------ the helper itself
def test_window_rules_against_a_direct_search():
    """tier1_hit / certain_tier against the rule spelled out candidate by candidate, for every (max_symbol, centre, symbol) of small alphabets and the
    boundaries 15/16 and 63/64."""
    for m in (0, 1, 14, 15, 16, 17, 62, 63, 64, 65, 90):
        for centre in range(-10, m + 11):
            s0 = 0 if m <= 15 else max(0, min(centre - 7, m - 15))
            w0 = 0 if m <= 63 else max(0, min(centre - 31, m - 63))
            for s in range(m + 1):
                top = s - s0
                hit1 = 0 <= top <= 15 and (top < 15 or s == m)
                assert bool(tr.tier1_hit(centre, s, m)) == hit1, (m, centre, s)
                topw = s - w0
                hit2 = 0 <= topw <= 63 and (topw < 63 or s == m)
                want = 1 if hit1 else 2 if hit2 else 3
                got = int(tr.certain_tier(np.array([centre]), np.array([centre]), np.array([centre]), np.array([s]), m)[0])
                assert got == want, (m, centre, s, got, want)


def test_centres_and_ties():
    """Gaussian centre = rint(mean / q) - min, half to even; the mixture takes the FIRST of equal largest weights."""
    assert tr.centre_gaussian(np.float32([2.5, 3.5, -0.5, 7.0]), np.float32([1, 1, 1, 2]), -3).tolist() == [5, 7, 3, 7]
    assert tr.centre_table(3, 99).tolist() == [49, 49, 49]
    probs = [np.float32([0.4, 0.2, 0.3]), np.float32([0.4, 0.5, 0.3]), np.float32([0.2, 0.3, 0.4])]
    assert tr.heaviest(probs).tolist() == [0, 1, 2]
    means = [np.float32([10, 10, 10]), np.float32([20, 20, 20]), np.float32([30, 30, 30])]
    assert tr.centre_mixture(means, means, probs, np.float32([1, 1, 1]), 0).tolist() == [10, 20, 30]


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("make", [lambda: hc.gauss_narrow(mn=-150), lambda: hc.gauss_clamped(mn=5000), lambda: hc.gauss_clamped(seed=22, mn=-5300),
                                  lambda: hc.gauss_wide()], ids=["narrow", "clamped_min5000", "clamped_min-5300", "wide"])
def test_gaussian_tier_cases(orc, make):
    """a. GaussTable: >= 20 % of the symbols certain in each of tiers 1, 2, 3, mixed inside every four rows (narrow; both clamps saturated with the
    mean far below / above [min, max]); wide rows: >= 400 symbols, tier 1 misses >= 50 %."""
    _roundtrip(orc, make())


@pytest.mark.parametrize("k", [2, 3, 4])
def test_mixture_tier_cases(orc, k):
    """b. MixTable, k = 2, 3, 4: >= 20 % of the symbols certain in tier 3; rows with two exactly equal largest weights are present."""
    case = hc.mixture(k)
    _roundtrip(orc, case)
    p = np.stack(case.prob)
    top = p.max(0)
    tied = (p == top[None, :]).sum(0) >= 2
    assert tied.mean() >= 0.15 and np.all(p[0][tied] == top[tied]) and np.all(p[1][tied] == top[tied])
    assert np.abs(p.sum(0) - 1).max() < 1e-6


@pytest.mark.parametrize("lp", [100, 1000])
def test_table_tier_cases(orc, lp):
    """c. generic float / uint16 tables, lp = 100 and 1000: >= 20 % of the symbols certain in tier 3; the uint16 form of the table (orc.cdf_to_int16)
    gives the same tiers."""
    case = hc.skewed_table(lp)
    t, _ = _roundtrip(orc, case)
    t16 = tr.tiers_table(orc.cdf_to_int16(case.cdf), case.sym.astype(np.int64), lp - 2)
    assert np.array_equal(t, t16)
    assert np.all(np.diff(tr.integerise(case.cdf), axis=1) >= 1)


@pytest.mark.parametrize("m", hc.BOUNDARY_M)
def test_boundary_cases(orc, m):
    """d. max_symbol in {0, 1, 14, 15, 16, 17, 62, 63, 64, 65, 200, 4000, 32765}; the window-edge symbols s0 + 14, s0 + 15, w0 + 62, w0 + 63 occur where the
    alphabet has them, in tiers 1, 2, 2 and 3."""
    case = hc.boundary(m)
    t, _ = _roundtrip(orc, case)
    sym, mn, _ = hc.symbols(case)
    s = sym.astype(np.int64)
    even = np.arange(case.n) % 2 == 0
    c = tr.centre_gaussian(case.mean, case.q, mn)
    s0, w0 = tr.window_start(c, m, 16, 7), tr.window_start(c, m, 64, 31)
    exact = tr.certain_tier(c, c, c, s, m)          # scale = 0: the estimate IS the centre
    # (a clamped window can put s0 + 15 or w0 + 62 inside tier 1's reach, and the last candidate is accepted where it is max_symbol)
    for edge, tier, exists, last in ((s0 + 14, 1, m >= 14, False), (s0 + 15, 2, m >= 17, True), (w0 + 62, 2, m >= 64, False), (w0 + 63, 3, m >= 65, True)):
        at = even & (s == edge) & ((edge < m) if last else (edge <= m))
        if exists:
            assert np.any(exact[at] == tier) and np.all((exact[at] == tier) | (exact[at] == 1)), (m, tier, exact[at])
            assert np.all((t[at] == exact[at]) | (t[at] == 0)), (m, tier, t[at])
    if m in hc.BOUNDARY_M_MIX:
        _roundtrip(orc, hc.boundary(m, mixed=True))


def test_chunk_shape_cases(orc):
    """f. chunks of 1, 2, 3, 4, 5, 63, 64, 65, 67, 128, 129 symbols, a last chunk of one symbol, chunk > n; an alphabet wider than 64 and one of 15 symbols."""
    seen = set()
    for n, chunk in hc.CHUNK_SHAPES:
        for wide in (True, False):
            case = hc.chunk_shape(n, chunk, wide)
            _roundtrip(orc, case)
            seen |= set(hc.chunk_lengths(n, chunk))
    assert {1, 2, 3, 4, 5, 63, 64, 65, 67, 128, 129} <= seen
    assert any(hc.chunk_lengths(n, c)[-1] == 1 and len(hc.chunk_lengths(n, c)) > 1 for n, c in hc.CHUNK_SHAPES) and any(c > n for n, c in hc.CHUNK_SHAPES)


def test_bit_reader_cases(orc):
    """g. high rate: every chunk beyond 512 bytes, all four residues of the byte count mod 4; near-zero rate: the pure chunks take <= 8 bytes."""
    cnts = [_roundtrip(orc, case)[1] for case in hc.high_rate_streams()]
    hc.check_residues(cnts)
    for case, cnt in zip(hc.high_rate_streams(), cnts):
        lens = np.array(hc.chunk_lengths(case.n, case.chunk))
        assert np.all(8 * cnt >= 9.5 * lens), (8 * cnt / lens)               # about 10 bits per symbol
    _roundtrip(orc, hc.near_zero_rate())


def test_worst_rate_case(orc):
    """h. every symbol at the smallest interval (hi == lo + 1): 16 bits each, 16 n <= 8 cnt <= 16 n + 256 -- inside the encoder's 2 * symbols + 32 bytes."""
    case = hc.worst_rate()
    _roundtrip(orc, case)
    sym, _, _ = hc.symbols(case)
    c = tr.integerise(hc.oracle_table(orc, case))
    rows = np.arange(case.n)
    assert np.all(c[rows, sym + 1] - c[rows, sym] == 1)


def test_slice_cases(orc):
    """i. slices of max_symbol 0, 15, 16, 63, 64, 3000 and an empty one; tier-3-certain symbols in the widest; plain and two-component form."""
    bounds, cases = hc.slices()
    assert np.diff(bounds).tolist() == list(hc.SLICE_LEN) and 0 in np.diff(bounds)
    for case in cases:
        if case is not None:
            _roundtrip(orc, case)
            _roundtrip(orc, hc.as_mixture(case))


def test_too_wide_case():
    """e. 32 767 levels: row length 32 768, one more than the format takes."""
    d = hc.too_wide()
    xi = np.rint(d["x"] / d["q"])
    assert int(xi.max() - xi.min()) + 2 == 32768
