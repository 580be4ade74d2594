"""Which search tier of the attribute decoder a symbol must take: a numpy restatement of the WINDOW RULES of hac_decode_chunk
(gauspcc_amd/csrc/attributes.hip).  It is no coder and imports nothing from the library.

The decoder finds the symbol s of a row in three tiers, 0 <= s <= max_symbol = lp - 2:

  tier 1  16 candidates from s0 = clamp(centre - 7, 0, max_symbol - 15)  (s0 = 0 when max_symbol <= 15);
          taken when the highest qualifying candidate is not the window's last one, or is max_symbol itself
  tier 2  64 candidates from w0 = clamp(estimate - 31, 0, max_symbol - 63)  (w0 = 0 when max_symbol <= 63); same acceptance rule
  tier 3  binary search over 0 .. max_symbol

`centre` depends on the row alone, so tier 1 is decided exactly.  `estimate` depends on the coder's state (p = (value - low) / span), so
tiers 2 and 3 are decided only where EVERY estimate the row allows gives the same answer: the functions answer 1, 2, 3 or 0 for "unknown".

    generic table   centre = max_symbol // 2                 estimate = int(p * max_symbol), p within the symbol's integerised interval
    Gaussian        centre = rint(mean / q) - min            estimate = rint((mean + max(scale, 1e-9) * z) / q) - min, |z| <= 5.2
    mixture         the same from the heaviest component (strict >: the first of equal weights)

(normcdfinv(1e-7) = -5.1993, and the decoder clamps p to [1e-7, 1 - 1e-7].)  float32 where the kernel is float32; np.rint is half-to-even
like rintf.
"""
import numpy as np

Z_MAX = np.float32(5.2)      # > |normcdfinv(1e-7)| = 5.1993
EST_MARGIN = 1               # symbols: the estimate's float32 evaluation against this one
TABLE_MARGIN = 2             # symbols: the floors of the coder between the symbol's interval and p


def _clamp(v, lo, hi):
    return np.maximum(lo, np.minimum(v, hi))


def window_start(pos, max_symbol, width, back):
    """s0 (width 16, back 7) or w0 (width 64, back 31) of a window put at `pos`."""
    pos = np.asarray(pos, dtype=np.int64)
    if max_symbol <= width - 1:
        return np.zeros_like(pos)
    return _clamp(pos - back, 0, max_symbol - (width - 1))


def window_hit(start, s, max_symbol, width):
    """The acceptance rule of tiers 1 and 2: s is among the window's first width - 1 candidates, or is its last one and max_symbol."""
    start = np.asarray(start, dtype=np.int64); s = np.asarray(s, dtype=np.int64)
    return ((start <= s) & (s <= start + width - 2)) | ((s == max_symbol) & (s == start + width - 1))


def tier1_hit(centre, s, max_symbol):
    """Exact: tier 1 decodes symbol s of a row whose window is centred on `centre`."""
    return window_hit(window_start(centre, max_symbol, 16, 7), s, max_symbol, 16)


# ------------------------------------------------------------------ centre of the three row kinds
def centre_table(n, max_symbol):
    return np.full(n, max_symbol // 2, dtype=np.int64)


def _sym_of(v, q, min_value):
    """rint(v / q) - min in float32, as an int64 (values beyond int32 saturate like the device's float -> int conversion)."""
    r = np.rint(np.asarray(v, np.float32) / np.asarray(q, np.float32)).astype(np.float64)
    return np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64) - int(min_value)


def centre_gaussian(mean, q, min_value):
    return _sym_of(mean, q, min_value)


def heaviest(probs):
    """Index of the heaviest component per row; strict > from component 0 on, so the FIRST of equal weights."""
    p = np.stack([np.asarray(a, np.float32) for a in probs], 0)
    best = np.zeros(p.shape[1], dtype=np.int64)
    for i in range(1, p.shape[0]):
        best = np.where(p[i] > p[best, np.arange(p.shape[1])], i, best)
    return best


def heaviest_component(means, scales, probs):
    best = heaviest(probs)
    rows = np.arange(best.size)
    m = np.stack([np.asarray(a, np.float32) for a in means], 0)[best, rows]
    sc = np.stack([np.asarray(a, np.float32) for a in scales], 0)[best, rows]
    return m, sc


def centre_mixture(means, scales, probs, q, min_value):
    m, _ = heaviest_component(means, scales, probs)
    return centre_gaussian(m, q, min_value)


# ------------------------------------------------------------------ estimate intervals
def estimate_bounds_gaussian(mean, scale, q, min_value):
    """[lo, hi] that holds every estimate of a Gaussian row, margin included."""
    mean = np.asarray(mean, np.float32); q = np.asarray(q, np.float32)
    sc = np.maximum(np.asarray(scale, np.float32), np.float32(1e-9))
    return _sym_of(mean - Z_MAX * sc, q, min_value) - EST_MARGIN, _sym_of(mean + Z_MAX * sc, q, min_value) + EST_MARGIN


def integerise(cdf):
    """The coder's integers of a float table: rint(cdf * (65536 - (lp - 1))) + index, the last entry 65536."""
    cdf = np.asarray(cdf, np.float32)
    lp = cdf.shape[1]
    c = np.rint(cdf * np.float32(65536 - (lp - 1))).astype(np.int64) + np.arange(lp, dtype=np.int64)[None, :]
    c[:, lp - 1] = 65536
    return c


def estimate_bounds_table(cdf_int, s, max_symbol):
    """[lo, hi] that holds every estimate int(p * max_symbol) of a table row coding symbol s: p lies in the symbol's interval [lo, hi) / 65536."""
    c = np.asarray(cdf_int, np.int64)
    rows = np.arange(c.shape[0])
    s = np.asarray(s, np.int64)
    c_lo = c[rows, s]
    c_hi = np.where(s == max_symbol, 65536, c[rows, np.minimum(s + 1, c.shape[1] - 1)])
    return c_lo * max_symbol // 65536 - TABLE_MARGIN, -(-c_hi * max_symbol // 65536) + TABLE_MARGIN


# ------------------------------------------------------------------ the certain tier
def certain_tier(centre, est_lo, est_hi, s, max_symbol):
    """1, 2 or 3 where every estimate in [est_lo, est_hi] sends symbol s to that tier, 0 where the estimates disagree."""
    s = np.asarray(s, np.int64)
    t1 = tier1_hit(centre, s, max_symbol)
    w_lo = window_start(est_lo, max_symbol, 64, 31)
    w_hi = window_start(est_hi, max_symbol, 64, 31)
    # the starts that accept s form one interval, so both ends inside it means all inside; all outside: the intervals are disjoint
    all_hit = window_hit(w_lo, s, max_symbol, 64) & window_hit(w_hi, s, max_symbol, 64)
    none_hit = (s < w_lo) | (s - 62 - (s == max_symbol) > w_hi)          # below every window, or past every window's last accepted candidate
    return np.where(t1, 1, np.where(all_hit, 2, np.where(none_hit, 3, 0))).astype(np.int64)


def tier2_certain(centre, est_lo, est_hi, s, max_symbol):
    return certain_tier(centre, est_lo, est_hi, s, max_symbol) == 2


def tier3_certain(centre, est_lo, est_hi, s, max_symbol):
    return certain_tier(centre, est_lo, est_hi, s, max_symbol) == 3


def tiers_gaussian(mean, scale, q, min_value, s, max_symbol):
    lo, hi = estimate_bounds_gaussian(mean, scale, q, min_value)
    return certain_tier(centre_gaussian(mean, q, min_value), lo, hi, s, max_symbol)


def tiers_mixture(means, scales, probs, q, min_value, s, max_symbol):
    m, sc = heaviest_component(means, scales, probs)
    return tiers_gaussian(m, sc, q, min_value, s, max_symbol)


def tiers_table(cdf, s, max_symbol):
    """cdf: the float table (integerised here) or an integer table as the uint16 coder takes it."""
    cdf = np.asarray(cdf)
    c = integerise(cdf) if cdf.dtype.kind == "f" else cdf.astype(np.int64) & 0xFFFF
    lo, hi = estimate_bounds_table(c, s, max_symbol)
    return certain_tier(centre_table(c.shape[0], max_symbol), lo, hi, s, max_symbol)
