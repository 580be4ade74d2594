"""Inputs of the attribute coder's tier tests, shared by tests/test_hac_tier_ref_cpu.py (the oracle alone) and
tests/test_gpu_attr_coder_tiers.py (the device against the oracle): the same arrays on both sides.

Every x is k * q with an integer k and a q of few mantissa bits, so round(x / q) == k exactly in float32 on every machine, and every mean is
(c + f) * q with |f| <= 0.3, so rint(mean / q) == c whatever the last bit of the division.  A case states its CONDITIONS in `expect`;
check_static / check_cnt assert them from the inputs and the oracle's byte counts, never from the code under test.
"""
import numpy as np

from . import hac_tier_ref as tr

QS = np.array([0.5, 1.0, 2.0, 0.75, 1.25], np.float32)


class Case:
    """kind 'gauss': mean, scale, q, x.  'mix': lists mean / scale / prob, q, x.  'table': cdf (float32, n x lp), sym."""

    def __init__(self, name, kind, chunk, expect, **arrays):
        self.name, self.kind, self.chunk, self.expect = name, kind, int(chunk), dict(expect)
        self.mean = self.scale = self.prob = self.q = self.x = self.cdf = self.sym = None
        for k, v in arrays.items():
            setattr(self, k, v)

    @property
    def n(self):
        return int(self.sym.size if self.kind == "table" else self.x.size)

    def __repr__(self):
        return f"Case({self.name})"


def symbols(case):
    """(sym int16, min, max): what every coder here derives from x -- round(x / q) in float32, half to even."""
    if case.kind == "table":
        return case.sym, 0, case.cdf.shape[1] - 2
    xi = np.rint(case.x / case.q).astype(np.int64)
    mn, mx = int(xi.min()), int(xi.max())
    return (xi - mn).astype(np.int16), mn, mx


def oracle_table(orc, case):
    if case.kind == "table":
        return case.cdf
    _, mn, mx = symbols(case)
    if case.kind == "gauss":
        return orc.gaussian_cdf(case.mean, case.scale, case.q, mn, mx)
    return orc.gaussian_mixed_cdf(case.mean, case.scale, case.prob, case.q, mn, mx)


def tiers(case):
    """The certain tier of every symbol (0: unknown), from the inputs alone."""
    sym, mn, mx = symbols(case)
    s, m = sym.astype(np.int64), mx - mn
    if case.kind == "table":
        return tr.tiers_table(case.cdf, s, m)
    if case.kind == "gauss":
        return tr.tiers_gaussian(case.mean, case.scale, case.q, mn, s, m)
    return tr.tiers_mixture(case.mean, case.scale, case.prob, case.q, mn, s, m)


def centres(case):
    sym, mn, mx = symbols(case)
    if case.kind == "table":
        return tr.centre_table(case.n, mx - mn)
    if case.kind == "gauss":
        return tr.centre_gaussian(case.mean, case.q, mn)
    return tr.centre_mixture(case.mean, case.scale, case.prob, case.q, mn)


def chunk_lengths(n, chunk):
    return [min(chunk, n - c) for c in range(0, n, chunk)]


def check_static(case):
    """The conditions a case states about its inputs.  Returns the tier array."""
    e = case.expect
    sym, mn, mx = symbols(case)
    m = mx - mn
    assert int(sym.min()) == 0 and int(sym.max()) == m
    if "max_symbol" in e:
        assert m == e["max_symbol"], (case, m)
    if "min_max_symbol" in e:
        assert m >= e["min_max_symbol"], (case, m)
    t = tiers(case)
    for tier, frac in e.get("tier_min", {}).items():
        got = float(np.mean(t == tier))
        assert got >= frac, f"{case}: {got:.3f} of the symbols are certain in tier {tier}, {frac} wanted"
    if "tier1_miss_min" in e:
        miss = 1.0 - float(np.mean(tr.tier1_hit(centres(case), sym.astype(np.int64), m)))
        assert miss >= e["tier1_miss_min"], f"{case}: tier 1 misses {miss:.3f} of the symbols"
    if e.get("interleaved"):
        # one pass of the decoder serves four rows of a chunk: every full group of four holds at least two different certain tiers
        for c0 in range(0, case.n, case.chunk):
            tc = t[c0:c0 + case.chunk]
            g = tc[:tc.size // 4 * 4].reshape(-1, 4)
            distinct = np.array([len(set(row[row > 0].tolist())) for row in g])
            assert distinct.size == 0 or distinct.min() >= 2, f"{case}: a group of four rows with one tier only (chunk at {c0})"
    if "chunk_lengths" in e:
        assert set(e["chunk_lengths"]) <= set(chunk_lengths(case.n, case.chunk)), (case, chunk_lengths(case.n, case.chunk))
    return t


def check_cnt(case, cnt):
    """The conditions a case states about the ORACLE's chunk byte counts."""
    e = case.expect
    cnt = np.asarray(cnt, np.int64)
    lens = np.array(chunk_lengths(case.n, case.chunk), np.int64)
    assert cnt.size == lens.size
    assert np.all(cnt >= 1) and np.all(cnt <= 2 * lens + 32), f"{case}: a chunk beyond the encoder's 2 * symbols + 32 scratch bytes"
    if "pure_chunks" in e:
        idx, bound = e["pure_chunks"]
        assert int(cnt[list(idx)].max()) <= bound, (case, cnt)
    if e.get("worst_rate"):
        assert cnt.size == 1 and 16 * case.n <= 8 * int(cnt[0]) <= 16 * case.n + 256, (case, cnt)
    if "every_chunk_over" in e:
        assert int(cnt.min()) > e["every_chunk_over"], (case, cnt)


def check_residues(cnts):
    """Bit-reader edges over a set of high-rate streams: every length of the last, partial word, and block crossings."""
    cnt = np.concatenate([np.asarray(c, np.int64) for c in cnts])
    assert set((cnt % 4).tolist()) == {0, 1, 2, 3}, cnt
    assert int(cnt.max()) > 512 and np.any((cnt > 256))


# ------------------------------------------------------------------ generators
def _mean_of(centre_abs, q, rng):
    """(c + f) * q, |f| <= 0.3: rint(mean / q) == c."""
    return ((centre_abs.astype(np.float64) + rng.uniform(-0.3, 0.3, centre_abs.size)) * q.astype(np.float64)).astype(np.float32)


def _x_of(k_abs, q):
    return (k_abs.astype(np.float32) * q).astype(np.float32)          # exact: few bits times few bits


def _q(n, rng):
    return QS[rng.randint(0, QS.size, n)]


def gauss_narrow(seed=1, n=6000, chunk=2500, m=300, mn=-150):
    """a. narrow Gaussian rows (scale / q in {0, 0.25, 0.5, 1}), x placed by tier: |s - centre| <= 7, 8..25, >= 40 on both sides, at 0 and max_symbol;
    rows cycle tier 1, 2, 3 so every pass of four rows mixes them."""
    rng = np.random.RandomState(seed)
    q = _q(n, rng)
    c = rng.randint(70, m - 70 + 1, n)
    i = np.arange(n)
    sign = np.where(rng.rand(n) < 0.5, -1, 1)
    d = np.where(i % 3 == 0, rng.randint(-7, 8, n), np.where(i % 3 == 1, sign * rng.randint(8, 26, n), sign * rng.randint(40, 70, n)))
    s = c + d
    s[2], s[5] = 0, m                                                   # two tier-3 slots: the ends of the alphabet
    s[8], s[11] = m, 0
    scale = (np.array([0.0, 0.25, 0.5, 1.0], np.float32)[(i // 3) % 4] * q).astype(np.float32)
    return Case(f"gauss_narrow_min{mn}", "gauss", chunk, dict(max_symbol=m, tier_min={1: 0.2, 2: 0.2, 3: 0.2}, interleaved=True),
                mean=_mean_of(c + mn, q, rng), scale=scale, q=q, x=_x_of(s + mn, q))


def gauss_clamped(seed=2, n=6000, chunk=2500, m=300, mn=5000):
    """a. the mean far outside [min, max] on either side: both clamps of s0 and of w0 saturate (windows at 0 and at max_symbol - 15 / - 63)."""
    rng = np.random.RandomState(seed)
    q = _q(n, rng)
    i = np.arange(n)
    below = (i // 3) % 2 == 0                                           # the mean lies below min: windows start at 0
    c = np.where(below, rng.randint(-5200, -4800, n), rng.randint(5400, 5800, n)) + m // 2
    lo_s = np.where(i % 3 == 0, rng.randint(0, 15, n), np.where(i % 3 == 1, rng.randint(15, 63, n), rng.randint(64, m + 1, n)))
    hi_s = np.where(i % 3 == 0, rng.randint(m - 15, m + 1, n), np.where(i % 3 == 1, rng.randint(m - 63, m - 15, n), rng.randint(0, m - 63, n)))
    s = np.where(below, lo_s, hi_s)
    s[0], s[3] = 0, m
    scale = (np.array([0.0, 0.25, 0.5, 1.0], np.float32)[(i // 3) % 4] * q).astype(np.float32)
    return Case(f"gauss_clamped_min{mn}", "gauss", chunk, dict(max_symbol=m, tier_min={1: 0.2, 2: 0.2, 3: 0.2}, interleaved=True),
                mean=_mean_of(c + mn, q, rng), scale=scale, q=q, x=_x_of(s + mn, q))


def gauss_wide(seed=3, n=5000, chunk=1700, ratio=50.0, name="gauss_wide", expect=None):
    """a. the scaling attribute's shape: scale / q about `ratio`, x drawn from the row's own distribution; the quantile estimate carries the decode."""
    rng = np.random.RandomState(seed)
    q = _q(n, rng)
    c = rng.randint(-30, 31, n)
    mean = _mean_of(c, q, rng)
    scale = (q * (ratio * rng.uniform(0.8, 1.2, n))).astype(np.float32)
    k = np.rint((mean.astype(np.float64) + scale.astype(np.float64) * rng.randn(n)) / q.astype(np.float64)).astype(np.int64)
    expect = dict(min_max_symbol=400, tier1_miss_min=0.5) if expect is None else expect
    return Case(name, "gauss", chunk, expect, mean=mean, scale=scale, q=q, x=_x_of(k, q))


def mixture(k, seed=4, n=4500, chunk=2000, m=400, mn=-200):
    """b. symbols from a light component whose mean is >= 100 symbols from the heaviest one's: centre and estimate point at the wrong component.
    Every fifth row has two exactly equal largest weights (components 0 and 1: the decoder takes component 0) and codes from component 1."""
    rng = np.random.RandomState(seed + k)
    q = _q(n, rng)
    i = np.arange(n)
    tie = i % 5 == 0
    heavy = np.where(tie, 0, i % k)
    weights = {2: [0.7, 0.3], 3: [0.5, 0.3, 0.2], 4: [0.4, 0.3, 0.2, 0.1]}[k]
    tied = {2: [0.5, 0.5], 3: [0.4, 0.4, 0.2], 4: [0.3, 0.3, 0.2, 0.2]}[k]
    prob = np.zeros((k, n), np.float32)
    centre = np.zeros((k, n), np.int64)
    ch = rng.randint(150, 251, n)
    sign = np.where(rng.rand(n) < 0.5, -1, 1)
    for r in range(n):
        if tie[r]:
            prob[:, r] = tied
        else:
            rest = [j for j in range(k) if j != heavy[r]]
            prob[heavy[r], r] = weights[0]
            prob[rest, r] = weights[1:]
    for j in range(k):
        off = sign * (100 + 10 * j + rng.randint(0, 20, n)) * np.where(j % 2 == 0, 1, -1)
        centre[j] = np.where(heavy == j, ch, np.clip(ch + off, 8, m - 8))
    light = np.where(tie, 1, (heavy + 1 + rng.randint(0, k - 1, n)) % k)
    from_heavy = (i % 3 == 2) & ~tie
    comp = np.where(from_heavy, heavy, light)
    s = centre[comp, i] + np.where(from_heavy, rng.randint(-3, 4, n), rng.randint(-1, 2, n))
    s[1], s[4] = 0, m
    ratio = np.where(np.arange(k)[:, None] == heavy[None, :], rng.choice([0.5, 1.0, 2.0], (k, n)), rng.choice([0.25, 0.5, 1.0], (k, n)))
    return Case(f"mixture_k{k}", "mix", chunk, dict(max_symbol=m, tier_min={3: 0.2}, ties=True),
                mean=[_mean_of(centre[j] + mn, q, rng) for j in range(k)], scale=[(ratio[j] * q).astype(np.float32) for j in range(k)],
                prob=[prob[j].copy() for j in range(k)], q=q, x=_x_of(s + mn, q))


def skewed_table(lp, seed=5, n=3000, chunk=1300):
    """c. generic tables whose estimate p * max_symbol is more than 40 symbols from the coded one: all mass in the last (first) three symbols,
    the coded symbol mid-row.  Rows cycle tail-heavy, head-heavy, peaked at the middle (tier 1) and uniform."""
    rng = np.random.RandomState(seed + lp)
    m = lp - 2
    i = np.arange(n)
    pmf = np.full((n, lp - 1), 1e-9)
    kind = i % 4
    pmf[kind == 0, -3:] = 1.0 / 3
    pmf[kind == 1, :3] = 1.0 / 3
    idx = np.arange(lp - 1)
    pmf[kind == 2] = np.exp(-0.5 * ((idx[None, :] - m // 2) / 3.0) ** 2) + 1e-9
    pmf[kind == 3] = 1.0
    pmf /= pmf.sum(1, keepdims=True)
    cdf = np.concatenate([np.zeros((n, 1)), np.cumsum(pmf, 1)], 1).clip(0, 1).astype(np.float32)
    cdf[:, -1] = 1.0
    if lp == 100:
        tail, head = rng.randint(66, 91, n), rng.randint(8, 31, n)
    else:
        mid = np.where(rng.rand(n) < 0.5, rng.randint(100, 481, n), rng.randint(520, 901, n))
        tail = head = mid
    s = np.where(kind == 0, tail, np.where(kind == 1, head, np.where(kind == 2, m // 2 + rng.randint(-5, 6, n), rng.randint(0, m + 1, n))))
    s[2], s[3] = m, 0
    return Case(f"table_lp{lp}", "table", chunk, dict(max_symbol=m, tier_min={3: 0.2}), cdf=cdf, sym=s.astype(np.int16))


BOUNDARY_M = (0, 1, 14, 15, 16, 17, 62, 63, 64, 65, 200, 4000, 32765)
BOUNDARY_M_MIX = (15, 16, 63, 64, 4000)


def boundary(m, mixed=False, seed=6):
    """d. max_symbol = m exactly (one element at min, one at max).  Even rows have scale 0, where estimate == centre and so s0 AND w0 are known:
    they code 0, 1, m - 1, m, s0 + 14, s0 + 15, w0 + 62, w0 + 63 in turn (where the alphabet has them); odd rows are wide, symbols uniform."""
    rng = np.random.RandomState(seed + m)
    n = 300 if m > 4000 else 600
    chunk = 100 if m > 4000 else 250
    mn = -(m // 3)
    q = _q(n, rng)
    i = np.arange(n)
    c = rng.randint(0, m + 1, n)
    s0 = tr.window_start(c, m, 16, 7)
    w0 = tr.window_start(c, m, 64, 31)
    special = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, m - 1), np.full(n, m), s0 + 14, s0 + 15, w0 + 62, w0 + 63])
    pick = special[(i // 2) % 8, i]
    rand = rng.randint(0, m + 1, n)
    s = np.where((i % 2 == 0) & (pick >= 0) & (pick <= m), pick, rand)
    s[1], s[3] = 0, m
    scale = np.where(i % 2 == 0, 0.0, q * (0.3 + rng.rand(n) * m / 4.0)).astype(np.float32)
    mean = _mean_of(c + mn, q, rng)
    x = _x_of(s + mn, q)
    if not mixed:
        return Case(f"boundary_m{m}", "gauss", chunk, dict(max_symbol=m), mean=mean, scale=scale, q=q, x=x)
    c2 = rng.randint(0, m + 1, n)
    w = np.where(i % 4 < 2, 0.6, 0.4).astype(np.float32)
    return Case(f"boundary_mix_m{m}", "mix", chunk, dict(max_symbol=m), mean=[mean, _mean_of(c2 + mn, q, rng)],
                scale=[scale, (q * rng.choice([0.0, 0.5, 2.0], n)).astype(np.float32)], prob=[w, (np.float32(1) - w).astype(np.float32)], q=q, x=x)


CHUNK_SHAPES = ((7, 1), (5, 2), (7, 3), (9, 4), (13, 5), (130, 63), (129, 64), (132, 65), (139, 67), (257, 128), (263, 129), (77, 1000))


def chunk_shape(n, chunk, wide, seed=7):
    """f. chunks of 1, 2, 3, 4, 5, 63, 64, 65, 67, 128 and 129 symbols over CHUNK_SHAPES (chunk = 1: one chunk per symbol; a last chunk of one symbol;
    chunk > n), on an alphabet wider than 64 (wide rows) and on one of 15 symbols."""
    rng = np.random.RandomState(seed)
    lens = set(chunk_lengths(n, chunk))
    if wide:
        base = gauss_wide(seed, 263, chunk)
        x = base.x[:n].copy()
        x[0], x[1] = -100 * base.q[0], 100 * base.q[1]
        return Case(f"chunks_wide_n{n}_c{chunk}", "gauss", chunk, dict(min_max_symbol=65, chunk_lengths=lens), mean=base.mean[:n], scale=base.scale[:n],
                    q=base.q[:n], x=x)
    q = _q(n, rng)
    c = rng.randint(0, 15, n)
    s = np.clip(c + rng.randint(-2, 3, n), 0, 14)
    s[0], s[1] = 0, 14
    return Case(f"chunks_small_n{n}_c{chunk}", "gauss", chunk, dict(max_symbol=14, chunk_lengths=lens), mean=_mean_of(c - 7, q, rng),
                scale=(q * rng.choice([0.0, 0.5, 1.5], n)).astype(np.float32), q=q, x=_x_of(s - 7, q))


def high_rate(chunk, n, seed):
    """g. about 10 bits per symbol (scale / q about 300): chunks of 900 .. 2 600 bytes cross the bit reader's 256-byte blocks several times."""
    return gauss_wide(seed, n, chunk, ratio=300.0, name=f"high_rate_c{chunk}", expect=dict(min_max_symbol=1500, every_chunk_over=512))


def high_rate_streams():
    return [high_rate(700, 9 * 700 + 411, 8), high_rate(2000, 3 * 2000 + 1300, 9)]


def near_zero_rate(seed=10, n=30000, chunk=10000, m=100):
    """g. scale = 0 and every x on its mean: the pure chunks (the first and the last) cost a few bytes; the alphabet is wider than 64 only because of
    two outliers in the middle chunk."""
    rng = np.random.RandomState(seed)
    q = _q(n, rng)
    c = rng.randint(20, 81, n)
    s = c.copy()
    s[15000], s[15001] = 0, m
    return Case("near_zero_rate", "gauss", chunk, dict(max_symbol=m, pure_chunks=((0, 2), 8)), mean=_mean_of(c - 50, q, rng), scale=np.zeros(n, np.float32), q=q,
                x=_x_of(s - 50, q))


def worst_rate(seed=11, n=10000, m=40):
    """h. one chunk in which every symbol has the smallest interval the format has (hi == lo + 1, 16 bits): scale = 0, x >= 3 symbols off its mean."""
    rng = np.random.RandomState(seed)
    q = _q(n, rng)
    c = rng.randint(0, m + 1, n)
    d = rng.randint(3, 20, n)
    s = np.where(c + d <= m, c + d, c - d)
    s = np.where(s < 0, c + 3, s)
    s[0], s[1] = 0, m
    c[0], c[1] = 10, 20
    return Case("worst_rate", "gauss", n, dict(max_symbol=m, worst_rate=True), mean=_mean_of(c - 20, q, rng), scale=np.zeros(n, np.float32), q=q, x=_x_of(s - 20, q))


SLICE_M = (0, 15, 16, None, 63, 64, 3000)            # None: an empty slice
SLICE_LEN = (1, 10001, 37, 0, 2500, 10064, 4000)      # 10 000-symbol chunks: 1 / 2 (the second: one symbol) / 1 / 0 / 1 / 2 / 1


def slices(seed=12):
    """i. slices with max_symbol 0, 15, 16, 63, 64 and 3000 (and an empty one) for ONE call of the slices coder; returns (bounds, [Case per slice]).
    Component 2 of the mixed form rides along in case.mean2 / scale2 / prob (weights 0.6 / 0.4, the heavy one alternating)."""
    bounds, cases = [0], []
    for j, (m, ln) in enumerate(zip(SLICE_M, SLICE_LEN)):
        bounds.append(bounds[-1] + ln)
        if not ln:
            cases.append(None)
            continue
        rng = np.random.RandomState(seed + j)
        q = _q(ln, rng)
        i = np.arange(ln)
        mn = 40 * j - 100
        if m > 64:
            c = rng.randint(100, m - 100 + 1, ln)
            sign = np.where(rng.rand(ln) < 0.5, -1, 1)
            s = c + np.where(i % 2 == 0, rng.randint(-7, 8, ln), sign * rng.randint(40, 100, ln))
            ratio = rng.choice([0.0, 0.5, 1.0], ln)
            expect = dict(max_symbol=m, tier_min={3: 0.2})
        else:
            c = rng.randint(0, m + 1, ln)
            s = rng.randint(0, m + 1, ln)
            ratio = rng.choice([0.0, 0.5, 2.0], ln)
            expect = dict(max_symbol=m)
        if ln > 1:
            s[0], s[ln - 1] = 0, m
        case = Case(f"slice{j}_m{m}", "gauss", 10000, expect, mean=_mean_of(c + mn, q, rng), scale=(ratio * q).astype(np.float32), q=q, x=_x_of(s + mn, q))
        case.mean2 = _mean_of(rng.randint(0, m + 1, ln) + mn, q, rng)
        case.scale2 = (q * rng.choice([0.25, 1.0], ln)).astype(np.float32)
        w = np.where(i % 2 == 0, 0.6, 0.4).astype(np.float32)
        case.prob = [w, (np.float32(1) - w).astype(np.float32)]
        cases.append(case)
    return bounds, cases


def as_mixture(case):
    """The two-component form of a slice case (kind 'mix')."""
    return Case(case.name + "_mix", "mix", case.chunk, case.expect, mean=[case.mean, case.mean2],
                scale=[case.scale, case.scale2], prob=case.prob, q=case.q, x=case.x)


TOO_WIDE_BOUNDS = (0, 200, 500)


def too_wide(n=500, seed=13):
    """e. 32 767 quantised levels (row length 32 768): one more than int16 symbols index.  (x, mean, scale, q, mean2, scale2, prob)"""
    rng = np.random.RandomState(seed)
    q = np.ones(n, np.float32)
    k = rng.randint(-100, 101, n)
    k[250], k[300] = -16383, 16383                     # both in [200, 500): one slice of TOO_WIDE_BOUNDS is too wide, the other is not
    w = np.full(n, 0.5, np.float32)
    return dict(x=_x_of(k, q), mean=np.zeros(n, np.float32), scale=np.full(n, 30.0, np.float32), q=q, mean2=np.full(n, 5.0, np.float32),
                scale2=np.full(n, 2.0, np.float32), prob=[w, w.copy()])
