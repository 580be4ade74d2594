"""The bit-level coder models of tests/rc_carry_ref.py against the oracle, and what the generated lanes reach.

The models are only worth their records if they ARE the oracle's coders: their bytes equal orc.cp_encode / orc.rc_encode on
random rows and on every generated lane, and the oracle's decoders return the symbols.  The rest asserts, from the models'
records, that the generated set holds every carry ripple, flush value and pending run that tests/test_gpu_rc_carry.py is
there to put through the device coders -- conditions of the set, not of any kernel."""
import numpy as np
import pytest

from tests import rc_carry_ref as R

LPS = (3, 5, 17)
CARRY_LENGTHS = (32, 64, 128)
PENDING_LENGTHS = (32, 64)


def _encode(orc, coder, rows, sym):
    return orc.cp_encode(rows, sym) if coder == "carry" else orc.rc_encode(rows, sym)


def _decode(orc, coder, rows, data):
    return orc.cp_decode(rows, data) if coder == "carry" else orc.rc_decode(rows, data)


def _scratch_stride(max_syms):
    """csrc/rc_format.hpp: rc_scratch_stride -- the bytes of a lane's scratch row in the device encoder"""
    return (2 * max_syms + 32 + 15) & ~15


@pytest.fixture(scope="module")
def coded():
    """{(coder, lp, length): [(case, rows, sym, bytes, model)]} of every generated lane"""
    out = {}
    for coder, lengths in (("carry", CARRY_LENGTHS), ("carryless", PENDING_LENGTHS)):
        for lp in LPS:
            for length in lengths:
                out[coder, lp, length] = [(case, rows, sym) + R.model_encode(coder, rows, sym) for case, rows, sym in R.lanes(coder, lp, length)]
    return out


def _all(coded, coder, lp=None):
    return [e for (c, l, _), v in coded.items() if c == coder and lp in (None, l) for e in v]


@pytest.mark.parametrize("coder", ["carry", "carryless"])
@pytest.mark.parametrize("lp", LPS)
def test_models_equal_the_oracle_on_random_rows(orc, coder, lp):
    rs = np.random.RandomState(17 * lp)
    for n in (1, 2, 33, 700):
        rows, sym = R.random_rows(rs, n, lp)
        data, _ = R.model_encode(coder, rows, sym)
        assert data == _encode(orc, coder, rows, sym)
        assert np.array_equal(_decode(orc, coder, rows, data), sym)
    # skewed rows (a few bits per hundred symbols, and sixteen bits for a symbol): the flush and the carries over a long quiet string
    rows = np.zeros((400, lp), np.uint16)
    rows[:, 1:lp - 1] = np.where(np.arange(400)[:, None] % 2 == 0, np.arange(1, lp - 1)[None, :], 65536 - (lp - 2) + np.arange(lp - 2)[None, :])
    for sym in (np.zeros(400, np.uint8), np.full(400, lp - 2, np.uint8), (np.arange(400) % (lp - 1)).astype(np.uint8)):
        data, _ = R.model_encode(coder, rows, sym)
        assert data == _encode(orc, coder, rows, sym)
        assert np.array_equal(_decode(orc, coder, rows, data), sym)


@pytest.mark.parametrize("coder", ["carry", "carryless"])
def test_generated_lanes_equal_the_oracle_and_decode(orc, coded, coder):
    lanes = _all(coded, coder)
    assert len(lanes) >= 100
    for case, rows, sym, data, _ in lanes:
        lp = rows.shape[1]
        assert rows.dtype == np.uint16 and sym.dtype == np.uint8 and int(sym.max()) <= lp - 2
        assert (rows[:, 0] == 0).all() and (rows[:, lp - 1] == 0).all() and (np.diff(rows[:, :lp - 1].astype(np.int64), axis=1) > 0).all(), case
        assert data == _encode(orc, coder, rows, sym), case
        assert np.array_equal(_decode(orc, coder, rows, data), sym), case
        # the device encoder stores whole 32-bit words into a scratch row of rc_scratch_stride(lane length) bytes
        assert (len(data) + 3) // 4 * 4 <= _scratch_stride(len(sym)) - 4, case


def test_generator_is_deterministic():
    a = R.make_lane("carry", 5, 31, 52, "carry", 64, seed=9, interior=True)
    b = R.make_lane("carry", 5, 31, 52, "carry", 64, seed=9, interior=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = R.make_lane("carryless", 17, 1, 33, "one", 32, seed=9, long_n1=True)
    d = R.make_lane("carryless", 17, 1, 33, "one", 32, seed=9, long_n1=True)
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])


def _the_carry(case, model):
    """the one carry of a generated lane that went through the whole run"""
    hits = [c for c in model.carries if c.flipped == case["run"] and c.flush == (case["ending"] == "flush")]
    assert len(hits) == 1, (case, model.carries)
    return hits[0]


@pytest.mark.parametrize("lp", LPS)
def test_every_case_does_what_it_says(coded, lp):
    """carry: one carry through exactly `run` ones, arriving where CARRY_RUNS says; nocarry / flush_keep: no long carry, and
    the run stands in the bytes; flush: q = 4.  Carry-less: `pending` == run at a resolution to the asked bit and n1."""
    for case, rows, sym, data, m in _all(coded, "carry", lp):
        p, t, ending = case["prefix_bits"], case["run"], case["ending"]
        if ending in ("carry", "flush"):
            c = _the_carry(case, m)
            if ending == "carry":
                assert c.pos == (p + 1 + t) % 32 and c.words == (p + 1 + t) // 32, (case, c)
            else:
                assert m.q == 4 and c.pos == (p % 32 + 1 + t) % 32 and c.words * 32 + c.pos == m.nbits - 2, (case, c)
            assert R.longest_one_run(data) < max(t, 20), case
        else:
            assert all(c.flipped < 32 for c in m.carries), (case, m.carries)
            assert R.longest_one_run(data) >= t, case
            assert ending == "nocarry" or m.q < 4
    for case, rows, sym, data, m in _all(coded, "carryless", lp):
        t, ending = case["run"], case["ending"]
        if ending == "flush":
            r = m.resolutions[-1]
            assert r.flush and r.pending == t + 1, (case, r)
        else:
            hits = [r for r in m.resolutions if r.pending == t and not r.flush]
            assert len(hits) == 1 and hits[0].bit == (ending == "one") and (hits[0].n1 > 1) == case["long_n1"], (case, m.resolutions)
            r = hits[0]
        assert (R.longest_zero_run if r.bit else R.longest_one_run)(data) >= t, case     # the bit, then the run of its complement


@pytest.mark.parametrize("lp", LPS)
def test_carry_set_covers_every_ripple_and_arrival(coded, lp):
    lanes = _all(coded, "carry", lp)
    carries = [(case, c) for case, _, _, _, m in lanes for c in m.carries]
    ends = {R.end_word(c) for _, c in carries}
    # ripple length: inside the accumulator, first / second / third stored word, eighth or later
    assert {0, 1, 2, 3} <= ends and max(ends) >= 8
    # ... and ending exactly at a word boundary: the run fills the accumulator and 0, 1, 2 and 7 whole words
    whole = {(c.flipped - c.pos) // 32 for _, c in carries if c.flipped >= c.pos and (c.flipped - c.pos) % 32 == 0 and (c.pos or c.flipped)}
    assert {0, 1, 2, 7} <= whole
    # ... and at a word's first bit (31 ones of that word flip)
    assert {R.end_word(c) for _, c in carries if c.flipped >= c.pos and (c.flipped - c.pos) % 32 == 31} >= {1, 2}
    # arrival position: 0 (the accumulator is empty: straight into the stored words), 1 and 31, each with a walk of two words
    for pos in (0, 1, 31):
        assert any(c.pos == pos and R.end_word(c) >= 2 for _, c in carries), pos
        assert any(c.pos == pos and R.end_word(c) == 1 for _, c in carries) or pos == 1
    # the straddle starts at these offsets
    assert {case["prefix_bits"] for case, c in carries if c.flipped == case["run"] and case["ending"] == "carry"} >= {0, 1, 31, 32, 33}
    # both range branches straddle B: Lp > 3 has lanes whose straddling symbols are interior, and lanes that use the first / last symbol
    if lp > 3:
        assert {case["interior"] for case, c in carries if c.flipped == case["run"] and R.end_word(c) >= 2} == {False, True}


@pytest.mark.parametrize("lp", LPS)
def test_carry_set_covers_every_flush(coded, lp):
    lanes = _all(coded, "carry", lp)
    qs = {m.q for _, _, _, _, m in lanes}
    zeros = R.model_encode("carry", *R.plain_lane(lp, 64, 5, zeros=True))[1]
    assert zeros.q == 0 and qs >= {1, 2, 3, 4}
    flush_carries = [c for _, _, _, _, m in lanes for c in m.carries if c.flush]
    assert any(c.flipped >= 64 and R.end_word(c) >= 2 for c in flush_carries)          # q = 4 behind 64 or more ones
    assert any(R.end_word(c) == 0 for c in flush_carries) and any(c.flipped >= 200 for c in flush_carries)
    # the same runs with no carry at all: ended below B by a symbol, or left standing by a flush with q < 4
    kept = {(case["prefix_bits"], case["run"]) for case, _, _, _, m in lanes if case["ending"] == "nocarry"}
    assert kept == {(case["prefix_bits"], case["run"]) for case, _, _, _, m in lanes if case["ending"] == "carry"}
    assert any(case["ending"] == "flush_keep" and case["run"] >= 64 for case, _, _, _, _ in lanes)


@pytest.mark.parametrize("lp", LPS)
def test_carryless_set_covers_every_pending_run(coded, lp):
    res = [r for _, _, _, _, m in _all(coded, "carryless", lp) for r in m.resolutions]
    for want in (lambda p: p == 31, lambda p: p == 32, lambda p: p == 33, lambda p: p == 64, lambda p: p >= 100):
        for bit in (0, 1):
            assert any(want(r.pending) and r.bit == bit and r.n1 == 1 and not r.flush for r in res)
            assert any(want(r.pending) and r.bit == bit and r.n1 > 1 and not r.flush for r in res)
    # the flush's own run (pending + 1 copies) on either side of a word
    assert {r.pending for r in res if r.flush} >= {32, 33, 34, 65}
    # a word's worth of bits in one put (n1 + pending == 32) and one more (the put_run branch)
    assert {r.n1 + r.pending for r in res if not r.flush} >= {32, 33}
    assert {r.pos for r in res if r.pending >= 31} >= {0, 1, 31}


def test_lane_geometry_restated():
    """csrc/rc_format.hpp: rc_plan.  Versions 3 and 4 at chunk_log2 = 11: 64-symbol lanes up to 16 384 symbols; chunk_log2 = 6:
    32-symbol lanes; 128-symbol lanes from 16 385 to 32 768 symbols with chunk_log2 >= 8."""
    for v in (3, 4):
        assert [R.lane_log2(n, 11, v) for n in (1, 64, 8192, 16384)] == [6] * 4
        assert [R.lane_log2(n, 11, v) for n in (16385, 32768, 32769, 1 << 17, 1 << 20)] == [7, 7, 8, 9, 10]
        assert [R.lane_log2(n, 6, v) for n in (1, 5000, 1 << 20)] == [5] * 3
        assert [R.lane_log2(n, 8, v) for n in (16384, 16385, 32768, 1 << 20)] == [6, 7, 7, 7]
    assert [R.lane_log2(n, 11, 2) for n in (1, 32768, 32769, 1 << 20)] == [7, 7, 8, 11]
    assert R.lane_log2(5000, 10, 1) == 10
