"""The device range coders on the lanes that random data never produces (tests/rc_carry_ref.py; what the set holds is
asserted, without a GPU, in tests/test_rc_carry_ref_cpu.py).

Version 4 (k_rc_encode<RC_CODER_CARRY>): carries that ripple out of the writer's accumulator through one, two, three and
eight of the 32-bit words already stored, that end on a word's last and first bit, that arrive with the accumulator empty,
and the flush's own carry (q = 4) through such a run -- each lane once coded forwards (an even lane of its stream) and once
backwards (an odd lane: its bytes reversed).  Versions 1-3 and the reference layout (RC_CODER_CARRYLESS): pending runs of
31, 32, 33, 64 and 100 bits resolved to 0 and to 1, and left to the flush.  The staged decoders thereby read 0111...1 /
1000...0 strings in both directions.  Every comparison is byte- or symbol-exact against the oracle."""
import numpy as np
import pytest

from tests import rc_carry_ref as R

pytestmark = pytest.mark.gpu

LPS = (3, 5, 17)
CHUNK_LOG2_OF = {32: 6, 64: 11}          # (lane length: the chunk_log2 that gives it in a stream of up to 16 384 symbols)


@pytest.fixture(scope="module")
def gh():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: the HIP path has no fallback")
    from tests import gpu_helpers

    return gpu_helpers


def _cat(entries):
    return np.concatenate([e[-2] for e in entries]), np.concatenate([e[-1] for e in entries])


def _lane_bytes(orc, rows, sym, llog, version):
    """the oracle's bytes of every lane of a stream on its own (to name the lane a differing stream differs in)"""
    S = 1 << llog
    enc = orc.cp_encode if version >= 4 else orc.rc_encode
    return [enc(rows[i:i + S], sym[i:i + S]) for i in range(0, len(sym), S)]


def _check_stream(gh, orc, rows, sym, chunk_log2, version, lane_len):
    """bytes == the oracle's stream, the oracle decodes the device's bytes, the device decodes them"""
    assert 1 << R.lane_log2(len(sym), chunk_log2, version) == lane_len
    data = gh.rc_encode(rows, sym, chunk_log2, version)
    ref = orc.stream_encode(rows, sym, chunk_log2, version)
    if data != ref:
        at = next((i for i, (a, b) in enumerate(zip(data, ref)) if a != b), min(len(data), len(ref)))
        lens = np.cumsum([0] + [len(b) for b in _lane_bytes(orc, rows, sym, R.lane_log2(len(sym), chunk_log2, version), version)])
        lane = int(np.searchsorted(lens, at - (len(ref) - lens[-1]), side="right")) - 1
        pytest.fail(f"first differing byte at {at} of {len(data)} / {len(ref)}: lane {lane} of {len(lens) - 1}")
    assert np.array_equal(orc.stream_decode(rows, data, chunk_log2, version), sym)
    assert np.array_equal(gh.rc_decode(rows, data, chunk_log2, version), sym)


def _both_ways(coder, lp, length, extra=()):
    filler = lambda: R.plain_lane(lp, length, 77)
    return _cat(R.both_ways([l[1:] for l in R.lanes(coder, lp, length)] + list(extra), filler))


@pytest.mark.parametrize("length", [64, 32])
@pytest.mark.parametrize("lp", LPS)
def test_carry_lanes_forwards_and_backwards(gh, orc, lp, length):
    """every generated version-4 lane of 64 (32) symbols, and a lane whose flush has q = 0, on an even and on an odd slot"""
    rows, sym = _both_ways("carry", lp, length, [R.plain_lane(lp, length, 5, zeros=True)])
    assert len(sym) <= 16384
    _check_stream(gh, orc, rows, sym, CHUNK_LOG2_OF[length], 4, length)


@pytest.mark.parametrize("lp", LPS)
def test_carry_ripples_through_eight_stored_words(gh, orc, lp):
    """128-symbol lanes (a stream of 16 385 to 32 768 symbols at chunk_log2 >= 8) hold runs of 240 to 300 ones: a carry wraps
    seven whole words and more.  Plain lanes fill the stream up; the last lane is short."""
    head = _cat(R.both_ways([l[1:] for l in R.lanes("carry", lp, 128)], lambda: R.plain_lane(lp, 128, 78)))
    tail = R.plain_lane(lp, 16384 + 128 + 57 - len(head[1]), 79)
    rows, sym = np.concatenate([head[0], tail[0]]), np.concatenate([head[1], tail[1]])
    _check_stream(gh, orc, rows, sym, 8, 4, 128)


@pytest.mark.parametrize("length", [64, 32])
@pytest.mark.parametrize("lp", LPS)
def test_pending_lanes_forwards_and_backwards(gh, orc, lp, length):
    """the carry-less coder in the lanes of a version-3 stream: every pending-run lane on an even and on an odd slot"""
    rows, sym = _both_ways("carryless", lp, length)
    assert len(sym) <= 16384
    _check_stream(gh, orc, rows, sym, CHUNK_LOG2_OF[length], 3, length)


@pytest.mark.parametrize("lp", LPS)
def test_pending_lanes_in_the_reference_layout(gh, orc, lp):
    """chunk_log2 = 0: one carry-less lane per stream, the bare coder bytes"""
    for case, rows, sym in R.lanes("carryless", lp, 64) + R.lanes("carryless", lp, 32):
        data = gh.rc_encode(rows, sym, 0)
        assert data == orc.rc_encode(rows, sym), case
        assert data == orc.stream_encode(rows, sym, 0), case
        assert np.array_equal(orc.rc_decode(rows, data), sym), case
        assert np.array_equal(gh.rc_decode(rows, data, 0), sym), case


@pytest.mark.parametrize("version", [4, 3])
@pytest.mark.parametrize("lp", LPS)
def test_adversarial_and_plain_lanes_share_a_wave(gh, orc, lp, version):
    """Two waves of 64-symbol lanes in which every third lane is a generated one and the rest seeded filler (the lanes of a
    wave run in lockstep: the long walks diverge from their neighbours), ending on a short last lane that still holds a run."""
    gen = R.lanes("carry" if version == 4 else "carryless", lp, 64)
    entries = [gen[(i // 3) % len(gen)][1:] if i % 3 == 0 else R.plain_lane(lp, 64, 300 + i) for i in range(72)]
    short = gen[8 if version == 4 else 12]            # (31, 84) carry: the run and its carry stand in the first symbols / pending 64
    n_short = 23
    data, m = R.model_encode("carry" if version == 4 else "carryless", short[1][:n_short], short[2][:n_short])
    assert (max(c.flipped for c in m.carries) if version == 4 else max(r.pending for r in m.resolutions)) >= 64
    entries.append((short[1][:n_short], short[2][:n_short]))
    rows, sym = _cat(entries)
    assert len(sym) == 72 * 64 + n_short
    _check_stream(gh, orc, rows, sym, 11, version, 64)
