"""The expected `.b` file, put together from the ORACLE coder's output: what tests/test_gpu_attributes.py compares the product's files with
and what tests/test_attr_pins_cpu.py compares with the files the reference's own Python wrote (tests/golden/attr_b_*.npz).

    Gaussian family   f32 min | f32 max | i32 len(cnt bytes) | cnt | payload      HAC/utils/encodings_cuda.py:366-376
    Bernoulli         f32 p | i32 len(cnt bytes) | cnt | payload, every row [0, 1 - p, 1] in float32      :435-464
"""
import numpy as np

CHUNK = 10000


def _tail(cnt, payload):
    return np.array([4 * len(cnt)], np.int32).tobytes() + cnt.astype(np.int32).tobytes() + payload.tobytes()


def gaussian_file(orc, sym, table, mn, mx, chunk=CHUNK):
    """(file bytes, bit count) from int16 symbols and the float32 CDF table they are coded with."""
    payload, cnt = orc.hac_encode(np.ascontiguousarray(sym, dtype=np.int16), np.ascontiguousarray(table, dtype=np.float32), chunk)
    return np.float32(mn).tobytes() + np.float32(mx).tobytes() + _tail(cnt, payload), (len(payload) + 4 * len(cnt)) * 8 + 96


def bernoulli_row(p1):
    return np.array([0.0, np.float32(1) - np.float32(p1), 1.0], np.float32)


def bernoulli_file(orc, xs, p1, chunk=CHUNK):
    """(file bytes, bit count) from the {0, 1} values and the float32 share of ones the reference stores (:440, 456)."""
    xs = np.asarray(xs).reshape(-1)
    cdf = np.tile(bernoulli_row(p1), (xs.size, 1))
    payload, cnt = orc.hac_encode(xs.astype(np.int16), cdf, chunk)
    return np.float32(p1).tobytes() + _tail(cnt, payload), (len(payload) + 4 * len(cnt)) * 8 + 64


def parse_gaussian(blob):
    """(min, max, cnt int32, payload uint8) of a Gaussian-family file."""
    blob = bytes(blob)
    mn, mx = (float(v) for v in np.frombuffer(blob[:8], np.float32))
    lc = int(np.frombuffer(blob[8:12], np.int32)[0])
    return mn, mx, np.frombuffer(blob[12:12 + lc], np.int32), np.frombuffer(blob[12 + lc:], np.uint8)


def parse_bernoulli(blob):
    """(p, cnt int32, payload uint8) of a Bernoulli file."""
    blob = bytes(blob)
    lc = int(np.frombuffer(blob[4:8], np.int32)[0])
    return np.frombuffer(blob[:4], np.float32)[0], np.frombuffer(blob[8:8 + lc], np.int32), np.frombuffer(blob[8 + lc:], np.uint8)
