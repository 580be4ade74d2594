"""The project's own restatement of the tri-plane latent bitstream (gauspcc_amd/arm_codec.py), in numpy float64 and
plain Python: quantised parameters, integer CDF rows, chunk order, header, ideal size and the size bound.  Bytes come from the
library's host coder (gsac_host_encode_u16), which needs no GPU.

  mu_q = rint(16 mu) / 16, s_q = max(rint(16 s) / 16, 1 / 16)            (float32, as the coder's kernels form them)
  A = ceil(max |y|) + 2, L = 2 A + 1 symbols, index y + A
  row: e_0 = 0, e_L = 1, e_j = F(j - A - 0.5), F(t) = 0.5 - 0.5 sign(t - mu_q) expm1(-|t - mu_q| / s_q); entry = rint(e_j (65536 - L)) + j mod 2^16
  chunk (c, k): channel c, columns k S .. min(W, (k + 1) S) - 1, symbols by row then column; chunks in (channel, strip) order
"""
import ctypes
import struct

import numpy as np
import torch

from tests import arm_ref

QUANT = 16
MAGIC, VERSION = b"GSAL", 1


def make_arm(layers, seed, mu_bias=0.0, ls_pin=None, spread=1.5):
    """An ArmMLP (CPU) with random weights: hidden layers N(0, 0.3) (a residual block gets them too), the mu row N(0, 0.1), the ls row
    N(0, spread) so that s = exp(-ls / 2) runs over the whole clamp range [1e-3, 148] for integer contexts of a few units.
    ls_pin: the ls row is zero and its bias this value (+-20: either clamp end).  mu_bias: added to mu's bias."""
    from gauspcc_amd.arm import ArmMLP

    g = torch.Generator().manual_seed(seed)
    arm = ArmMLP(12, layers)
    lin = arm.linears()
    with torch.no_grad():
        for m in lin[:-1]:
            m.w.copy_(torch.randn(m.w.shape, generator=g) * 0.3)
            m.b.copy_(torch.randn(m.b.shape, generator=g) * 0.3)
        out = lin[-1]
        out.w[0].copy_(torch.randn(out.w.shape[1], generator=g) * 0.1)
        out.w[1].copy_(torch.randn(out.w.shape[1], generator=g) * spread)
        out.b.copy_(torch.tensor([mu_bias, 0.0]))
        if ls_pin is not None:
            out.w[1].zero_()
            out.b[1] = ls_pin
    return arm


def smooth_latent(C, H, W, seed, amp=6.0, noise=1.0):
    """round(low-pass field + Laplace noise): neighbours are correlated, so the context matters.  (C, H, W) float32, integer-valued."""
    rng = np.random.default_rng(seed)
    hh, ww = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    field = np.zeros((C, H, W))
    for c in range(C):
        for _ in range(4):
            fh, fw, ph = rng.uniform(0.3, 2.5), rng.uniform(0.3, 2.5), rng.uniform(0, 2 * np.pi)
            field[c] += rng.normal() * np.sin(2 * np.pi * (fh * hh + fw * ww) + ph)
    return np.round(amp * field / 2 + rng.laplace(0.0, noise, (C, H, W))).astype(np.float32)


def params_cpu(y, arm):
    """(mu, s) of every latent of y (C, H, W) from ArmMLP.forward on the CPU, float32, flat in (c, h, w) order"""
    with torch.no_grad():
        raw = arm(arm_ref.contexts_torch(torch.as_tensor(y, dtype=torch.float32).reshape((1,) + tuple(y.shape[-3:]))))
    mu, ls = raw[:, 0], raw[:, 1]
    return mu.numpy(), torch.exp(-0.5 * torch.clamp(ls, min=arm_ref.LS_MIN, max=arm_ref.LS_MAX)).numpy()


def quantise(mu, s):
    mu, s = np.asarray(mu, dtype=np.float32), np.asarray(s, dtype=np.float32)
    return (np.rint(mu * np.float32(QUANT)) / np.float32(QUANT)).astype(np.float32), \
        np.maximum(np.rint(s * np.float32(QUANT)) / np.float32(QUANT), np.float32(1.0 / QUANT)).astype(np.float32)


def ac_max_val(y):
    return int(np.ceil(np.abs(np.asarray(y, dtype=np.float64)).max())) + 2


def cdf64(t, mu, s):
    d = np.asarray(t, dtype=np.float64) - mu
    return 0.5 - 0.5 * np.sign(d) * np.expm1(-np.abs(d) / s)


def rows_ref(mu_q, s_q, A):
    """(n, L + 1) int64 rows before the modulo: rint(F64 (65536 - L)) + j, entry 0 = 0, entry L = 65536"""
    L = 2 * A + 1
    mu, s = np.asarray(mu_q, dtype=np.float64).reshape(-1, 1), np.asarray(s_q, dtype=np.float64).reshape(-1, 1)
    j = np.arange(L + 1)
    e = cdf64(j - A - 0.5, mu, s)
    e[:, 0], e[:, L] = 0.0, 1.0
    return np.rint(e * (65536 - L)).astype(np.int64) + j


def ideal_bits(y, mu_q, s_q):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    p = cdf64(y + 0.5, mu_q, s_q) - cdf64(y - 0.5, mu_q, s_q)
    return float(-np.log2(np.maximum(p, 2.0 ** -16)).sum())


def size_bound_bits(ideal, n, A, n_chunks, header_bytes):
    """1 % for the integerisation, the one-count floor per symbol (-log2(1 - L / 65536) < 2 L / 65536), a 32-bit count and at most a
    40-bit flush per chunk (96 bits), the header"""
    L = 2 * A + 1
    return 1.01 * ideal + n * 2 * L / 65536 + 96 * n_chunks + 8 * header_bytes


def chunk_order(C, H, W, S):
    """flat (c, h, w) indices of every chunk's symbols, chunks in (channel, strip) order"""
    idx = np.arange(C * H * W).reshape(C, H, W)
    return [idx[c, :, k * S:min(W, (k + 1) * S)].reshape(-1) for c in range(C) for k in range(-(-W // S))]


def host_encode(sym, rows_u16):
    """torchac's bytes of int16 symbols under uint16 rows (n, lp): the library's host coder"""
    from gauspcc_amd import _lib

    sym = np.ascontiguousarray(sym, dtype=np.int16)
    rows = np.ascontiguousarray(rows_u16, dtype=np.uint16)
    n, lp = rows.shape
    cap = 4 * n + 64
    out = np.zeros(cap, dtype=np.uint8)
    nb = ctypes.c_int64(0)
    _lib.check(_lib.lib().gsac_host_encode_u16(sym.ctypes.data, rows.ctypes.data, n, lp, out.ctypes.data, cap, ctypes.byref(nb)))
    return out[:nb.value].tobytes()


def host_decode(data, rows_u16):
    from gauspcc_amd import _lib

    rows = np.ascontiguousarray(rows_u16, dtype=np.uint16)
    n, lp = rows.shape
    buf = np.frombuffer(data, dtype=np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    out = np.zeros(n, dtype=np.int16)
    _lib.check(_lib.lib().gsac_host_decode_u16(rows.ctypes.data, buf.ctypes.data, len(data), n, lp, out.ctypes.data))
    return out


def build_header(C, H, W, A, S, dims, counts):
    """"GSAL", u16 version, u16 16, u32 C, H, W, S, u16 A, u8 n widths, u8 0, the widths, u32 chunk count, u32 byte counts"""
    return (struct.pack("<4sHHIIIIHBB", MAGIC, VERSION, QUANT, C, H, W, S, A, len(dims), 0) + bytes(dims)
            + struct.pack("<I", len(counts)) + b"".join(struct.pack("<I", c) for c in counts))


def chunk_payloads(y, rows_u16, S):
    """every chunk's bytes of y (C, H, W) under rows (n, L + 1) uint16 (flat (c, h, w) order)"""
    C, H, W = y.shape
    A = (rows_u16.shape[1] - 2) // 2
    sym = (np.asarray(y).reshape(-1) + A).astype(np.int16)
    return [host_encode(sym[ix], rows_u16[ix]) for ix in chunk_order(C, H, W, S)]


def encode_ref(y, mu, s, S, dims):
    """the whole stream of y (C, H, W) under float32 (mu, s) (unquantised), rows from float64"""
    C, H, W = y.shape
    A = ac_max_val(y)
    mu_q, s_q = quantise(mu, s)
    rows = (rows_ref(mu_q, s_q, A) & 0xFFFF).astype(np.uint16)
    parts = chunk_payloads(y, rows, S)
    return build_header(C, H, W, A, S, dims, [len(p) for p in parts]) + b"".join(parts)
