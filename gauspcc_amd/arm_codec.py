"""The bitstream of CAT-3DGS's tri-plane latents under its auto-regressive model, on the device (gsac_arm_encode / gsac_arm_decode): what
scene/gaussian_model.py's encode_triplane / decode_triplane do with the `constriction` range coder, a CPU copy of the planes and a Python
loop of W + 3 (H - 1) wavefront steps per plane and level,

    info, real_rate_byte = gaussians.encode_triplane(path)      ->   info, real_rate_byte = encode_triplane(grid, path)
    planes = gaussians.decode_triplane(path, info)               ->   planes = decode_triplane(grid, path)

`grid` is the tri-plane module: `.grids[level][plane]` ([1, C, H, W] each, planes xy, yz, zx) and the three `gauspcc_amd.arm.ArmMLP`s
`.arm`, `.arm2`, `.arm3`.  The files keep the reference's names (xy_bitstream_{j}.bin, ...).

THE BYTE FORMAT IS THIS LIBRARY'S OWN, not `constriction`'s: a file written here is read here.  What follows the reference is the
modelling -- context, ARM, get_mu_scale, the 1 / 16 quantisation of mu and scale, AC_MAX_VAL = ceil(max |y|) + 2, the wavefront
dependency, file names and return shapes.  DESIGN.md section 7 has the format.

One stream codes one latent grid y[C, H, W] of integer-valued float32 under one ArmMLP:

    encode_latents(y, arm, strip=None) -> bytes          decode_latents(data, arm) -> [1, C, H, W] float32 CUDA
    parse_header(data) -> dict                            (pure Python)

Header, little-endian: "GSAL", u16 version (1), u16 quantisation constant (16), u32 C, H, W, S, u16 A, u8 n (the ARM's widths, 12 and 2
included), u8 0, n x u8 widths, u32 chunk count, that many u32 byte counts; the chunks' payloads follow in (channel, strip) order.
Only the float mode (FPFM = 0); inputs must be float32 CUDA tensors (type and device checks as arm_rate).
"""
import ctypes
import os
import struct

import torch
import torch.nn as nn

from . import _lib, runtime
from .arm import _check_arm
from .runtime import ptrs

MAGIC, VERSION, QUANT = b"GSAL", 1, 16
MAX_AC_MAX_VAL, MIN_STRIP, MAX_STRIPS = 1024, 4, 1024
_FIXED = struct.Struct("<4sHHIIIIHBB")
PLANES = ("xy", "yz", "zx")


def default_strip(width):
    """The smallest multiple of 8 that cuts `width` columns into at most 64 strips: one wave per channel."""
    return 8 * max(1, -(-int(width) // 512))


def build_header(C, H, W, A, S, dims, counts):
    return (_FIXED.pack(MAGIC, VERSION, QUANT, C, H, W, S, A, len(dims), 0) + bytes(dims)
            + struct.pack(f"<I{len(counts)}I", len(counts), *counts))


def parse_header(data):
    """The header of one stream: C, H, W, A, S, quant, dims, counts, header_bytes and offsets (of every chunk's payload in `data`).
    ValueError on anything malformed; no GPU call."""
    data = bytes(data)
    if len(data) < _FIXED.size:
        raise ValueError("arm_codec: truncated header")
    magic, version, quant, C, H, W, S, A, nd, _ = _FIXED.unpack_from(data, 0)
    if magic != MAGIC:
        raise ValueError(f"arm_codec: bad magic {magic!r}")
    if version != VERSION:
        raise ValueError(f"arm_codec: version {version} (this library reads {VERSION})")
    if quant != QUANT:
        raise ValueError(f"arm_codec: quantisation constant {quant} ({QUANT} supported)")
    if min(C, H, W) < 1:
        raise ValueError(f"arm_codec: empty grid {C} x {H} x {W}")
    if S < MIN_STRIP:
        raise ValueError(f"arm_codec: strips of {S} columns (at least {MIN_STRIP})")
    if not 2 <= A <= MAX_AC_MAX_VAL:
        raise ValueError(f"arm_codec: AC_MAX_VAL {A} outside [2, {MAX_AC_MAX_VAL}]")
    pos = _FIXED.size
    if len(data) < pos + nd + 4:
        raise ValueError("arm_codec: truncated header")
    dims = list(data[pos:pos + nd])
    pos += nd
    (nch,) = struct.unpack_from("<I", data, pos)
    pos += 4
    K = -(-W // S)
    if K > MAX_STRIPS or C * H * W > 1 << 30:
        raise ValueError(f"arm_codec: grid {C} x {H} x {W} in strips of {S} is too large")
    if nch != C * K:
        raise ValueError(f"arm_codec: {nch} chunks, {C} channels x {K} strips expected")
    if len(data) < pos + 4 * nch:
        raise ValueError("arm_codec: truncated header")
    counts = list(struct.unpack_from(f"<{nch}I", data, pos))
    pos += 4 * nch
    if sum(counts) != len(data) - pos:
        raise ValueError(f"arm_codec: chunk sizes sum to {sum(counts)}, the payload has {len(data) - pos} bytes")
    offsets, run = [], pos
    for c in counts:
        offsets.append(run)
        run += c
    return {"C": C, "H": H, "W": W, "A": A, "S": S, "quant": quant, "dims": dims, "counts": counts, "header_bytes": pos, "offsets": offsets}


def _ints(vs):
    return (ctypes.c_int * max(len(vs), 1))(*vs)


def _arm_args(arm, who):
    dims, params = _check_arm(arm)
    for p in params:
        if p.dtype != torch.float32:
            raise TypeError(f"{who}: an ARM parameter must be float32, got {p.dtype}")
        if not p.is_cuda:
            raise RuntimeError(f"{who}: an ARM parameter must be a CUDA tensor (got {p.device}); gauspcc_amd has no CPU path")
        if p.device != params[0].device:
            raise ValueError(f"{who}: an ARM parameter on {p.device}, another on {params[0].device}")
    return dims, torch.cat([p.detach().reshape(-1) for p in params])


def _call(fn, *args):
    try:
        _lib.check(fn(*args))
    except _lib.GpccError as e:
        if e.code in (-2, -3, -5):    # GPCC_ERR_ARG / _RANGE / _FORMAT: the caller's data, not the device
            raise ValueError(str(e)) from None
        raise


def encode_levels(levels, arm, strips=None):
    """The levels of one plane under one ARM in one launch: a list of streams (bytes), one per level."""
    who = "encode_latents"
    dims, flat = _arm_args(arm, who)
    dev = flat.device
    ys, shapes = [], []
    for i, t in enumerate(levels):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: latent {i} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: latent {i} must be float32, got {t.dtype}")
        if not t.is_cuda:
            raise RuntimeError(f"{who}: latent {i} must be a CUDA tensor (got {t.device}); gauspcc_amd has no CPU path")
        if t.device != dev:
            raise ValueError(f"{who}: latent {i} on {t.device}, the ARM on {dev}")
        if t.dim() == 4 and t.shape[0] == 1:
            shape = tuple(t.shape[1:])
        elif t.dim() == 3:
            shape = tuple(t.shape)
        else:
            raise ValueError(f"{who}: latent {i} of shape {tuple(t.shape)}; [1, C, H, W] expected")
        if min(shape) < 1:
            raise ValueError(f"{who}: latent {i} of shape {tuple(t.shape)} is empty")
        shapes.append(shape)
        ys.append(t.detach().reshape(shape).contiguous())
    if not ys:
        raise ValueError(f"{who}: no latent")
    strips = [None] * len(ys) if strips is None else list(strips)
    S = [default_strip(s[2]) if v is None else int(v) for s, v in zip(shapes, strips)]
    for v, s in zip(S, shapes):
        if v < MIN_STRIP:
            raise ValueError(f"{who}: strips of {v} columns (at least {MIN_STRIP})")
        if -(-s[2] // v) > MAX_STRIPS:
            raise ValueError(f"{who}: {s[2]} columns in strips of {v} are more than {MAX_STRIPS} strips")
    n = len(ys)
    A = (ctypes.c_int * n)()
    data, nbytes, cnt, nch = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_void_p(), ctypes.c_int64()
    _call(_lib.lib().gsac_arm_encode, runtime.context(dev), n, ptrs(ys), _ints([s[0] for s in shapes]), _ints([s[1] for s in shapes]),
          _ints([s[2] for s in shapes]), _ints(S), flat.data_ptr(), len(dims) - 1, _ints(dims), A, ctypes.byref(data), ctypes.byref(nbytes),
          ctypes.byref(cnt), ctypes.byref(nch), runtime.stream_ptr(dev))
    counts = list((ctypes.c_int32 * nch.value).from_address(cnt.value)) if nch.value else []
    payload = ctypes.string_at(data.value, nbytes.value) if nbytes.value else b""
    out, c0, b0 = [], 0, 0
    for (C, H, W), s, a in zip(shapes, S, A):
        k = C * -(-W // s)
        mine = counts[c0:c0 + k]
        out.append(build_header(C, H, W, a, s, dims, mine) + payload[b0:b0 + sum(mine)])
        c0 += k
        b0 += sum(mine)
    return out


def decode_levels(datas, arm):
    """The inverse of encode_levels: a list of [1, C, H, W] float32 tensors on the ARM's device, all streams in one launch."""
    who = "decode_latents"
    dims, flat = _arm_args(arm, who)
    dev = flat.device
    heads = [parse_header(d) for d in datas]
    if not heads:
        raise ValueError(f"{who}: no stream")
    for h in heads:
        if h["dims"] != dims:
            raise ValueError(f"{who}: the stream was coded under an ARM of widths {h['dims']}, this one has {dims}")
    outs = [torch.empty((1, h["C"], h["H"], h["W"]), dtype=torch.float32, device=dev) for h in heads]
    payload = b"".join(bytes(d)[h["header_bytes"]:] for d, h in zip(datas, heads))
    counts = [c for h in heads for c in h["counts"]]
    buf = ctypes.create_string_buffer(payload, max(len(payload), 1))
    cnt = (ctypes.c_int32 * max(len(counts), 1))(*counts)
    _call(_lib.lib().gsac_arm_decode, runtime.context(dev), len(heads), ptrs(outs), _ints([h["C"] for h in heads]), _ints([h["H"] for h in heads]),
          _ints([h["W"] for h in heads]), _ints([h["S"] for h in heads]), _ints([h["A"] for h in heads]), flat.data_ptr(), len(dims) - 1,
          _ints(dims), ctypes.cast(buf, ctypes.c_void_p), len(payload), ctypes.cast(cnt, ctypes.c_void_p), len(counts), runtime.stream_ptr(dev))
    return outs


def encode_latents(y, arm, strip=None):
    """One grid y ([1, C, H, W] or [C, H, W], integer-valued float32, CUDA) under `arm` -> one stream.  strip: columns per strip
    (>= 4; default: default_strip(W)).  ValueError for a latent that is not an integer or beyond +-1022 (AC_MAX_VAL <= 1024), or an ARM
    whose mu / scale is not finite somewhere."""
    return encode_levels([y], arm, [strip])[0]


def decode_latents(data, arm):
    """The grid of one stream: [1, C, H, W] float32 on the ARM's device.  ValueError for a malformed header or another ARM's widths."""
    return decode_levels([data], arm)[0]


def _arms(grid):
    return (grid.arm, grid.arm2, grid.arm3)


def encode_triplane(grid, pre_path_name):
    """Writes {xy,yz,zx}_bitstream_{level}.bin under pre_path_name: round(latent * 16) of every plane and level, one launch per plane.
    Returns ([AC_MAX_VAL list of xy, of yz, of zx], the files' summed size in bytes)."""
    info, real_rate_byte = [], 0
    for p, (name, arm) in enumerate(zip(PLANES, _arms(grid))):
        levels = [torch.round(g[p].detach() * QUANT) for g in grid.grids]
        streams = encode_levels(levels, arm)
        info.append([parse_header(s)["A"] for s in streams])
        for j, s in enumerate(streams):
            path = os.path.join(pre_path_name, f"{name}_bitstream_{j}.bin")
            with open(path, "wb") as f:
                f.write(s)
            real_rate_byte += os.path.getsize(path)
    return info, real_rate_byte


def decode_triplane(grid, pre_path_name, info=None):
    """One nn.ParameterList of the three [1, C, H, W] planes per level of grid.grids: the decoded latents / 16, on the ARMs' device.
    The files describe themselves; `info` is accepted for the reference's signature and not needed."""
    n = len(grid.grids)
    planes = []
    for name, arm in zip(PLANES, _arms(grid)):
        datas = []
        for j in range(n):
            with open(os.path.join(pre_path_name, f"{name}_bitstream_{j}.bin"), "rb") as f:
                datas.append(f.read())
        planes.append(decode_levels(datas, arm))
    return [nn.ParameterList([nn.Parameter(planes[p][j] / QUANT, requires_grad=False) for p in range(3)]) for j in range(n)]
