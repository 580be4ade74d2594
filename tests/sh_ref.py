"""Restatements of the spherical-harmonic colour contract of include/gauspcc.h (gsr_sh_forward / gsr_sh_backward), independent of the
library and of gauspcc_amd.sh_utils:

  forward32 / backward32   numpy float32, operation for operation what csrc/sh.hip computes: the same bits
  colors64 / eval64        float64 torch with autograd: the values and gradients the float32 results are measured against
  torch32_colors / torch32_eval   the float32 torch program a framework runs without the kernel (pipe.convert_SHs_python): the error
                           of this program on the same inputs is the e_t32 of the project's bound e_dev <= 4 e_t32 + 1e-6 scale

Coefficients are (P, M, 3) here ("rasteriser layout"); eval64 / torch32_eval take eval_sh's (..., 3, M).  One table of constants and one
table of polynomials serve both number types: `terms` only multiplies, adds and subtracts, in the contract's order.
"""
from math import pi, sqrt

import numpy as np
import torch

C0 = 0.5 * sqrt(1 / pi)
C1 = sqrt(3 / (4 * pi))
C2A, C2C, C2E = 0.5 * sqrt(15 / pi), 0.25 * sqrt(5 / pi), 0.25 * sqrt(15 / pi)
C3A, C3B, C3C, C3D, C3F = 0.25 * sqrt(35 / (2 * pi)), 0.5 * sqrt(105 / pi), 0.25 * sqrt(21 / (2 * pi)), 0.25 * sqrt(7 / pi), 0.25 * sqrt(105 / pi)
C4A, C4B, C4C, C4D = 0.75 * sqrt(35 / pi), 0.75 * sqrt(35 / (2 * pi)), 0.75 * sqrt(5 / pi), 0.75 * sqrt(5 / (2 * pi))
C4E, C4G, C4I = (3 / 16) * sqrt(1 / pi), (3 / 8) * sqrt(5 / pi), (3 / 16) * sqrt(35 / pi)


def count(degree):
    return (degree + 1) ** 2


def terms(degree, x, y, z, n):
    """(basis, grads): basis[k] = b_k(d) and grads[k] = (db_k/dx, db_k/dy, db_k/dz) with None for an identically zero derivative; n(v)
    makes a constant of the arrays' number type.  Written in the order of the header: every product and difference is one operation."""
    one = torch.ones_like(x) if isinstance(x, torch.Tensor) else np.ones_like(x)
    b = [n(C0) * one]
    g = [(None, None, None)]
    if degree >= 1:
        b += [n(-C1) * y, n(C1) * z, n(-C1) * x]
        g += [(None, n(-C1) * one, None), (None, None, n(C1) * one), (n(-C1) * one, None, None)]
    if degree >= 2:
        xx, yy, zz = x * x, y * y, z * z
        xy, yz, xz = x * y, y * z, x * z
        xmy = xx - yy
        b += [n(C2A) * xy, n(-C2A) * yz, n(C2C) * ((n(2.0) * zz - xx) - yy), n(-C2A) * xz, n(C2E) * xmy]
        g += [(n(C2A) * y, n(C2A) * x, None),
              (None, n(-C2A) * z, n(-C2A) * y),
              ((n(-2.0) * n(C2C)) * x, (n(-2.0) * n(C2C)) * y, (n(4.0) * n(C2C)) * z),
              (n(-C2A) * z, None, n(-C2A) * x),
              ((n(2.0) * n(C2E)) * x, (n(-2.0) * n(C2E)) * y, None)]
    if degree >= 3:
        p = n(3.0) * xx - yy
        q = (n(4.0) * zz - xx) - yy
        r = (n(2.0) * zz - n(3.0) * xx) - n(3.0) * yy
        s = xx - n(3.0) * yy
        xyz = xy * z
        b += [n(-C3A) * (y * p), n(C3B) * xyz, n(-C3C) * (y * q), n(C3D) * (z * r), n(-C3C) * (x * q), n(C3F) * (z * xmy), n(-C3A) * (x * s)]
        g += [(n(-C3A) * (n(6.0) * xy), n(-C3A) * (n(3.0) * xmy), None),
              (n(C3B) * yz, n(C3B) * xz, n(C3B) * xy),
              (n(-C3C) * (n(-2.0) * xy), n(-C3C) * (q - n(2.0) * yy), n(-C3C) * (n(8.0) * yz)),
              (n(C3D) * (n(-6.0) * xz), n(C3D) * (n(-6.0) * yz), n(C3D) * (r + n(4.0) * zz)),
              (n(-C3C) * (q - n(2.0) * xx), n(-C3C) * (n(-2.0) * xy), n(-C3C) * (n(8.0) * xz)),
              (n(C3F) * (n(2.0) * xz), n(C3F) * (n(-2.0) * yz), n(C3F) * xmy),
              (n(-C3A) * (n(3.0) * xmy), n(-C3A) * (n(-6.0) * xy), None)]
    if degree >= 4:
        zz7 = n(7.0) * zz
        u = zz7 - n(1.0)
        v = zz7 - n(3.0)
        t19 = n(21.0) * zz - n(3.0)
        b += [n(C4A) * (xy * xmy), n(-C4B) * (yz * p), n(C4C) * (xy * u), n(-C4D) * (yz * v), n(C4E) * (zz * (n(35.0) * zz - n(30.0)) + n(3.0)),
              n(-C4D) * (xz * v), n(C4G) * (xmy * u), n(-C4B) * (xz * s), n(C4I) * (xx * s - yy * p)]
        g += [(n(C4A) * (y * p), n(C4A) * (x * s), None),
              (n(-C4B) * (n(6.0) * xyz), n(-C4B) * (z * (n(3.0) * xmy)), n(-C4B) * (y * p)),
              (n(C4C) * (y * u), n(C4C) * (x * u), n(C4C) * (n(14.0) * xyz)),
              (None, n(-C4D) * (z * v), n(-C4D) * (y * t19)),
              (None, None, n(C4E) * (z * (n(140.0) * zz - n(60.0)))),
              (n(-C4D) * (z * v), None, n(-C4D) * (x * t19)),
              (n(C4G) * (n(2.0) * (x * u)), n(C4G) * (n(-2.0) * (y * u)), n(C4G) * (n(14.0) * (z * xmy))),
              (n(-C4B) * (z * (n(3.0) * xmy)), n(-C4B) * (n(-6.0) * xyz), n(-C4B) * (x * s)),
              (n(C4I) * (n(4.0) * (x * s)), n(C4I) * (n(-4.0) * (y * p)), None)]
    return b, g


# ---------------------------------------------------------------------------------------------------------------- numpy float32
F = np.float32


def _direction32(means, campos):
    v = means.astype(F) - campos.astype(F)[None, :]
    l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    length = np.sqrt(l2)
    centre = l2 == F(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(centre[:, None], F(0.0), v / length[:, None]).astype(F)
    return d, length, centre


def forward32(sh, degree, means=None, campos=None, dirs=None):
    """sh (P, M, 3) float32.  means + campos: (colours, clamped bool (P, 3)); dirs: (values, None)."""
    sh = np.asarray(sh, F)
    d = _direction32(np.asarray(means), np.asarray(campos))[0] if dirs is None else np.asarray(dirs, F)
    b, _ = terms(degree, d[:, 0], d[:, 1], d[:, 2], F)
    val = b[0][:, None] * sh[:, 0, :]
    for k in range(1, count(degree)):
        val = val + b[k][:, None] * sh[:, k, :]
    assert val.dtype == F
    if dirs is not None:
        return val, None
    v = val + F(0.5)
    clamped = v < F(0.0)
    return np.where(clamped, F(0.0), v).astype(F), clamped


def backward32(sh, degree, dcolors, means=None, campos=None, dirs=None, clamped=None):
    """(dL_dsh (P, M, 3), dL_dmeans or dL_ddirs (P, 3)), float32, as gsr_sh_backward writes them."""
    sh, dcolors = np.asarray(sh, F), np.asarray(dcolors, F)
    P, M, _ = sh.shape
    if dirs is None:
        d, length, centre = _direction32(np.asarray(means), np.asarray(campos))
        g = np.where(clamped, F(0.0), dcolors).astype(F)
    else:
        d, g, clamped = np.asarray(dirs, F), dcolors, np.zeros((P, 3), bool)
    b, gb = terms(degree, d[:, 0], d[:, 1], d[:, 2], F)
    K = count(degree)
    gsh = np.zeros((P, M, 3), F)
    for k in range(K):
        gsh[:, k, :] = np.where(clamped, F(0.0), b[k][:, None] * g)
    if degree == 0:                                          # no term: exactly +0
        return gsh, np.zeros((P, 3), F)
    acc = [None, None, None]                                 # each sum starts with its first term
    for k in range(1, K):
        t = (sh[:, k, 0] * g[:, 0] + sh[:, k, 1] * g[:, 1]) + sh[:, k, 2] * g[:, 2]
        for a in range(3):
            if gb[k][a] is not None:
                acc[a] = gb[k][a] * t if acc[a] is None else acc[a] + gb[k][a] * t
    gd = np.stack(acc, 1)
    assert gd.dtype == F and gsh.dtype == F
    if dirs is not None:
        return gsh, gd
    dot = (gd[:, 0] * d[:, 0] + gd[:, 1] * d[:, 1]) + gd[:, 2] * d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        gm = np.where(centre[:, None], F(0.0), (gd - d * dot[:, None]) / length[:, None]).astype(F)
    return gsh, gm


# ---------------------------------------------------------------------------------------------------------------- torch
def _torch_values(sh, degree, d):
    """sum_k b_k(d) sh[:, k, :] for sh (P, M, 3) and d (P, 3), in the tensors' own dtype."""
    b, _ = terms(degree, d[:, 0], d[:, 1], d[:, 2], lambda v: v)
    val = b[0][:, None] * sh[:, 0, :]
    for k in range(1, count(degree)):
        val = val + b[k][:, None] * sh[:, k, :]
    return val


def _torch_direction(means, campos):
    v = means - campos[None, :]
    length = v.norm(dim=1, keepdim=True)
    return torch.where(length > 0, v / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(v))


def colors64(sh, means, campos, degree):
    """float64, differentiable in sh and means: max(values + 0.5, 0)."""
    return torch.clamp_min(_torch_values(sh.double(), degree, _torch_direction(means.double(), campos.double())) + 0.5, 0.0)


def eval64(degree, sh, dirs):
    """float64 eval_sh: sh (P, 3, M), dirs (P, 3)."""
    return _torch_values(sh.double().transpose(1, 2), degree, dirs.double())


def torch32_colors(sh, means, campos, degree):
    return torch.clamp_min(_torch_values(sh.float(), degree, _torch_direction(means.float(), campos.float())) + 0.5, 0.0)


def torch32_eval(degree, sh, dirs):
    return _torch_values(sh.float().transpose(1, 2), degree, dirs.float())
