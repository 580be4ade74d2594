"""CPU checks of the spherical-harmonic colour pass: the two restatements of tests/sh_ref.py and gauspcc_amd.sh_utils' torch path against
tests/golden/sh.npz (the reference's own utils/sh_utils.py, see tests/golden/make_sh_golden.py), and the ABI entries.

Bounds.  float64 against float64: the two programs differ only in how they associate a few products, so 1e-12 relative to the largest
value is three orders above what double rounding can give.  float32: the project's standing e <= 4 e_t32 + 1e-6 scale, e_t32 the error
of the reference's own float32 run stored in the fixture (values) or of the float32 torch program on the same inputs (gradients)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import sh_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEGREES = (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sh.npz"))
    d = {k: g[k] for k in g.files}
    d["sh"] = d["sh_q"].astype(np.float64) / 32          # (N, 3, M)
    return d


def _holds(e, e_t32, scale, what):
    assert e <= 4 * e_t32 + 1e-6 * scale, (what, e, e_t32, scale)


def _grads64(gold, deg):
    sh = torch.tensor(gold["sh"], requires_grad=True)
    dirs = torch.tensor(gold["dirs"], requires_grad=True)
    val = sr.eval64(deg, sh, dirs)
    (val * torch.tensor(gold["weights"], dtype=torch.float64)).sum().backward()
    return val.detach().numpy(), sh.grad.numpy(), (dirs.grad.numpy() if dirs.grad is not None else np.zeros_like(gold["dirs"]))


def test_fixture_shape(gold):
    assert gold["sh"].shape == (200, 3, 25) and gold["dirs"].shape == (200, 3)
    assert np.abs(np.linalg.norm(gold["dirs"], axis=1) - 1).max() < 1e-15
    assert float(np.abs(gold["sh"]).max()) <= 2.0 and gold["sh"].astype(np.float32).astype(np.float64).tolist() == gold["sh"].tolist()


@pytest.mark.parametrize("deg", DEGREES)
def test_float64_restatement_matches_reference(gold, deg):
    val, gsh, gdirs = _grads64(gold, deg)
    for got, want, what in ((val, gold[f"value64_{deg}"], "value"), (gsh[:16], gold[f"gsh64_{deg}"], "grad sh"), (gdirs, gold[f"gdirs64_{deg}"], "grad dirs")):
        scale = max(float(np.abs(want).max()), 1e-300)
        assert float(np.abs(got - want).max()) <= 1e-12 * scale, (deg, what)
    assert not gsh[:, :, sr.count(deg):].any()


@pytest.mark.parametrize("deg", DEGREES)
def test_float32_restatement_within_float32_torch_error(gold, deg):
    sh32 = np.ascontiguousarray(gold["sh"].transpose(0, 2, 1)).astype(np.float32)        # (N, M, 3)
    d32 = gold["dirs"].astype(np.float32)
    want = gold[f"value64_{deg}"]
    val, none = sr.forward32(sh32, deg, dirs=d32)
    assert none is None and val.dtype == np.float32
    e_t32 = float(np.abs(gold[f"value32_{deg}"].astype(np.float64) - want).max())
    _holds(float(np.abs(val.astype(np.float64) - want).max()), e_t32, float(np.abs(want).max()), ("value", deg))
    # the hand-written backward against autograd in float64; e_t32 from autograd of the float32 torch program
    gsh, gd = sr.backward32(sh32, deg, gold["weights"], dirs=d32)
    _, gsh64, gd64 = _grads64(gold, deg)
    sh_t = torch.tensor(gold["sh"], dtype=torch.float32, requires_grad=True)
    d_t = torch.tensor(d32, requires_grad=True)
    (sr.torch32_eval(deg, sh_t, d_t) * torch.tensor(gold["weights"])).sum().backward()
    t_gd = d_t.grad.numpy() if d_t.grad is not None else np.zeros_like(d32)
    _holds(float(np.abs(gsh.transpose(0, 2, 1) - gsh64).max()), float(np.abs(sh_t.grad.numpy() - gsh64).max()), float(np.abs(gsh64).max()), ("grad sh", deg))
    _holds(float(np.abs(gd - gd64).max()), float(np.abs(t_gd - gd64).max()), float(np.abs(gd64).max()), ("grad dirs", deg))
    assert not gsh[:, sr.count(deg):].any()


def test_float32_restatement_clamping_mode_matches_float64():
    """The means3D form: direction, +0.5, clamp, the camera-centre rule and the normalisation's backward, against float64 autograd."""
    rng = np.random.default_rng(3)
    P, deg, M = 400, 3, 16
    sh = rng.standard_normal((P, M, 3)).astype(np.float32)
    sh[:, 0] -= np.float32(0.5 / sr.C0)                      # value + 0.5 is then symmetric about 0
    means = rng.uniform(-2, 2, (P, 3)).astype(np.float32)
    cam = np.array([0.25, -0.5, 3.0], np.float32)
    means[5] = cam
    dcol = rng.standard_normal((P, 3)).astype(np.float32)
    col, clamped = sr.forward32(sh, deg, means=means, campos=cam)
    assert 0.4 < clamped.mean() < 0.6
    gsh, gm = sr.backward32(sh, deg, dcol, means=means, campos=cam, clamped=clamped)
    assert np.isfinite(col).all() and np.isfinite(gm).all() and not gm[5].any()
    assert np.array_equal(col[5], np.maximum(np.float32(sr.C0) * sh[5, 0] + np.float32(0.5), 0))

    def run(dtype, fn):
        s, m = torch.tensor(sh, dtype=dtype, requires_grad=True), torch.tensor(means, dtype=dtype, requires_grad=True)
        c = fn(s, m, torch.tensor(cam, dtype=dtype), deg)
        (c * torch.tensor(dcol, dtype=dtype)).sum().backward()
        return c.detach().numpy(), s.grad.numpy(), m.grad.numpy()

    c64, s64, m64 = run(torch.float64, sr.colors64)
    c32, s32, m32 = run(torch.float32, sr.torch32_colors)
    # a channel within float32 rounding of the clamp may fall on either side of it: those are compared nowhere
    pre = sr._torch_values(torch.tensor(sh).double(), deg, sr._torch_direction(torch.tensor(means).double(), torch.tensor(cam).double())).numpy() + 0.5
    safe = np.abs(pre) > 1e-5
    assert safe.mean() > 0.99 and np.array_equal(clamped[safe], pre[safe] < 0)
    rows = safe.all(axis=1)
    _holds(float(np.abs(col - c64)[safe].max()), float(np.abs(c32 - c64)[safe].max()), float(np.abs(c64).max()), "colours")
    _holds(float(np.abs(gsh - s64)[rows].max()), float(np.abs(s32 - s64)[rows].max()), float(np.abs(s64).max()), "grad sh")
    _holds(float(np.abs(gm - m64)[rows].max()), float(np.abs(m32 - m64)[rows].max()), float(np.abs(m64).max()), "grad means")


@pytest.mark.parametrize("deg", DEGREES)
def test_sh_utils_eval_sh_cpu(gold, deg):
    from gauspcc_amd import sh_utils

    want = gold[f"value64_{deg}"]
    sh, dirs = torch.tensor(gold["sh"], requires_grad=True), torch.tensor(gold["dirs"], requires_grad=True)
    val = sh_utils.eval_sh(deg, sh, dirs)
    assert val.dtype == torch.float64 and val.shape == (200, 3)
    assert float(np.abs(val.detach().numpy() - want).max()) <= 1e-12 * float(np.abs(want).max())
    (val * torch.tensor(gold["weights"], dtype=torch.float64)).sum().backward()
    assert float(np.abs(sh.grad.numpy()[:16] - gold[f"gsh64_{deg}"]).max()) <= 1e-12 * float(np.abs(gold[f"gsh64_{deg}"]).max())
    if deg:
        assert float(np.abs(dirs.grad.numpy() - gold[f"gdirs64_{deg}"]).max()) <= 1e-12 * float(np.abs(gold[f"gdirs64_{deg}"]).max())
    v32 = sh_utils.eval_sh(deg, sh.detach().float(), dirs.detach().float())
    assert v32.dtype == torch.float32
    _holds(float(np.abs(v32.double().numpy() - want).max()), float(np.abs(gold[f"value32_{deg}"].astype(np.float64) - want).max()),
           float(np.abs(want).max()), deg)


def test_sh_utils_eval_sh_shapes_and_errors(gold):
    from gauspcc_amd import sh_utils

    sh, dirs = torch.tensor(gold["sh"]), torch.tensor(gold["dirs"])
    # leading batch dimensions, another channel count, more coefficients stored than active
    a = sh_utils.eval_sh(2, sh.reshape(20, 10, 3, 25), dirs.reshape(20, 10, 3))
    assert a.shape == (20, 10, 3) and torch.equal(a.reshape(200, 3), sh_utils.eval_sh(2, sh, dirs))
    one = sh_utils.eval_sh(2, sh[:, :1], dirs)
    assert one.shape == (200, 1) and torch.equal(one[:, 0], sh_utils.eval_sh(2, sh, dirs)[:, 0])
    assert torch.equal(sh_utils.eval_sh(1, sh, dirs), sh_utils.eval_sh(1, sh[..., :4], dirs))
    assert sh_utils.sh_basis(3, dirs).shape == (200, 16)
    with pytest.raises(ValueError):
        sh_utils.eval_sh(5, sh, dirs)
    with pytest.raises(ValueError):
        sh_utils.eval_sh(3, sh[..., :15], dirs)
    with pytest.raises(RuntimeError):                       # the clamping form has no CPU path
        sh_utils.sh_colors(sh.transpose(1, 2).float(), dirs.float(), torch.zeros(3), 3)


def test_rgb_sh_round_trip(gold):
    from gauspcc_amd import sh_utils

    assert abs(sh_utils.C0 - float(gold["c0"])) <= 1e-16
    rgb = np.linspace(0, 1, 30).reshape(10, 3)
    for x in (rgb, rgb.astype(np.float32), torch.tensor(rgb), torch.tensor(rgb, dtype=torch.float32)):
        s = sh_utils.RGB2SH(x)
        back = sh_utils.SH2RGB(s)
        assert type(s) is type(x) and s.dtype == x.dtype and s.shape == x.shape
        tol = 1e-15 if "64" in str(x.dtype) else 1e-6
        assert float(abs(back - x).max()) <= tol
        assert float(abs(s - (x - 0.5) / float(gold["c0"])).max()) <= tol * 4
    assert sh_utils.SH2RGB(sh_utils.RGB2SH(0.25)) == pytest.approx(0.25, abs=1e-15)
    # a DC-only Gaussian shows the colour it was initialised from
    dc = sh_utils.RGB2SH(torch.tensor(rgb))[:, :, None]
    assert float((sh_utils.eval_sh(0, dc, torch.zeros(10, 3, dtype=torch.float64)) + 0.5 - torch.tensor(rgb)).abs().max()) <= 1e-15


def test_entry_points_declared_and_exported():
    from gauspcc_amd import _lib

    header = open(os.path.join(ROOT, "include", "gauspcc.h")).read()
    for name in ("gsr_sh_forward", "gsr_sh_backward"):
        assert re.search(r"GPCC_API\s+int\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name) and getattr(_lib.lib(), name).argtypes
    src = open(os.path.join(ROOT, "gauspcc_amd", "csrc", "sh.hip")).read()
    assert "fmaf" not in src and "__fma" not in src          # the contract: one IEEE operation per step
    assert "sh.hip" in open(os.path.join(ROOT, "gauspcc_amd", "csrc", "Makefile")).read()
