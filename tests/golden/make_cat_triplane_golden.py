"""Generate tests/golden/cat_triplane.npz by IMPORTING CAT-3DGS's scene/triplane.py from a checkout of the reference project (it is not
part of this repository; it needs einops and typing_extensions):

    python tests/golden/make_cat_triplane_golden.py <reference checkout>

Only inputs, parameter values, state-dict key names and shapes and the reference's float32 CPU outputs are stored -- no reference source
text.  scene/triplane.py imports `scene.synthesis` and `scene.arm`; the stub `scene` package of make_arm_golden.py lets those load without
the rest of the framework.  The constructor calls `.cuda()` on an index tensor: `torch.Tensor.cuda` is replaced by a no-op for this
process and everything runs on the CPU.  TriPlaneField.forward builds a tensor with device='cuda', so the generator runs forward's three
lines before get_density itself (pts - pca_mean, matmul with the rotation, / variance) and calls the module's own contract_to_unisphere
and get_density.

Inputs come from tests/cat_triplane_ref.py (case "odd": 65 points, C = 3, resolution [5, 7, 3], multipliers [1, 2]); the three ARMs get
randn * 0.06 parameters with last biases (0.3, -2.0) from generator seed 11.  Stored per path (`con`: contract=True, `pln`: contract=False):

  <path>_pts, <path>_<transform parameter>, plane_<l>_<p> (shared), arm_<j> (the 30 ARM parameters in state-dict order), w (upstream weights)
  <path>_q_feat, <path>_q_bits    get_density(itr=-1): features of the planes rounded to 1 / 16, total_bits
  <path>_q_gp<l><p>               autograd plane gradients of sum(features * w), itr=-1
  <path>_r_feat, <path>_r_zero    get_density(itr=3) with comp_iter=10: raw planes, and the second return value (the integer 0)
  <path>_r_gp<l><p>, pln_r_gpts   its plane gradients and, on the normalize_aabb path, the gradient of the points (pln_q_gpts for itr=-1)
  con_unisphere                   contract_to_unisphere on con_x (mag below 1, exactly 1, above 1, far away)
  con_normalized                  con_normalize_aabb of con_unisphere
  keys, shapes_<i>                the state dict's key names and shapes
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cat_triplane_ref as R  # noqa: E402

CASE = "odd"
CON_X = [[0.2, -0.3, 0.4], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.5, 0.5, 0.5], [1.0, 1.0, -1.0], [3.0, -0.1, 0.2], [-40.0, 25.0, 60.0], [0.0, 0.0, 1e-3]]


def import_triplane(ref):
    scene = types.ModuleType("scene")
    scene.__path__ = [os.path.join(ref, "src", "gs_compress", "CAT-3DGS", "scene")]
    sys.modules["scene"] = scene
    torch.Tensor.cuda = lambda self, *a, **k: self
    return importlib.import_module("scene.triplane")


def build(mod, contract, grids, xf, arms):
    _, _, C, res, mult, _, _ = next(c for c in R.CASES if c[0] == CASE)
    config = {"grid_dimensions": 2, "input_coordinate_dim": 3, "output_coordinate_dim": C, "resolution": list(res)}
    field = mod.TriPlaneField(1.0, config, list(mult), contract, 10)
    sd = field.state_dict()
    with torch.no_grad():
        for l, level in enumerate(grids):
            for p, plane in enumerate(level):
                sd[f"grids.{l}.{p}"].copy_(plane)
        arm_keys = [k for k in sd if k.startswith("arm")]
        for k, v in zip(arm_keys, arms):
            sd[k].copy_(v)
        sd["aabb"].copy_(xf["aabb"])
        if contract:
            sd["rotation_matrix"].copy_(xf["rotation"])
            sd["pca_mean"].copy_(xf["pca_mean"])
            sd["variance"].copy_(xf["variance"])
            sd["con_aabb"].copy_(xf["con_aabb"])
    field.load_state_dict(sd)
    return field, list(sd.keys()), [tuple(v.shape) for v in sd.values()], arm_keys


def run(field, pts, itr, w, contract):
    for p in field.parameters():
        p.grad = None
    pts = pts.clone().requires_grad_(not contract)
    x = pts
    if contract:
        x = x - field.pca_mean
        x = torch.matmul(x, field.rotation_matrix.detach())
        x = x / field.variance.detach()
        x = field.contract_to_unisphere(x.clone().detach(), torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]))
    feat, bits = field.get_density(x, itr=itr)
    (feat * w).sum().backward()
    gps = [[p.grad.clone() for p in level] for level in field.grids]
    return feat.detach(), bits, gps, (None if contract else pts.grad.clone())


def main(ref):
    mod = import_triplane(ref)
    out = {}
    g = torch.Generator().manual_seed(11)
    arms = None
    for path, contract in (("con", True), ("pln", False)):
        pts, grids, xf, _ = R.make_case(CASE, contract)
        if arms is None:
            probe, _, _, arm_keys = build(mod, contract, grids, xf, [])
            arms = [torch.randn(probe.state_dict()[k].shape, generator=g) * 0.06 for k in arm_keys]
            for j, k in enumerate(arm_keys):
                if k.endswith("mlp.8.b"):
                    arms[j] = torch.tensor([0.3, -2.0])
            w = torch.randn(pts.shape[0], probe.feat_dim, generator=g)
            for j, a in enumerate(arms):
                out[f"arm_{j}"] = a.numpy()
            out["w"] = w.numpy()
            for l, level in enumerate(grids):
                for p, plane in enumerate(level):
                    out[f"plane_{l}_{p}"] = plane.numpy()
        field, keys, shapes, _ = build(mod, contract, grids, xf, arms)
        out["keys"] = np.asarray(keys)
        for i, s in enumerate(shapes):
            out[f"shapes_{i}"] = np.asarray(s, dtype=np.int64)
        out[f"{path}_pts"] = pts.numpy()
        for k, v in xf.items():
            out[f"{path}_{k}"] = v.numpy()
        for tag, itr in (("q", -1), ("r", 3)):
            feat, bits, gps, gpts = run(field, pts, itr, w, contract)
            out[f"{path}_{tag}_feat"] = feat.numpy()
            if tag == "q":
                out[f"{path}_q_bits"] = bits.detach().numpy()
            else:
                assert isinstance(bits, int) and bits == 0
                out[f"{path}_r_zero"] = np.int64(bits)
            for l, level in enumerate(gps):
                for p, gp in enumerate(level):
                    out[f"{path}_{tag}_gp{l}{p}"] = gp.numpy()
            if gpts is not None:
                out[f"{path}_{tag}_gpts"] = gpts.numpy()
            print(f"{path} itr {itr}: features {tuple(feat.shape)}, bits {float(bits):.4f}, non-finite rows {int((~torch.isfinite(feat).all(1)).sum())}")
        if contract:
            x = torch.tensor(CON_X)
            y = field.contract_to_unisphere(x, torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]))
            out["con_x"], out["con_unisphere"] = x.numpy(), y.numpy()
            out["con_normalized"] = mod.con_normalize_aabb(y, field.aabb, field.con_aabb).detach().numpy()
            z = field.contract_to_unisphere(torch.zeros(1, 3), torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]))
            out["con_origin_is_nan"] = np.bool_(bool(torch.isnan(z).all()))
    path = os.path.join(HERE, "cat_triplane.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
