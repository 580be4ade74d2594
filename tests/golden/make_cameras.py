"""Generate tests/golden/cameras.npz by RUNNING the reference's own camera construction -- `getWorld2View2` and `getProjectionMatrix`
(src/gs_compress/HAC/utils/graphics_utils.py:38-71) -- from a checkout of the reference project (not part of this repository):

    python tests/golden/make_cameras.py <reference checkout>

Only inputs and what the reference's functions computed are stored -- no reference source text.

`Camera` (HAC/scene/cameras.py:17-57) moves every tensor to the GPU in its constructor and cannot be built on a CPU, so what its lines
54-57 do with the two functions' results is restated here (`camera_matrices`): the transpose of each, their product through `bmm`, and
`camera_center = world_view_transform.inverse()[3, :3]`.  `tanfovx` / `tanfovy` are math.tan(FoV * 0.5), as
HAC/gaussian_renderer/__init__.py:199-200 hands them to the rasteriser's settings.

Cameras (R: camera-to-world rotation, T: world-to-camera translation, as the reference's loaders pass them; C: the camera's centre):
  identity             the camera of tests/test_gpu_rasterizer.py::_scene at 200 x 120 (control: the same matrices)
  yaw90                a quarter turn about y: the rotation block is a signed permutation with a zero diagonal
  general              axis-angle (0.4, -0.7, 0.5), C = (1, -2, -6), FoVx 1.0, FoVy 0.75
  general_anisotropic  axis-angle (-0.5, 0.3, 0.9) (mostly roll), FoVx 0.9 < FoVy 1.05: tan(FoVx / 2) < tan(FoVy / 2), focal lengths
                       in pixels 1.9 : 1 at 200 x 120 and 2.1 : 1 at 83 x 45
  translated_scaled    axis-angle (0.2, 0.6, -0.3), getWorld2View2(R, T, translate=(0.5, -1.0, 0.25), scale=1.5): the two arguments of
                       the reference's scene normalisation

The run ends with a mutation self-check (tests/raster_ref.MUTANTS): for every camera but `identity`, on the scene the GPU gradient
tests use (raster_ref.scene_for_camera, 1200 Gaussians at 83 x 45), each wrong reading of the matrices must move the conics of the
index-free float64 projection by at least 100 x the 1e-4 norm-relative tolerance of those tests (`focal_y := focal_x` only where the
focal lengths differ).  A camera that does not bite is to be replaced.
"""
import importlib.util
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_wiring import save_npz      # noqa: E402

ZNEAR, ZFAR = 0.01, 100.0             # cameras.py:48-49
GRAD_TOL = 1e-4                       # tests/test_gpu_raster_backward.py: every gradient, norm-relative
CHECK = dict(n=1200, seed=3, W=83, H=45, cluster=300)


def rodrigues(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def _pose(R, C):
    """(R, T) of a camera with camera-to-world rotation R and centre C: Rt = [R^T | T], T = -R^T C."""
    R = np.asarray(R, np.float64)
    return R, -R.T @ np.asarray(C, np.float64)


def camera_inputs():
    out = {}
    R, T = _pose(np.eye(3), (0.0, 0.0, -6.0))
    out["identity"] = dict(R=R, T=T, FoVx=1.0, FoVy=2 * math.atan(math.tan(0.5) * 120 / 200))
    R, T = _pose(np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]), (-6.0, 0.5, 0.25))
    out["yaw90"] = dict(R=R, T=T, FoVx=1.0, FoVy=2 * math.atan(math.tan(0.5) * 120 / 200))
    R, T = _pose(rodrigues((0.4, -0.7, 0.5)), (1.0, -2.0, -6.0))
    out["general"] = dict(R=R, T=T, FoVx=1.0, FoVy=0.75)
    R = rodrigues((-0.5, 0.3, 0.9))
    R, T = _pose(R, -6.0 * R[:, 2] + np.array([0.3, -0.2, 0.1]))          # six units behind the origin along its own axis, a little off it
    out["general_anisotropic"] = dict(R=R, T=T, FoVx=0.9, FoVy=1.05)
    R, T = _pose(rodrigues((0.2, 0.6, -0.3)), (2.0, 1.0, -4.0))
    out["translated_scaled"] = dict(R=R, T=T, FoVx=1.0, FoVy=0.7, translate=np.array([0.5, -1.0, 0.25]), scale=1.5)
    return out


def camera_matrices(gu, c):
    """What Camera.__init__ forms (cameras.py:54-57), on the CPU."""
    w2v = gu.getWorld2View2(c["R"], c["T"], c["translate"], c["scale"]) if "translate" in c else gu.getWorld2View2(c["R"], c["T"])
    world_view_transform = torch.tensor(w2v).transpose(0, 1)
    projection_matrix = gu.getProjectionMatrix(znear=ZNEAR, zfar=ZFAR, fovX=c["FoVx"], fovY=c["FoVy"]).transpose(0, 1)
    full_proj_transform = (world_view_transform.unsqueeze(0).bmm(projection_matrix.unsqueeze(0))).squeeze(0)
    camera_center = world_view_transform.inverse()[3, :3]
    return world_view_transform, full_proj_transform, camera_center


def self_check(name, cam):
    from tests import raster_ref as rr

    sc = rr.scene_for_camera(cam, CHECK["n"], CHECK["seed"], CHECK["W"], CHECK["H"], cluster=CHECK["cluster"])
    t = rr.tensors(sc, "cpu")
    args = (t["means"], t["scales"], t["rots"], None, 1.0, t["view"], t["proj"], sc["tx"], sc["ty"], CHECK["W"], CHECK["H"])
    good = rr.project_matrix_form(*args)
    front = good[5] > 0.2
    con = torch.stack(good[2:5], 1)[front]
    fx, fy = CHECK["W"] / (2 * sc["tx"]), CHECK["H"] / (2 * sc["ty"])
    moves = {}
    for m in rr.MUTANTS:
        if m == "focal_y_is_focal_x" and abs(fx / fy - 1) < 0.2:
            continue
        bad = torch.stack(rr.mutant_projection(m)(*args)[2:5], 1)[front]
        bad = torch.nan_to_num(bad, nan=0.0, posinf=0.0, neginf=0.0)
        moves[m] = float((bad - con).norm() / con.norm())
        assert moves[m] >= 100 * GRAD_TOL, f"{name}: mutant {m} moves the conics by only {moves[m]:.2e}: replace the camera"
    print(f"  {name:<20} focal {fx:.2f} x {fy:.2f} at {CHECK['W']} x {CHECK['H']}; conics moved by " + ", ".join(f"{m} {v:.2f}" for m, v in moves.items()))
    return moves


def main(ref):
    torch.set_num_threads(1)
    spec = importlib.util.spec_from_file_location("ref_graphics_utils", os.path.join(ref, "src/gs_compress/HAC/utils/graphics_utils.py"))
    gu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gu)
    inputs = camera_inputs()
    out = {"names": np.array(list(inputs))}
    cams = {}
    for name, c in inputs.items():
        view, full, centre = camera_matrices(gu, c)
        assert view.dtype == full.dtype == centre.dtype == torch.float32
        cam = dict(R=c["R"], T=c["T"], FoVx=np.float64(c["FoVx"]), FoVy=np.float64(c["FoVy"]), znear=np.float64(ZNEAR), zfar=np.float64(ZFAR),
                   translate=np.asarray(c.get("translate", np.zeros(3)), np.float64), scale=np.float64(c.get("scale", 1.0)),
                   world_view_transform=view.numpy(), full_proj_transform=full.numpy(), camera_center=centre.numpy(),
                   tanfovx=np.float64(math.tan(c["FoVx"] * 0.5)), tanfovy=np.float64(math.tan(c["FoVy"] * 0.5)))
        cams[name] = cam
        out.update({f"{name}/{k}": v for k, v in cam.items()})
    print("mutation self-check:")
    for name, cam in cams.items():
        if name != "identity":
            for m, v in self_check(name, cam).items():
                out[f"{name}/mutation_{m}"] = np.float64(v)
    path = os.path.join(HERE, "cameras.npz")
    save_npz(path, out)
    print(f"cameras.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
