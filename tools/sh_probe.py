"""Times the spherical-harmonic colour pass (gsr_sh_forward / gsr_sh_backward behind gauspcc_amd.sh_utils.sh_colors) against the float32
torch program a framework runs with pipe.convert_SHs_python -- normalise (xyz - campos), eval_sh as a torch expression, clamp_min(. + 0.5,
0) -- in the same process, alternating, with device events, warm.  Writes the report profiles/r07_sh.txt holds.

    python tools/sh_probe.py [--iters 30] [--rounds 3] [--out profiles/r07_sh.txt]

Sections: 1. a call through Python (what training pays: allocations, autograd, launches); 2. the two entry points alone, back to back on
preallocated buffers, against the byte bound of the shapes; 3. one frame of tests/test_gpu_rd_loop.py's 200 k scene rendered with shs=
against the same frame with colors_precomp=."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gauspcc_amd import _lib, runtime, sh_utils  # noqa: E402

HBM = 6.3e12   # bytes / s: the achievable rate the project's byte bounds use
CASES = [(100_000, 3, 16), (100_000, 1, 16), (1_000_000, 3, 16), (1_000_000, 1, 16)]


def torch_colors(shs, means, campos, deg):
    d = means - campos
    d = d / d.norm(dim=1, keepdim=True)
    return torch.clamp_min(sh_utils._eval_sh_torch(deg, shs.transpose(1, 2), d) + 0.5, 0.0)


def _inputs(P, M, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shs = torch.randn(P, M, 3, device="cuda", generator=g) * 0.5
    shs[:, 0] += 0.5
    means = torch.rand(P, 3, device="cuda", generator=g) * 4 - 2
    campos = torch.tensor([0.25, -0.5, 6.0], device="cuda")
    w = torch.randn(P, 3, device="cuda", generator=g)
    return shs, means, campos, w


def _round(fn, shs, means, w, iters):
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for e in ev:
        s, m = shs.detach().requires_grad_(True), means.detach().requires_grad_(True)
        e[0].record()
        c = fn(s, m)
        e[1].record()
        c.backward(w)
        e[2].record()
    torch.cuda.synchronize()
    fwd = sum(e[0].elapsed_time(e[1]) for e in ev) / iters
    return {"fwd": fwd, "fwd+bwd": fwd + sum(e[1].elapsed_time(e[2]) for e in ev) / iters}


def _stats(rounds):
    return {p: (statistics.median(r[p] for r in rounds), min(r[p] for r in rounds), max(r[p] for r in rounds)) for p in rounds[0]}


def _calls(P, deg, M, iters, rounds):
    shs, means, campos, w = _inputs(P, M)
    paths = {"hip": lambda s, m: sh_utils.sh_colors(s, m, campos, deg), "torch": lambda s, m: torch_colors(s, m, campos, deg)}
    for fn in paths.values():
        _round(fn, shs, means, w, 3)
    runs = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            runs[k].append(_round(fn, shs, means, w, iters))
    return {k: _stats(v) for k, v in runs.items()}


def _raw(P, deg, M, iters, rounds, calibrate=False):
    """gsr_sh_forward and gsr_sh_backward alone: `iters` calls back to back between two events, preallocated outputs."""
    shs, means, campos, w = _inputs(P, M)
    col, cl = torch.empty(P, 3, device="cuda"), torch.empty(P, 3, dtype=torch.uint8, device="cuda")
    gsh, gm = torch.empty_like(shs), torch.empty_like(means)
    L, ctx, st = _lib.lib(), runtime.context(shs.device), runtime.stream_ptr(shs.device)
    strides = (shs.stride(1), shs.stride(2), shs.stride(0))

    def fwd():
        _lib.check(L.gsr_sh_forward(ctx, P, deg, shs.data_ptr(), *strides, means.data_ptr(), campos.data_ptr(), None, col.data_ptr(), cl.data_ptr(), st))

    def bwd():
        _lib.check(L.gsr_sh_backward(ctx, P, deg, M, shs.data_ptr(), *strides, means.data_ptr(), campos.data_ptr(), None, cl.data_ptr(), w.data_ptr(),
                                     gsh.data_ptr(), *strides, gm.data_ptr(), None, st))

    out = {}
    for name, fn in (("gsr_sh_forward", fwd), ("gsr_sh_backward", bwd)):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / iters * 1e3)          # us per call
        out[name] = (statistics.median(ts), min(ts), max(ts))
    if calibrate:
        # what this GPU does with the same buffers in torch's own kernels: a pure store and a copy of the 12 M bytes per Gaussian
        for name, fn in (("torch zero_ of dL_dsh", gsh.zero_), ("torch copy_ shs -> dL_dsh", lambda: gsh.copy_(shs))):
            for _ in range(5):
                fn()
            ts = []
            for _ in range(rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) / iters * 1e3)
            out[name] = (statistics.median(ts), min(ts), max(ts))
    K = (deg + 1) ** 2
    bytes_ = {"torch zero_ of dL_dsh": P * 12 * M, "torch copy_ shs -> dL_dsh": P * 24 * M,
              "gsr_sh_forward": P * (12 * K + 12 + 12 + 3), "gsr_sh_backward": P * (12 * K + 12 + 3 + 12 + 12 * M + 12)}
    return out, bytes_


def _frame(rounds, frames=10):
    """tests/test_gpu_rd_loop.py's 200 k-anchor scene and camera at 1600 x 1060: its neural Gaussians rendered with colors_precomp= and with
    shs= (degree 3; the DC coefficient is RGB2SH of the Gaussian's colour, the rest small noise), no_grad."""
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians
    from gauspcc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from gauspcc_amd.synth import SyntheticGaussianModel
    from tests.test_gpu_rd_loop import _camera

    dev = torch.device("cuda", 0)
    W, H = 1600, 1060
    pc = SyntheticGaussianModel(200_000, seed=3)
    cam, view, full, tx, ty = _camera(torch, pc, W, H, dev)
    rast = GaussianRasterizer(GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=tx, tanfovy=ty, bg=torch.tensor([0.05, 0.1, 0.15], device=dev),
                                                            scale_modifier=1.0, viewmatrix=view, projmatrix=full, sh_degree=3, campos=cam.camera_center,
                                                            prefiltered=False, debug=False))
    with torch.no_grad():
        xyz, color, opacity, scaling, rot, _ = generate_neural_gaussians(cam, pc, None)
        P = xyz.shape[0]
        shs = torch.randn(P, 16, 3, device=dev, generator=torch.Generator(device="cuda").manual_seed(1)) * 0.05
        shs[:, 0] = sh_utils.RGB2SH(color)
        geom = dict(means3D=xyz, means2D=None, opacities=opacity, scales=scaling, rotations=rot, cov3D_precomp=None)
        paths = {"colors_precomp=": lambda: rast(shs=None, colors_precomp=color, **geom), "shs=": lambda: rast(shs=shs, colors_precomp=None, **geom)}
        for fn in paths.values():
            fn()
        runs = {k: [] for k in paths}
        for _ in range(rounds):
            for k, fn in paths.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(frames):
                    fn()
                b.record()
                torch.cuda.synchronize()
                runs[k].append(a.elapsed_time(b) / frames)
    return P, {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["Spherical-harmonic colours on gfx950: gsr_sh_forward / gsr_sh_backward (csrc/sh.hip) behind gauspcc_amd.sh_utils.sh_colors, against the",
             "float32 torch program of pipe.convert_SHs_python on the same GPU: d = (xyz - campos) / |xyz - campos|, eval_sh as a torch expression",
             "(gauspcc_amd.sh_utils' fallback), clamp_min(. + 0.5, 0); autograd for its backward.  shs (P, 16, 3) float32 contiguous.",
             "Times are measured; byte bounds are computed from the shapes at the %.1f TB/s the project uses as the achievable HBM rate." % (HBM / 1e12),
             "",
             "1. A call through Python (tools/sh_probe.py: device events, warm, one process, hip and torch alternating, %d rounds x %d calls, median" % (args.rounds, args.iters),
             "   [min, max] of the round means, ms per call).  fwd = the forward with the graph built, fwd+bwd = forward + backward for shs and means3D.",
             ""]
    for P, deg, M in CASES:
        res = _calls(P, deg, M, args.iters, args.rounds)
        lines.append("   P = %d, degree %d of M = %d" % (P, deg, M))
        for k, phases in res.items():
            lines.append("      %-6s " % k + "  ".join("%s %.3f [%.3f, %.3f]" % (p, *v) for p, v in phases.items()))
        for p in res["hip"]:
            lines.append("      torch / hip, %-7s %.1fx" % (p, res["torch"][p][0] / res["hip"][p][0]))
    lines += ["",
              "2. The entry points alone: %d calls back to back on preallocated buffers between two device events, %d rounds, us per call, median" % (args.iters, args.rounds),
              "   [min, max] (measured).  Bound (computed): forward reads 12 K + 12 B and writes 15 B per Gaussian, backward reads 12 K + 27 B and",
              "   writes 12 M + 12 B, K = (degree + 1)^2 active coefficients; reached = bytes / time.  The bound counts active coefficients only: with",
              "   degree 1 of M = 16 the 48 active bytes of each 192-byte row still cost whole sectors.  shs at P = 1 M is 192 MB and fits the",
              "   256 MiB Infinity Cache together with little else, so warm repeats may be served partly from it; at P = 100 k a call is shorter",
              "   than the host's launch path, so its time is the launch rate, not the memory path.  At P = 1 M, degree 3, torch's own zero_ and copy_",
              "   on the dL_dsh buffer are timed the same way: what this GPU reaches on a pure store and on a copy of the same bytes.",
              ""]
    for P, deg, M in CASES:
        out, bytes_ = _raw(P, deg, M, args.iters, args.rounds, calibrate=(P, deg) == (1_000_000, 3))
        lines.append("   P = %d, degree %d of M = %d" % (P, deg, M))
        for name, (med, lo, hi) in out.items():
            bound = bytes_[name] / HBM * 1e6
            lines.append("      %-25s %8.1f [%.1f, %.1f] us   bound %6.1f us (%.1f MB)   reached %.2f TB/s = %.0f %% of the bound's rate" % (
                name, med, lo, hi, bound, bytes_[name] / 1e6, bytes_[name] / med / 1e6, 100 * bound / med))
    P, fr = _frame(args.rounds)
    lines += ["",
              "3. One frame of tests/test_gpu_rd_loop.py's 200 k-anchor scene (%d Gaussians, 1600 x 1060, degree 3 of M = 16), torch.no_grad(), 10 frames" % P,
              "   between two device events, %d rounds alternating, ms per frame, median [min, max] (measured):" % args.rounds]
    for k, v in fr.items():
        lines.append("      %-16s %.3f [%.3f, %.3f]" % (k, *v))
    lines.append("      shs= costs %.3f ms more per frame (gsr_sh_forward over all %d Gaussians and its two output allocations)" % (
        fr["shs="][0] - fr["colors_precomp="][0], P))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
