"""Times gauspcc_amd.loss_utils.wavelet_loss (gsr_wavelet_l1_forward / gsr_wavelet_l1_backward) against the float32 torch conv2d program
of tests/wavelet_ref.py -- the stand-in for pytorch_wavelets, which cannot be installed and so cannot be timed -- and
tcgs_photometric_loss against that program plus the reference's SSIM formula (tests/ssim_ref.py: ssim_torch32), in the same process,
alternating, with device events, warm.  Writes the report profiles/r07_wavelet.txt holds.

    python tools/wavelet_probe.py [--iters 50] [--rounds 5] [--size 3x1060x1600] [--step 0] [--out profiles/r07_wavelet.txt]

Phases: fwd = the training forward (the graph is built), step = forward + backward, eval = the forward under torch.no_grad().  Times are
medians [min, max] over rounds of --iters calls each, and include the Python-side allocations and launches of every call."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gauspcc_amd import loss_utils  # noqa: E402
from tests import ssim_ref, wavelet_ref  # noqa: E402

HBM = 6.3e12   # bytes / s: the achievable rate the project's byte bounds use


def _phase_times(fn, x, y, iters):
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    evals = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for e in ev:
        a = x.detach().requires_grad_(True)
        e[0].record()
        s = fn(a, y)
        e[1].record()
        s.backward()
        e[2].record()
    evals[0].record()
    with torch.no_grad():
        for _ in range(iters):
            fn(x, y)
    evals[1].record()
    torch.cuda.synchronize()
    fwd = sum(e[0].elapsed_time(e[1]) for e in ev) / iters
    bwd = sum(e[1].elapsed_time(e[2]) for e in ev) / iters
    return {"fwd": fwd, "step": fwd + bwd, "eval": evals[0].elapsed_time(evals[1]) / iters}


def _measure(paths, x, y, iters, rounds):
    for fn in paths.values():   # warm: code objects, MIOpen's algorithm choice
        _phase_times(fn, x, y, 3)
    runs = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            runs[k].append(_phase_times(fn, x, y, iters))
    out = {}
    for k, rs in runs.items():
        out[k] = {p: (statistics.median(r[p] for r in rs), min(r[p] for r in rs), max(r[p] for r in rs)) for p in rs[0]}
    return out


def _rows(title, res, lines):
    lines.append(title)
    for k, phases in res.items():
        lines.append("   %-6s " % k + "  ".join("%s %.3f [%.3f, %.3f]" % (p, *v) for p, v in phases.items()))
    for p in res["hip"]:
        lines.append("   torch / hip, %-4s  %.1fx  (ranges: hip [%.3f, %.3f], torch [%.3f, %.3f])" % (
            p, res["torch"][p][0] / res["hip"][p][0], res["hip"][p][1], res["hip"][p][2], res["torch"][p][1], res["torch"][p][2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", default="3x1060x1600")
    ap.add_argument("--step", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shape = tuple(int(v) for v in args.size.split("x"))
    step = args.step
    x, y = wavelet_ref.make_images(shape, seed=1, device="cuda")
    pixels = x.numel()

    def torch_tcgs(a, b):
        return (0.8 * loss_utils.l1_loss(a, b) + 0.2 * (1.0 - ssim_ref.ssim_torch32(a, b))) + 0.02 * wavelet_ref.wavelet_loss(a, b, step)

    wav = _measure({"hip": lambda a, b: loss_utils.wavelet_loss(a, b, step), "torch": lambda a, b: wavelet_ref.wavelet_loss(a, b, step)},
                   x, y, args.iters, args.rounds)
    full = _measure({"hip": lambda a, b: loss_utils.tcgs_photometric_loss(a, b, 0.2, 0.02, step)[0], "torch": torch_tcgs}, x, y, args.iters, args.rounds)

    lines = ["Wavelet loss on gfx950: gsr_wavelet_l1_forward / gsr_wavelet_l1_backward (csrc/wavelet.hip) against the float32 torch conv2d program",
             "(tests/wavelet_ref.py: wavelet_loss = a two-level afb1d-style DWT of both images, two grouped stride-2 F.conv2d per level, and the",
             "band L1 means; autograd for the backward).  That program stands in for pytorch_wavelets, which is not installed and was not timed.",
             "One MI355X, %s, step %d, images from tests/wavelet_ref.make_images.  Times are measured; the byte bounds are computed." % (args.size, step),
             "",
             "Device events, warm, same process, HIP and torch alternating (tools/wavelet_probe.py, %d rounds x %d calls, median [min, max] of the" % (args.rounds, args.iters),
             "round means, ms per call).  fwd = the training forward, step = forward + backward, eval = the forward under torch.no_grad().",
             ""]
    _rows("1. wavelet_loss(img1, img2, step=%d)" % step, wav, lines)
    lines.append("")
    _rows("2. tcgs_photometric_loss(image, gt, 0.2, 0.02, step=%d) against 0.8 l1 + 0.2 (1 - ssim_torch32) + 0.02 wavelet_loss (torch)" % step, full, lines)
    lines += ["",
              "3. Bytes (computed from the shape, %d pixels, not measured) at the %.1f TB/s the project uses as the achievable HBM rate:" % (pixels, HBM / 1e12),
              "   forward  reads  8 B/pixel = %.1f MB  -> %.1f us" % (8 * pixels / 1e6, 8 * pixels / HBM * 1e6),
              "   backward reads  8 B/pixel = %.1f MB, writes 4 B/pixel = %.1f MB  -> %.1f us" % (8 * pixels / 1e6, 4 * pixels / 1e6, 12 * pixels / HBM * 1e6),
              "   Both images fit the 256 MiB Infinity Cache, so a warm call is not an HBM-rate measurement; the per-call times above are",
              "   dominated by host work and launch gaps, as for the SSIM drop-in (profiles/r07_ssim.txt)."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
