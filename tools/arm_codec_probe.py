"""Times gauspcc_amd.arm_codec (gsac_arm_encode / gsac_arm_decode) at CAT-3DGS's shape for --anchors anchors: three planes, each with its
own ARM and two levels of 72 channels, round(sqrt(anchors / 36)) and twice that many texels per side (1 M anchors: 167^2 and 334^2, about
10 M latents per plane), and writes profiles/r07_arm_codec.txt.

    python tools/arm_codec_probe.py [--anchors 1000000] [--rounds 3] [--out profiles/r07_arm_codec.txt]

Per strip width S: encode and decode time per plane (host wall clock around the synchronising calls: the upload of the bytes and the copy
back are part of them), the streams' size against arm_rate's bits on the same latents, and the strips per channel at both levels.  Then the
excess of tests/test_gpu_arm_codec.py's size case over its ideal code length.

The reference's decode loop cannot be timed here: it needs the `constriction` package, which is absent.  As a LOWER bound on it the probe
times a torch restatement of its per-step work WITHOUT the coder: for each of the W + 3 (H - 1) wavefront steps of one (plane, level) an
index gather of the step's contexts on the host, a host-to-device copy, one MLP launch and a device-to-host copy."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gauspcc_amd import arm_codec as AC  # noqa: E402
from gauspcc_amd.arm import arm_rate  # noqa: E402
from tests import arm_codec_ref as R  # noqa: E402
from tests import arm_ref  # noqa: E402

DEV = "cuda"
CHANNELS = 72


def _smooth(side, g):
    """round(low-pass field + Laplace noise) on the device: neighbours are correlated"""
    coarse = torch.randn(1, CHANNELS, max(side // 16, 2), max(side // 16, 2), device=DEV, generator=g) * 3.0
    field = F.interpolate(coarse, size=(side, side), mode="bilinear", align_corners=True)
    u = torch.rand(1, CHANNELS, side, side, device=DEV, generator=g) - 0.5
    return torch.round(field - torch.sign(u) * torch.log1p(-2 * u.abs().clamp(max=0.4999)))


def _planes(anchors):
    g = torch.Generator(device=DEV).manual_seed(0)
    side = round((anchors / 36) ** 0.5)
    return side, [[_smooth(s, g) for s in (side, 2 * side)] for _ in range(3)], [R.make_arm([16, 16, 16, 16], 30 + i, spread=0.15).to(DEV) for i in range(3)]


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _measure(planes, arms, S, rounds):
    enc, dec, size = [], [], 0
    for r in range(rounds + 1):                               # the first round warms
        te = td = 0.0
        size = 0
        for lv, arm in zip(planes, arms):
            t, datas = _wall(lambda: AC.encode_levels(lv, arm, [S, S] if S else None))
            te += t
            t, back = _wall(lambda: AC.decode_levels(datas, arm))
            td += t
            size += sum(len(d) for d in datas)
            assert all(torch.equal(b, y) for b, y in zip(back, lv)), "round trip failed"
        if r:
            enc.append(te / 3)
            dec.append(td / 3)
    return enc, dec, size


def _reference_steps(y, arm):
    """the reference's per-step work without the coder, one (plane, level): contexts gathered on the host for wavefront w + 3 h = t"""
    C, H, W = y.shape[-3:]
    pad = F.pad(y.reshape(C, H, W).cpu(), (2, 2, 2, 2))
    hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    wave = (ww + 3 * hh).reshape(-1)
    order = torch.argsort(wave, stable=True)
    bounds = torch.searchsorted(wave[order].contiguous(), torch.arange(W + 3 * (H - 1) + 1))
    offs = torch.tensor([(i // 5) * (W + 4) + i % 5 for i in range(12)])
    base = (hh * (W + 4) + ww).reshape(-1)
    flat = pad.reshape(C, -1)
    params = list(arm.parameters())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for t in range(W + 3 * (H - 1)):
            pos = base[order[bounds[t]:bounds[t + 1]]]
            ctx = flat[:, (pos[:, None] + offs[None, :]).reshape(-1)].reshape(-1, 12)
            arm_ref.mlp_torch(ctx.to(DEV), params).cpu()
    return (time.perf_counter() - t0) * 1e3, W + 3 * (H - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_arm_codec.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/arm_codec_probe.py measures on the GPU; none is visible")
    side, planes, arms = _planes(args.anchors)
    n = 3 * CHANNELS * 5 * side * side
    with torch.no_grad():
        bits = sum(float(arm_rate(lv, arm)) for lv, arm in zip(planes, arms))
    lines = [f"tools/arm_codec_probe.py --anchors {args.anchors} --rounds {args.rounds}  ({torch.cuda.get_device_name(0)})",
             f"3 planes x [{CHANNELS}, {side}, {side}] + [{CHANNELS}, {2 * side}, {2 * side}], ARM 12-16-16-16-16-2 per plane: {n} latents, "
             f"arm_rate {bits / 8:.0f} bytes ({bits / n:.3f} bits per latent)",
             "ms per plane (both levels in one launch each way), median over the rounds [min, max]; bytes of all six streams, headers included",
             "   S  strips    encode ms              decode ms                 bytes   bytes x 8 / arm_rate bits"]
    dflt = AC.default_strip(2 * side)
    for S in (4, 8, 16, 32, 64):
        enc, dec, size = _measure(planes, arms, S, args.rounds)
        lines.append(f"  {S:2d}  {-(-side // S):3d}+{-(-2 * side // S):3d}  {statistics.median(enc):8.2f} [{min(enc):.2f}, {max(enc):.2f}]  "
                     f"{statistics.median(dec):8.2f} [{min(dec):.2f}, {max(dec):.2f}]  {size:10d}   {8 * size / bits:.4f}"
                     + ("   <- default_strip" if S == dflt else ""))
    y = torch.as_tensor(R.smooth_latent(8, 64, 96, 100 + 8 + 7 * 64 + 13 * 96)).to(DEV).reshape(1, 8, 64, 96)
    arm = R.make_arm([16, 16, 16, 16], 5, spread=0.15).to(DEV)
    data = AC.encode_latents(y, arm)
    h = AC.parse_header(data)
    _, mu, s = arm_rate(y, arm, reduce="none", return_params=True)
    mu_q, s_q = R.quantise(mu[0].reshape(-1).cpu().numpy(), s[0].reshape(-1).cpu().numpy())
    ideal = R.ideal_bits(y.cpu().numpy(), mu_q, s_q)
    lines.append(f"size case of tests/test_gpu_arm_codec.py ([8, 64, 96], S = {h['S']}, A = {h['A']}): {8 * len(data)} bits, ideal {ideal:.0f}, "
                 f"bound {R.size_bound_bits(ideal, y.numel(), h['A'], len(h['counts']), h['header_bytes']):.0f}; payload over ideal "
                 f"{100 * (8 * sum(h['counts']) / ideal - 1):+.3f} %, whole stream {100 * (8 * len(data) / ideal - 1):+.3f} %")
    lines.append("the reference's decode_triplane needs `constriction` (absent here) and cannot be timed; a LOWER bound, its per-step work without the coder")
    lines.append("(host gather, host-to-device copy, one MLP launch, device-to-host copy per wavefront step), one plane, in torch:")
    total = 0.0
    for y in planes[0]:
        _reference_steps(y[..., :32, :32].contiguous(), arms[0])                      # warm
        ms, steps = _reference_steps(y, arms[0])
        total += ms
        lines.append(f"  [{CHANNELS}, {y.shape[-2]}, {y.shape[-1]}]: {steps} steps, {ms:.1f} ms ({1e3 * ms / steps:.0f} us per step)")
    lines.append(f"  per plane {total:.1f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
