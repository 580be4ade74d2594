#!/usr/bin/env python3
"""Developer probe: the hash-grid encoder's training path on the anchors of the synthetic HAC model (calc_interp_feat's normalised
anchors into the 3-D encoder: 12 levels, log2 13) -- the inference forward (gsge_forward), the forward with the gradient path
(_GridEncode.apply) and the backward (gsge_backward: embedding and input gradients) timed apart with events on the stream, median
of `reps` after warm-up, for n_features 2 and 4.  Also the contributions per table row (median and maximum).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel table.
    python tools/grid_train_probe.py [anchors ...] [--reps R]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gauspcc_amd import _gridencoder  # noqa: E402
from gauspcc_amd.gridencoder import GridEncoder, _GridEncode, _tables, grid_encode  # noqa: E402
from gauspcc_amd.synth import SyntheticGaussianModel  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
if "--reps" in sys.argv:
    args.remove(str(reps))
sizes = [int(a) for a in args] or [100_000, 1_000_000]
RES3 = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


for n in sizes:
    m = SyntheticGaussianModel(n, seed=0, device="cuda:0")
    x = ((m.get_anchor - m.x_bound_min) / (m.x_bound_max - m.x_bound_min)).contiguous()
    N = x.shape[0]
    for F in (2, 4):
        enc = GridEncoder(num_dim=3, n_features=F, resolutions_list=RES3, log2_hashmap_size=13, ste_binary=True).cuda()
        enc.params.data.uniform_(-1, 1)
        L = enc.n_levels
        off, res, ml, bv, Rb = _tables(x, enc.offsets_list, enc.resolutions_list, 0, L, None)
        emb = torch.where(enc.params.detach() >= 0, 1.0, -1.0).contiguous()
        g = torch.randn(L, N, F, device="cuda")
        fi, ff, fb = [], [], []
        for it in range(reps + 3):
            with torch.no_grad():
                t_i, y0 = timed(lambda: grid_encode(x, emb, enc.offsets_list, enc.resolutions_list, False, 0, L))
            xi, ei = x.clone().requires_grad_(True), emb.clone().requires_grad_(True)
            t_f, y = timed(lambda: _GridEncode.apply(xi, ei, off, res, ml, bv, Rb, L, True))
            ge, gi = torch.zeros_like(emb), torch.empty_like(x)
            t_b, _ = timed(lambda: _gridencoder.backward_into(g, x, emb, off, res, ge, gi, F, L, Rb, bv, ml))
            if it >= 3:
                fi.append(t_i); ff.append(t_f); fb.append(t_b)
        assert torch.equal(y0, y.detach())
        # contributions per row: the key pass's rule restated in torch (float32 placement as on the device)
        cnt = torch.zeros(emb.shape[0], dtype=torch.int64, device="cuda")
        for l in range(L):
            r = int(enc.resolutions_list[l]); o = int(enc.offsets_list[l]); hms = int(enc.offsets_list[l + 1]) - o
            pos = x * float(r - 2) + 0.5
            pg = torch.floor(pos).long()
            for c in range(8):
                pl = torch.stack([torch.clamp(pg[:, d] + ((c >> d) & 1), max=r - 1) for d in range(3)], 1)
                use = ~((pl == 0) | (pl == r - 1)).any(1)
                if r ** 3 <= hms:
                    idx = pl[:, 0] + pl[:, 1] * r + pl[:, 2] * r * r
                else:
                    idx = (pl[:, 0] ^ ((pl[:, 1] * 2654435761) & 0xFFFFFFFF) ^ ((pl[:, 2] * 805459861) & 0xFFFFFFFF))
                cnt += torch.bincount(o + (idx[use] % hms), minlength=emb.shape[0])
        used = cnt[cnt > 0].double()
        print(f"{N} anchors  F={F}  L={L}  pairs={int(cnt.sum())}  rows used {used.numel()}/{emb.shape[0]}  contributions per used row: "
              f"median {float(used.median()):.0f}  max {int(used.max())}")
        print(f"  inference forward (gsge_forward)        {statistics.median(fi):.3f} ms  (min {min(fi):.3f})")
        print(f"  forward, gradient path (_GridEncode)    {statistics.median(ff):.3f} ms  (min {min(ff):.3f})")
        print(f"  backward (gsge_backward, both grads)    {statistics.median(fb):.3f} ms  (min {min(fb):.3f})", flush=True)
