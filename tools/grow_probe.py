#!/usr/bin/env python3
"""Developer probe: gpcc_grow_voxels (gauspcc_amd.growing.grow_voxels) and gpcc_scatter_max (gauspcc_amd.scatter.scatter_max) at HAC's
scale -- 1 M anchors, 10 offsets, feat_dim 50, HAC's three voxel sizes -- timed with CUDA events on the stream (median and spread of
`reps` after warm-up), beside the reference's torch sequence (anchor_growing's body, HAC/scene/gaussian_model.py:836-874, with scatter_max
as scatter_reduce "amax") on the same GPU, and the one-voxel skewed case.  Run it under `rocprofv3 --kernel-trace --stats` for the
kernel table (`--no-ref` leaves the torch sequence out of that run).
    python tools/grow_probe.py [reps] [--no-ref]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gauspcc_amd.growing import grow_voxels  # noqa: E402
from gauspcc_amd.scatter import scatter_max  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 10
ref = "--no-ref" not in sys.argv
FLT_MAX = torch.finfo(torch.float32).max


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(fn, n=reps):
    fn()
    fn()
    t = sorted(timed(fn) for _ in range(n))
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}


def torch_sequence(selected_xyz, anchor, cur_size, feat, mask, K):
    F = feat.shape[1]
    grid_coords = torch.round(anchor / cur_size).int()
    sel = torch.round(selected_xyz / cur_size).int()
    uniq, inverse = torch.unique(sel, return_inverse=True, dim=0)
    dup = torch.zeros(uniq.shape[0], dtype=torch.bool, device="cuda")
    for c in range(0, grid_coords.shape[0], 4096):
        dup |= (uniq.unsqueeze(1) == grid_coords[c:c + 4096]).all(-1).any(-1)
    keep = ~dup
    cand = uniq[keep] * cur_size
    nf = feat.unsqueeze(1).repeat(1, K, 1).view(-1, F)[mask]
    m = torch.full((uniq.shape[0], F), -FLT_MAX, device="cuda").scatter_reduce(0, inverse.unsqueeze(1).expand(-1, F), nf, "amax", include_self=False)
    return cand, m.masked_fill(m == -FLT_MAX, 0.0)[keep]


g = torch.Generator(device="cuda").manual_seed(0)
N, K, F, voxel_size = 1_000_000, 10, 50, 0.01
anchor = torch.round(torch.rand(N, 3, device="cuda", generator=g) * 20 / voxel_size) * voxel_size
offset = torch.randn(N, K, 3, device="cuda", generator=g) * 0.5
scaling = torch.rand(N, 3, device="cuda", generator=g) * 0.05
feat = torch.randn(N, F, device="cuda", generator=g)
mask = torch.rand(N * K, device="cuda", generator=g) > 0.7   # ~3 M candidates
all_xyz = (anchor.unsqueeze(1) + offset * scaling.unsqueeze(1)).view(-1, 3)
selected = all_xyz[mask].contiguous()
rows = torch.nonzero(mask).squeeze(1) // K
M = selected.shape[0]
for i in range(3):
    cur_size = voxel_size * (16 // 4 ** i)
    na, nf = grow_voxels(selected, anchor, cur_size, feat, rows)
    row = {"case": "hac", "level": i, "cur_size": cur_size, "anchors": N, "candidates": M, "new_anchors": na.shape[0],
           "grow_voxels": stats(lambda: grow_voxels(selected, anchor, cur_size, feat, rows))}
    # bytes the kernels must move at least: candidates and rows read, the feature rows gathered (4 F per candidate), anchors read, outputs
    row["min_bytes"] = 12 * M + 8 * M + 4 * F * M + 12 * N + (12 + 4 * F) * na.shape[0]
    if ref and i > 0:   # the coarsest level's unique set against 1 M anchors takes the longest; one repetition each
        row["torch_sequence"] = stats(lambda: torch_sequence(selected, anchor, cur_size, feat, mask, K), 1)
    print(json.dumps(row), flush=True)

# scatter_max alone, HAC's call shape: (candidates, 50) rows with an expanded index over the unique voxels of the finest level
uniq, inverse = torch.unique(torch.round(selected / voxel_size).int(), return_inverse=True, dim=0)
src = feat[rows].contiguous()
idx = inverse.unsqueeze(1).expand(-1, F)
print(json.dumps({"case": "scatter_max", "rows": M, "cols": F, "slots": uniq.shape[0],
                  "scatter_max": stats(lambda: scatter_max(src, idx, dim=0, dim_size=uniq.shape[0]))}), flush=True)

# skew: every candidate in one voxel
one = torch.rand(M, 3, device="cuda", generator=g) * 0.001
none = torch.zeros(0, 3, device="cuda")
zero = torch.zeros(M, dtype=torch.int64, device="cuda")
print(json.dumps({"case": "one_voxel", "candidates": M, "grow_voxels": stats(lambda: grow_voxels(one, none, 1.0, feat, rows)),
                  "scatter_max": stats(lambda: scatter_max(src, zero, dim=0, dim_size=1))}), flush=True)
