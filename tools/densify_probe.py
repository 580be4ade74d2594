#!/usr/bin/env python3
"""Developer probe: gauspcc_amd.densify.training_statis and adjust_anchor (growing stubbed: 5 % zero rows appended, pruning a no-op) at
100 k and 1 M anchors, K = 10, about half the anchors visible, beside the frameworks' torch sequence (tests/densify_ref.py:
torch_sequence_statis / torch_sequence_adjust) on the same tensors on the same GPU.  Per call: stream time between two events and host
wall time up to a final synchronise, medians and spread of `reps` after warm-up, the two programs alternating.  For training_statis also
the bytes the update needs at least, its achieved bytes/s and its share of the achievable HBM rate.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel table (`--no-ref` leaves the torch sequence out of that run).
    python tools/densify_probe.py [reps] [--no-ref]"""
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gauspcc_amd import densify  # noqa: E402
from tests import densify_ref as dr  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 20
ref = "--no-ref" not in sys.argv
DEV = "cuda:0"
HBM_ACHIEVABLE = 6.3e12      # bytes/s


def timed(fn, setup=None):
    if setup:
        setup()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def spread(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def compare(programs):
    """programs: name -> (fn, setup); warm-up twice each, then `reps` rounds alternating between them"""
    for fn, setup in programs.values():
        for _ in range(2):
            timed(fn, setup)
    t = {k: [] for k in programs}
    for _ in range(reps):
        for k, (fn, setup) in programs.items():
            t[k].append(timed(fn, setup))
    return {k: {"stream_ms": spread([x[0] for x in v]), "wall_ms": spread([x[1] for x in v])} for k, v in t.items()}


class Model:
    def __init__(self, N, K):
        self.__dict__.update(vars(dr.model(N, K, torch.float32, lib="torch", device=DEV)))
        self.n, self.grow = N, N // 20

    get_anchor = property(lambda self: torch.empty(self.n, 3, device=DEV))

    def anchor_growing(self, grads_norm, threshold, offset_mask):
        for k in ("opacity_accum", "anchor_demon"):
            setattr(self, k, torch.cat([getattr(self, k), torch.zeros(self.grow, 1, device=DEV)], dim=0))
        self.n += self.grow

    def prune_anchor(self, mask):
        pass


for N in (100_000, 1_000_000):
    K = 10
    g = torch.Generator(device=DEV).manual_seed(N)
    vis = torch.rand(N, device=DEV, generator=g) < 0.5
    V = int(vis.sum())
    opacity = torch.randn(V * K, 1, device=DEV, generator=g)
    sel = (opacity > 0).view(-1)
    S = int(sel.sum())
    filt = torch.rand(S, device=DEV, generator=g) < 0.7
    P = int(filt.sum())
    vp = types.SimpleNamespace(grad=torch.randn(S, 3, device=DEV, generator=g) * 0.001)
    ours, theirs = Model(N, K), Model(N, K)
    progs = {"densify": (lambda: densify.training_statis(ours, vp, opacity, filt, sel, vis), None)}
    if ref:
        progs["torch_sequence"] = (lambda: dr.torch_sequence_statis(theirs, vp.grad, opacity, filt, sel, vis), None)
    row = {"case": "training_statis", "anchors": N, "K": K, "visible": V, "selected": S, "passing": P, **compare(progs)}
    densify.check(DEV)
    # what the update must move at least: the visible mask; per visible anchor opacity and selection rows and two accumulators read and
    # written; per selected entry its filter byte; per passing entry two grad floats and two accumulators read and written
    row["min_bytes"] = N + V * (5 * K + 16) + S + P * (8 + 16)
    row["scan_bytes"] = 24 * (N + 1) + 4 * N + 4 * V     # the two rank arrays: written, scanned in place, read by the update
    sec = row["densify"]["stream_ms"]["median"] * 1e-3
    row["achieved_TBps_min_bytes"] = round(row["min_bytes"] / sec / 1e12, 4)
    row["share_of_achievable_hbm"] = round(row["min_bytes"] / HBM_ACHIEVABLE / sec, 4)
    print(json.dumps(row), flush=True)

    # adjust_anchor on accumulators of three iterations (those of `ours`, copied before every repetition: both programs replace them)
    for _ in range(2):
        densify.training_statis(ours, vp, opacity, filt, sel, vis)
    saved = {k: getattr(ours, k).clone() for k in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")}
    kw = dict(check_interval=3, success_threshold=0.5, grad_threshold=0.0002, min_opacity=1.5)

    def reset(m):
        def f():
            for k, v in saved.items():
                setattr(m, k, v.clone())
            m.n = N
        return f

    progs = {"densify": (lambda: densify.adjust_anchor(ours, **kw), reset(ours))}
    if ref:
        progs["torch_sequence"] = (lambda: dr.torch_sequence_adjust(theirs, Model.anchor_growing, **kw), reset(theirs))
    row = {"case": "adjust_anchor", "anchors": N, "K": K, "appended": N // 20, **compare(progs)}
    row["survivors"] = int(ours.anchor_demon.shape[0])
    if ref:
        assert theirs.anchor_demon.shape[0] == row["survivors"]
    print(json.dumps(row), flush=True)
