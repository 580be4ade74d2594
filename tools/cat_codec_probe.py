#!/usr/bin/env python
"""CAT-3DGS's attribute bitstream, measured: gauspcc_amd.cat_codec as whole calls, and the attribute part of the decode on the pipelined chain
kernel (gsac_decode_normal_chain) against the staged path (gshac_mlp2 + decoder_gaussian_slices, stage after stage).

    python tools/cat_codec_probe.py [--out profiles/r07_cat_codec.txt] [--sizes 100000 1000000]

Groups [12, 12, 13, 13], without and with the scaling / offsets MLPs.  Every size is a child process under its own time limit; the driver stops at
the first step that fails.  Timings: the median of REPEATS calls after a warm-up, wall clock around a device synchronisation, with the min .. max
spread.  The attribute part reads the files of the whole-call encode (file reads included on both sides) and is checked to give equal tensors.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
GROUPS = (12, 12, 13, 13)
RESOLUTION = 64
BLOCKS = (4, 8, 16, 32)


def _sync_time(torch, fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _med(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def _quiet(fn, *a, **kw):
    import contextlib
    import io

    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _fresh(torch, m, flags):
    import copy

    from gauspcc_amd.synth import SyntheticGaussianModelCAT

    d = SyntheticGaussianModelCAT(64, seed=9, chcm_slices_list=GROUPS, chcm_for_scaling=flags, chcm_for_offsets=flags, resolution=RESOLUTION, device="cuda:0")
    d.feature_net = copy.deepcopy(m.feature_net)
    d.mlp_chcm_list = m.mlp_chcm_list
    for name in ("mlp_chcm_scaling", "mlp_chcm_offsets"):
        if hasattr(m, name):
            setattr(d, name, getattr(m, name))
    return d


def step_size(n, out_json):
    import torch

    from gauspcc_amd import arm_codec, cat_codec
    from gauspcc_amd.synth import SyntheticGaussianModelCAT

    res = dict(n=n, configs=[])
    for flags in (False, True):
        mk = lambda k, seed: SyntheticGaussianModelCAT(k, seed=seed, chcm_slices_list=GROUPS, chcm_for_scaling=flags, chcm_for_offsets=flags,   # noqa: E731
                                                       resolution=RESOLUTION, scaling_spread=0.05, device="cuda:0")
        warm = mk(3000, 1)
        with tempfile.TemporaryDirectory() as d:
            p, _, _ = _quiet(cat_codec.conduct_encoding, warm, d, None, ckpt_path="synthetic")
            for chain in (True, False):
                _quiet(cat_codec.conduct_decoding, _fresh(torch, warm, flags), d, p, None, ckpt_path="synthetic", chain=chain)
        m = mk(n, 3)
        r = dict(flags=flags)
        with tempfile.TemporaryDirectory() as d, torch.no_grad():
            enc_t, dec_t = [], {True: [], False: []}
            for _ in range(REPEATS):
                dt, (patched, _, _) = _sync_time(torch, lambda: _quiet(cat_codec.conduct_encoding, m, d, None, ckpt_path="synthetic"))
                enc_t.append(dt)
                for chain in (True, False):
                    fresh = _fresh(torch, m, flags)
                    dt, _ = _sync_time(torch, lambda: _quiet(cat_codec.conduct_decoding, fresh, d, patched, None, ckpt_path="synthetic", chain=chain))
                    dec_t[chain].append(dt)
            N = patched[1]
            steps = -(-N // 500)
            names = [f"feat{i}" for i in range(len(GROUPS))] + ["scaling", "offsets"]
            r.update(N=N, steps=steps, encode=_med(enc_t), decode_chain=_med(dec_t[True]), decode_staged=_med(dec_t[False]),
                     attr_bytes=sum(os.path.getsize(os.path.join(d, f"{a}_{s}.b")) for a in names for s in range(steps)))
            # the attribute part alone, on the decoder's own inputs
            planes = arm_codec.decode_triplane(m.feature_net.attribute_net.grid, d, patched[11])
            anchor = fresh._anchor.data
            stages = cat_codec.stage_table(m)
            dt_ctx, ctx = _sync_time(torch, lambda: cat_codec._context(m, anchor, planes))
            Q = cat_codec._step_sizes(m, ctx)
            K = m.n_offsets
            keep = fresh._mask.data.view(N, K).to(torch.bool)
            mask = keep.unsqueeze(-1).repeat(1, 1, 3).view(N, 3 * K)
            bounds = cat_codec.slice_bounds(N)
            mins = {f"feat{i}": patched[4][i] for i in range(len(GROUPS))}; mins.update(scaling=patched[6], offsets=patched[8])
            maxs = {f"feat{i}": patched[5][i] for i in range(len(GROUPS))}; maxs.update(scaling=patched[7], offsets=patched[9])
            staged_fn = lambda: cat_codec.decode_staged(stages, ctx, Q, mask, bounds, d, steps, mins, maxs, N, m.feat_dim, K)                     # noqa: E731
            chain_fn = lambda b: cat_codec.decode_chain(stages, ctx, Q, keep, d, steps, mins, maxs, N, m.feat_dim, K, block_anchors=b)           # noqa: E731
            want = staged_fn()
            r["context_s"] = dt_ctx
            r["staged"] = _med([_sync_time(torch, staged_fn)[0] for _ in range(REPEATS)])
            r["chain"] = {}
            for b in (0,) + BLOCKS:
                got = chain_fn(b)
                r["chain"][str(b)] = dict(_med([_sync_time(torch, lambda: chain_fn(b))[0] for _ in range(REPEATS)]),
                                          equal=all(bool(torch.equal(got[k], want[k])) for k in want))
            r["exact"] = bool(torch.equal(fresh._anchor_feat.data, want["feat"]) and torch.equal(fresh._scaling.data, want["scaling"]))
        res["configs"].append(r)
        del m
        torch.cuda.empty_cache()
    json.dump(res, open(out_json, "w"))


def _fmt(t, unit=1e3):
    return f"{t['median'] * unit:9.2f} ms  (min {t['min'] * unit:.2f} .. max {t['max'] * unit:.2f})"


def report(sizes, out):
    L = ["CAT-3DGS attribute bitstream: gauspcc_amd.cat_codec, and gsac_decode_normal_chain against the staged decode",
         f"(tools/cat_codec_probe.py; medians of {REPEATS} calls after a warm-up, wall clock around a device synchronisation; synthetic models, groups",
         f" {list(GROUPS)}, feat_dim 50, 10 offsets, 500 anchors per slice, tri-plane 72 channels at {RESOLUTION} and {2 * RESOLUTION}, head 432-100-175)", ""]
    for res in sizes:
        for r in res["configs"]:
            S = len(GROUPS) + 2
            L += [f"== {res['n']} anchors ({r['N']} kept, {r['steps']} slices, {S} stages), scaling / offsets MLPs {'ON' if r['flags'] else 'off'}",
                  f"conduct_encoding (whole call: geometry, planes, attributes)  {_fmt(r['encode'])}",
                  f"conduct_decoding, chain=True  (whole call)                   {_fmt(r['decode_chain'])}",
                  f"conduct_decoding, chain=False (whole call)                   {_fmt(r['decode_staged'])}",
                  f"  context of the decode, one pass over all anchors           {r['context_s'] * 1e3:9.2f} ms (single call)",
                  f"  attribute part, staged: {S} x (gshac_mlp2 +) decoder_gaussian_slices  {_fmt(r['staged'])}",
                  ]
            for b, t in r["chain"].items():
                label = "default" if b == "0" else f"B = {b:>2}"
                L += [f"  attribute part, chain kernel, {label:>7}: {_fmt(t)}   staged / chain {r['staged']['median'] / t['median']:.2f} x   equal tensors: {t['equal']}"]
            L += [f"  attribute bytes {r['attr_bytes']}; whole-call round trip equals the staged tensors: {r['exact']}", ""]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write("\n".join(L))
    print("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_cat_codec.txt"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--step", choices=["size"])
    ap.add_argument("--n", type=int)
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.step == "size":
        return step_size(a.n, a.json)
    results = []
    with tempfile.TemporaryDirectory() as d:
        for n in a.sizes:
            js = os.path.join(d, f"size_{n}.json")
            # a fresh child under its own time limit; a step that fails or runs out of time ends the probe (nothing more is started on the GPU)
            rc = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step", "size", "--n", str(n), "--json", js]).returncode
            if rc != 0:
                print(f"size {n} ended with status {rc}: stopping", file=sys.stderr)
                return rc
            results.append(json.load(open(js)))
    report(results, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
