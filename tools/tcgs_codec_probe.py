#!/usr/bin/env python
"""TC-GS's attribute bitstream, measured: gauspcc_amd.tcgs_codec against the loop a TC-GS user ran before it existed.

    python tools/tcgs_codec_probe.py [--out profiles/r07_tcgs_codec.txt] [--sizes 100000 1000000]

"Before" is the reference's own loop (TC-GS/scene/gaussian_model.py:1197-1271, 1358-1420) restated here on this library's drop-ins: per
1 000-anchor slice the Triplane module, mlp_triplane as torch's nn.Sequential, then torchac_encodings.encoder_gaussian / decoder_gaussian per
attribute (table built and integerised on the device, shipped, coded by one host thread).  It runs over ALL slices of the scene, once (a loop of
seconds is its own average over hundreds of slices).  Only when its first PARENT_SLICES slices project a loop longer than PARENT_LIMIT_S is it
left at those slices and scaled; the profile then says so on the loop's own lines.  Every GPU step is a child process under its own time limit;
the driver stops at the first step that fails.  Other timings: the median of REPEATS calls after a warm-up, with the min .. max spread.
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

PARENT_SLICES = 40
PARENT_LIMIT_S = 180.0
REPEATS = 3
MLP_SHAPES = ((603, 100, 175), (300, 100, 175), (128, 100, 175), (256, 64, 32), (100, 64, 20), (64, 64, 64))     # TC-GS's layer, then narrower layers of its class
K = 4


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


def _sorted_inputs(torch, m):
    """what conduct_encoding codes, in its order (the Morton order of the kept anchors)"""
    from gauspcc_amd.pcc_utils import calculate_morton_order

    keep = m.get_mask_anchor
    a_int = torch.round(m.get_anchor[keep] / m.voxel_size)
    order = calculate_morton_order(a_int)
    return dict(anchor=a_int[order] * m.voxel_size, feat=m._anchor_feat[keep][order], scaling=m.get_scaling[keep][order], offs=m._offset[keep][order],
                mask=m.get_mask[keep][order])


def _parent_slice_context(torch, m, rows):
    ctx = m.triplane(rows.unsqueeze(1).repeat(1, K, 1), m.x_bound_max, m.x_bound_min)
    out = m.get_tri_mlp(torch.cat([ctx, rows], dim=1))
    fd, no = m.feat_dim, m.n_offsets
    mean, scale, mean_s, scale_s, mean_o, scale_o, qf, qs, qo = torch.split(out, [fd, fd, 6, 6, 3 * no, 3 * no, 1, 1, 1], dim=-1)
    flat = lambda t: t.contiguous().view(-1)
    return dict(feat=(flat(mean), torch.clamp(flat(scale), min=1e-9), 1 * (1 + torch.tanh(qf.contiguous().repeat(1, fd).view(-1)))),
                scaling=(flat(mean_s), torch.clamp(flat(scale_s), min=1e-9), 0.001 * (1 + torch.tanh(qs.contiguous().repeat(1, 6).view(-1)))),
                offsets=(flat(mean_o), torch.clamp(flat(scale_o), min=1e-9), 0.2 * (1 + torch.tanh(qo.contiguous().repeat(1, 3 * no).view(-1)))))


def _parent_loop(torch, m, src, path, nslices):
    """the loop of the module docstring over the first nslices slices: (encode seconds, decode seconds, split, bytes, exact?)"""
    from gauspcc_amd import torchac_encodings as te
    from gauspcc_amd.anchor_codec import ste_multistep

    N, no = src["anchor"].shape[0], m.n_offsets
    means = {k: src[k].mean() for k in ("feat", "scaling", "offs")}
    t = dict(enc_context=0.0, enc_coder=0.0, dec_context=0.0, dec_coder=0.0)
    infos, nbytes, exact = [], 0, True
    for s in range(nslices):
        sl = slice(s * 1000, min((s + 1) * 1000, N))
        dt, c = _sync_time(torch, lambda: _parent_slice_context(torch, m, src["anchor"][sl]))
        t["enc_context"] += dt
        mask = src["mask"][sl].repeat(1, 1, 3).view(-1, 3 * no).view(-1).to(torch.bool)
        x = dict(feat=ste_multistep(src["feat"][sl].reshape(-1), c["feat"][2], means["feat"]),
                 scaling=ste_multistep(src["scaling"][sl].reshape(-1), c["scaling"][2], means["scaling"]),
                 offsets=ste_multistep(src["offs"][sl].reshape(-1), c["offsets"][2], means["offs"])[mask])

        def enc():
            out = {}
            for k in ("feat", "scaling", "offsets"):
                p = tuple(v[mask] for v in c[k]) if k == "offsets" else c[k]
                out[k] = te.encoder_gaussian(x[k], *p, file_name=os.path.join(path, f"{k}_{s}.b"))
            return out
        dt, info = _sync_time(torch, enc)
        t["enc_coder"] += dt
        infos.append((info, x, mask))
        nbytes += sum(os.path.getsize(os.path.join(path, f"{k}_{s}.b")) for k in ("feat", "scaling", "offsets"))
    for s in range(nslices):
        sl = slice(s * 1000, min((s + 1) * 1000, N))
        info, x, mask = infos[s]
        dt, c = _sync_time(torch, lambda: _parent_slice_context(torch, m, src["anchor"][sl]))
        t["dec_context"] += dt

        def dec():
            out = {}
            for k in ("feat", "scaling", "offsets"):
                p = tuple(v[mask] for v in c[k]) if k == "offsets" else c[k]
                out[k] = te.decoder_gaussian(*p, file_name=os.path.join(path, f"{k}_{s}.b"), min_value=info[k][1], max_value=info[k][2])
            return out
        dt, got = _sync_time(torch, dec)
        t["dec_coder"] += dt
        exact = exact and all(torch.equal(got[k], x[k]) for k in got)
    return t, nbytes, exact


def step_size(n, out_json):
    import numpy as np
    import torch

    from gauspcc_amd import anchor_codec, arithmetic, tcgs_codec
    from gauspcc_amd import torchac_encodings as te
    from gauspcc_amd.encodings_cuda import _read_files, _write_files
    from gauspcc_amd.anchor_codec import ste_multistep
    from gauspcc_amd.synth import SyntheticGaussianModelTC

    res = dict(n=n)
    warm = SyntheticGaussianModelTC(3000, seed=1, resolution=64, device="cuda:0")
    with tempfile.TemporaryDirectory() as d:
        p, _ = _quiet(tcgs_codec.conduct_encoding, warm, d, ckpt_path="synthetic")
        _quiet(tcgs_codec.conduct_decoding, warm, d, p, ckpt_path="synthetic")
    m = SyntheticGaussianModelTC(n, seed=3, resolution=256, device="cuda:0")
    src = _sorted_inputs(torch, m)
    N, no, fd = src["anchor"].shape[0], m.n_offsets, m.feat_dim
    steps = -(-N // 1000)
    res.update(N=N, steps=steps)

    # ---- here: whole calls
    enc_t, dec_t = [], []
    with tempfile.TemporaryDirectory() as d:
        for _ in range(REPEATS):
            dt, (patched, _) = _sync_time(torch, lambda: _quiet(tcgs_codec.conduct_encoding, m, d, ckpt_path="synthetic"))
            enc_t.append(dt)
            fresh = SyntheticGaussianModelTC(64, seed=9, resolution=256, device="cuda:0")
            fresh.triplane, fresh.mlp_triplane, fresh.x_bound_min, fresh.x_bound_max = m.triplane, m.mlp_triplane, m.x_bound_min, m.x_bound_max
            dt, _ = _sync_time(torch, lambda: _quiet(tcgs_codec.conduct_decoding, fresh, d, patched, ckpt_path="synthetic"))
            dec_t.append(dt)
        res["new_exact"] = bool(torch.equal(fresh._anchor.data, src["anchor"]) and torch.equal(fresh._mask.data, src["mask"]))
        attr_files = [f for f in os.listdir(d) if f.split("_")[0] in ("feat", "scaling", "offsets")]
        res["new_attr_bytes"] = sum(os.path.getsize(os.path.join(d, f)) for f in attr_files)
        res["new_files"] = len(attr_files)
        new_first = {f: open(os.path.join(d, f), "rb").read() for f in attr_files if int(f.split("_")[1][:-2]) < 5}
        slice_bytes = [0] * steps
        for f in attr_files:
            slice_bytes[int(f.split("_")[1][:-2])] += os.path.getsize(os.path.join(d, f))
    res["new_encode"], res["new_decode"] = _med(enc_t), _med(dec_t)

    # ---- here: the parts (context, coder, file I/O), measured apart from the calls above
    bounds = anchor_codec.slice_bounds(N, 1000)
    ctx_t = [_sync_time(torch, lambda: tcgs_codec._context(m, src["anchor"]))[0] for _ in range(REPEATS)]
    c = tcgs_codec._context(m, src["anchor"])
    mask = anchor_codec.offsets_mask(src["mask"])
    xs = dict(feat=ste_multistep(src["feat"].reshape(-1), c["Q_feat"], src["feat"].mean()),
              scaling=ste_multistep(src["scaling"].reshape(-1), c["Q_scaling"], src["scaling"].mean()),
              offsets=ste_multistep(src["offs"].reshape(-1), c["Q_offsets"], src["offs"].mean())[mask])
    par = dict(feat=(c["mean"], c["scale"], c["Q_feat"]), scaling=(c["mean_scaling"], c["scale_scaling"], c["Q_scaling"]),
               offsets=tuple(v[mask].contiguous() for v in (c["mean_offsets"], c["scale_offsets"], c["Q_offsets"])))
    ss = dict(feat=[b * fd for b in bounds], scaling=[b * 6 for b in bounds], offsets=anchor_codec.offset_bounds(mask, N, bounds))
    enc_c, dec_c, wr_t, rd_t = [], [], [], []
    for _ in range(REPEATS):
        dt, coded = _sync_time(torch, lambda: {k: arithmetic.encode_normal_streams(xs[k].contiguous(), *par[k], ss[k]) for k in xs})
        enc_c.append(dt)
        dt, back = _sync_time(torch, lambda: {k: arithmetic.decode_normal_streams(*par[k], ss[k], *coded[k]) for k in xs})
        dec_c.append(dt)
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            for k in xs:
                mn, mx, data, cnt = coded[k]
                off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
                blob = data.tobytes()
                _write_files([(os.path.join(d, f"{k}_{i}.b"), blob[int(off[i]):int(off[i + 1])]) for i in range(steps)])
            wr_t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for k in xs:                                   # as decoder_gaussian_slices reads them: one _read_files call per attribute
                _, offs = _read_files([os.path.join(d, f"{k}_{i}.b") for i in range(steps)])
                assert offs[steps] == int(coded[k][3].sum())
            rd_t.append(time.perf_counter() - t0)
    res["new_coder_exact"] = all(bool(torch.equal(back[k], xs[k])) for k in xs)
    res.update(new_context=_med(ctx_t), new_enc_coder=_med(enc_c), new_dec_coder=_med(dec_c), new_write=_med(wr_t), new_read=_med(rd_t))
    res["symbols"] = {k: int(xs[k].numel()) for k in xs}

    # ---- row entries: the library's table against the torch-built one, first slices of every attribute
    entries = differing = worst = 0
    for k in xs:
        for i in range(min(steps, 3)):
            a, b = ss[k][i], ss[k][i + 1]
            if b == a:
                continue
            mn, mx = int(coded[k][0][i]), int(coded[k][1][i])
            p = tuple(v[a:b].contiguous() for v in par[k])
            dlt = ((arithmetic.normal_cdf_rows(*p, mn, mx).to(torch.int32) & 0xFFFF) - (te._int_rows(*p, mn, mx).to(torch.int32) & 0xFFFF)).abs()
            dlt = torch.minimum(dlt, 65536 - dlt)
            entries += dlt.numel(); differing += int((dlt != 0).sum()); worst = max(worst, int(dlt.max()))
    res.update(row_entries=entries, row_differing=differing, row_worst=worst)

    # ---- the files of the parent's coder on the SAME context: the first five slices of every attribute
    same = total = 0
    with tempfile.TemporaryDirectory() as d:
        for k in xs:
            for i in range(min(steps, 5)):
                a, b = ss[k][i], ss[k][i + 1]
                if b == a:
                    continue
                f = os.path.join(d, "p.b")
                te.encoder_gaussian(xs[k][a:b], *(v[a:b] for v in par[k]), file_name=f)
                total += 1
                same += int(open(f, "rb").read() == new_first[f"{k}_{i}.b"])
    res.update(parent_coder_files=total, parent_coder_files_identical=same)

    # ---- before: the per-slice loop
    nsl = min(steps, PARENT_SLICES)
    with tempfile.TemporaryDirectory() as d:
        _parent_loop(torch, m, src, d, 1)                                  # warm-up
        t, nbytes, exact = _parent_loop(torch, m, src, d, nsl)
        projected = sum(t.values()) * steps / nsl
        if nsl < steps and projected <= PARENT_LIMIT_S:                    # the whole loop, measured: what the documents quote
            nsl = steps
            t, nbytes, exact = _parent_loop(torch, m, src, d, nsl)
    res.update(parent_slices=nsl, parent=t, parent_bytes=nbytes, parent_exact=exact, new_bytes_first=sum(slice_bytes[:nsl]), parent_projected=projected)
    json.dump(res, open(out_json, "w"))


def step_mlp(out_json):
    import torch

    from gauspcc_amd import hac_codec

    n = 1_000_000
    g = torch.Generator(device="cuda").manual_seed(0)

    def timed(fn, reps=10):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return _med(ts)

    res = {}
    with torch.no_grad():
        for din, dh, dout in MLP_SHAPES:
            x = torch.randn(n, din, device="cuda", generator=g)
            w1, b1 = torch.randn(dh, din, device="cuda", generator=g) / din ** 0.5, torch.randn(dh, device="cuda", generator=g) * 0.1
            w2, b2 = torch.randn(dout, dh, device="cuda", generator=g) / dh ** 0.5, torch.randn(dout, device="cuda", generator=g) * 0.1
            lin = torch.nn.Sequential(torch.nn.Linear(din, dh), torch.nn.ReLU(), torch.nn.Linear(dh, dout)).cuda()
            res[f"{din}-{dh}-{dout}"] = dict(mlp2=timed(lambda: hac_codec.mlp2(x, w1, b1, w2, b2)), torch_sequential=timed(lambda: lin(x)))
            del x, lin
    json.dump(res, open(out_json, "w"))


def _fmt(t, unit=1e3):
    return f"{t['median'] * unit:9.2f} ms  (min {t['min'] * unit:.2f} .. max {t['max'] * unit:.2f})"


def report(sizes, mlp, out):
    L = ["TC-GS attribute bitstream: gauspcc_amd.tcgs_codec against the per-slice loop on the drop-ins that existed before it",
         f"(tools/tcgs_codec_probe.py; medians of {REPEATS} calls after a warm-up, wall clock around a device synchronisation; synthetic models,",
         " planes 3 x 50 x 256 x 256, mlp_triplane 603-100-175, feat_dim 50, 10 offsets, 1 000 anchors per slice)", ""]
    for r in sizes:
        scale = r["steps"] / r["parent_slices"]
        p = r["parent"]
        pe, pd = (p["enc_context"] + p["enc_coder"]) * scale, (p["dec_context"] + p["dec_coder"]) * scale
        L += [f"== {r['n']} anchors ({r['N']} kept, {r['steps']} slices; symbols feat {r['symbols']['feat']}, scaling {r['symbols']['scaling']}, offsets {r['symbols']['offsets']})",
              f"conduct_encoding (whole call, geometry included) {_fmt(r['new_encode'])}",
              f"conduct_decoding (whole call, geometry included) {_fmt(r['new_decode'])}",
              f"  context, one pass over all anchors              {_fmt(r['new_context'])}",
              f"  coder, encode: three device calls               {_fmt(r['new_enc_coder'])}",
              f"  coder, decode: three device calls               {_fmt(r['new_dec_coder'])}",
              f"  files: write {3 * r['steps']} (gpcc_write_files)            {_fmt(r['new_write'])}",
              f"  files: read them back (gpcc_read_files)         {_fmt(r['new_read'])}",
              f"  round trip exact: calls {r['new_exact']}, coder alone {r['new_coder_exact']}",
              (f"per-slice loop, attributes only, all {r['steps']} slices, run once:" if scale == 1 else
               f"per-slice loop, attributes only: NOT run whole (projected {r['parent_projected']:.0f} s); SCALED x {scale:.2f} from its first {r['parent_slices']} of {r['steps']} slices:"),
              f"  encode {pe * 1e3:9.2f} ms  (context {p['enc_context'] * scale * 1e3:.2f}, encoder_gaussian with its table and file {p['enc_coder'] * scale * 1e3:.2f})",
              f"  decode {pd * 1e3:9.2f} ms  (context {p['dec_context'] * scale * 1e3:.2f}, decoder_gaussian with its table and file {p['dec_coder'] * scale * 1e3:.2f})",
              f"  round trip exact: {r['parent_exact']}",
              f"ratio, loop (attributes only{'' if scale == 1 else ', scaled'}) / whole call here: encode {pe / r['new_encode']['median']:.1f} x, decode {pd / r['new_decode']['median']:.1f} x",
              f"attribute bytes: here {r['new_attr_bytes']} in {r['new_files']} files; first {r['parent_slices']} slices: here {r['new_bytes_first']}, the loop {r['parent_bytes']}"
              f" (the loop's context is torch's nn.Sequential, whose last bits differ from gshac_mlp2's: step sizes, and so a few symbols, differ)",
              f"the loop's coder on this codec's context, first slices: {r['parent_coder_files_identical']} of {r['parent_coder_files']} files byte-identical",
              f"row entries, library table against torch-built table: {r['row_differing']} of {r['row_entries']} differ"
              f" (share {r['row_differing'] / max(r['row_entries'], 1):.3e}, largest difference {r['row_worst']})", ""]
    if mlp:
        L += ["== gshac_mlp2_act in the wide matrix-pipe class k_mlp2_mfma_wide (din <= 608, dh <= 100, dout <= 176) against the plain kernel k_mlp2",
              "(1 000 000 rows, device time, 10 runs after 3; each dispatch in a process of its own, the plain one under GAUSPCC_DEV=1 GAUSPCC_MLP2_MFMA=0;",
              " the first shape is TC-GS's mlp_triplane, the others are narrower layers the class takes as well; torch's float32 nn.Sequential for scale)"]
        for shape in mlp["class"]:
            cls, plain = mlp["class"][shape]["mlp2"], mlp["plain"][shape]["mlp2"]
            L += [f"{shape}:",
                  f"  class {_fmt(cls)}",
                  f"  plain {_fmt(plain)}",
                  f"  torch {_fmt(mlp['class'][shape]['torch_sequential'])}",
                  f"  class / plain: {plain['median'] / cls['median']:.2f} x faster; the two ranges {'do not overlap' if cls['max'] < plain['min'] else 'OVERLAP'}"]
        L += [""]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write("\n".join(L))
    print("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_tcgs_codec.txt"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--step", choices=["size", "mlp"])
    ap.add_argument("--n", type=int)
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.step == "size":
        return step_size(a.n, a.json)
    if a.step == "mlp":
        return step_mlp(a.json)
    results, mlp = [], {}
    plain_env = dict(os.environ, GAUSPCC_DEV="1", GAUSPCC_MLP2_MFMA="0")      # the developer switch that sends every layer to k_mlp2
    with tempfile.TemporaryDirectory() as d:
        jobs = [(["--step", "size", "--n", str(n)], os.path.join(d, f"size_{n}.json"), 420, None, None) for n in a.sizes]
        jobs += [(["--step", "mlp"], os.path.join(d, "mlp_class.json"), 180, None, "class"), (["--step", "mlp"], os.path.join(d, "mlp_plain.json"), 180, plain_env, "plain")]
        for args, js, limit, env, tag in jobs:
            # a fresh child under its own time limit; a step that fails or runs out of time ends the probe (nothing more is started on the GPU)
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args + ["--json", js], env=env).returncode
            if rc != 0:
                print(f"step {args} ended with status {rc}: stopping", file=sys.stderr)
                return rc
            if args[1] == "size":
                results.append(json.load(open(js)))
            else:
                mlp[tag] = json.load(open(js))
    report(results, mlp, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
