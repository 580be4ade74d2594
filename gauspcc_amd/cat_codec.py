"""GaussianModel.conduct_encoding / conduct_decoding / estimate_final_bits of CAT-3DGS (src/gs_compress/CAT-3DGS/scene/gaussian_model.py:1056-1616)
on the gfx950 kernels.  The three functions take the model as their first argument and touch it only through the attributes the reference
methods touch, so they bind as methods:

    from gauspcc_amd import cat_codec
    GaussianModel.conduct_encoding = cat_codec.conduct_encoding        # (self, pre_path_name, weighted_mask, ckpt_path=None)
    GaussianModel.conduct_decoding = cat_codec.conduct_decoding        # (self, pre_path_name, patched_infos, weighted_mask, ckpt_path=None, chain=None)
    GaussianModel.estimate_final_bits = cat_codec.estimate_final_bits  # (self, weighted_mask)

Same files under `pre_path_name` (xyz_pcc.bin, feat{i}_{s}.b for every channel group i and 500-anchor slice s, scaling_{s}.b, offsets_{s}.b,
masks.b and the three tri-plane files per level of arm_codec.encode_triplane), the same twelve-element `patched_infos` (the feat bounds as
[group][slice] lists of 0-d tensors), the same log strings and `rate_set`, the same parameter replacement at the end of decoding.

What differs from TC-GS's loop (gauspcc_amd.tcgs_codec) is the CHANNEL-WISE CONTEXT MODEL: `feat` is cut into `chcm_slices_list` groups and
group i > 0 is coded under mean_i + dmean, clamp(scale_i + dscale, 1e-9) with (dmean | dscale) = mlp_chcm_list[i - 1](groups 0 .. i - 1 as
decoded); with chcm_for_scaling / chcm_for_offsets, scaling and offsets depend the same way on all decoded channels.  A STAGE is one such
stream per slice; `stage_table` lists them with the columns of the 175-wide context row they read.

    anchors     calculate_morton_order + compress / decompress_point_cloud     gauspcc_amd.pcc_utils (gpcc_encode / gpcc_decode)
    context     self.feature_net(anchor, itr=-1) per slice                     ONCE over all anchors: the tri-plane sampler (gsge_msplane_forward)
                                                                               and, for Linear - ReLU - Linear, gshac_mlp2 (specified fp32 order)
    encoder     encoder_gaussian per slice and stage                           the stages are independent once feat is quantised: the channel-context
                                                                               MLPs through gshac_mlp2, one encoder_gaussian_slices call per stage
    decoder     decoder_gaussian per slice and stage, each waiting for the     chain=False: stage after stage, gshac_mlp2 + decoder_gaussian_slices
                one before                                                     chain=True:  gsac_decode_normal_chain -- ONE launch, a workgroup per
                                                                               slice, a wave per stage, the stages of a slice run as a pipeline
    bits        encoder / decoder (masks.b)                                    torchac_encodings.encoder / decoder

The decoder samples the context from the planes decode_triplane RETURNED (multiples of 1 / 16: the encoder's quantised planes exactly), not from
what the model's grids hold.  The attribute files are raw torchac streams written and read by this pair only (torchac_encodings.
encoder_gaussian_slices has the reason); byte compatibility with the reference's files is out of scope (its planes need `constriction`).
`ckpt_path`: the GausPcgc checkpoint (the reference looks beside its own sources; here the argument or $GAUSPCGC_CKPT).
The steps shared with HAC, HAC++ and TC-GS (slice geometry, xyz_pcc.bin, masks.b, fill back and parameter replacement, the MLP dispatch) are
gauspcc_amd.anchor_codec's.
"""
import os
import time

import torch

from . import anchor_codec, arm_codec
from .anchor_codec import (Q_FEAT, Q_OFFSETS, Q_SCALING, bit2MB_scale, decode_anchors, decode_mask_stream, encode_anchors, encode_mask_stream,
                           install_decoded, mlp2_parts, n_slices, offset_bounds, offsets_mask, run_mlp2, slice_file_names, ste_multistep,
                           zero_filled)
from .encodings_cuda import _read_files, deferred_writes
from .mlp import mlp2_forward
from .torchac_encodings import decoder_gaussian_slices, encoder_gaussian_slices, host

anchor_round_digits = 16           # CAT-3DGS/utils/encodings.py:12
MAX_BATCH_SIZE = 500               # CAT-3DGS/scene/gaussian_model.py:1178
_CONTEXT_ROWS = 1 << 17            # anchors per pass of the context (432 floats of features each)
# the class of gsac_decode_normal_chain (include/gauspcc.h)
CHAIN_MAX_STAGES, CHAIN_MAX_CH, CHAIN_MAX_DH, CHAIN_DEFAULT_BLOCK = 8, 64, 128, 8
# chain=None takes the kernel below this many slices.  The staged path launches one wave per slice and stage after stage: from about one slice per
# SIMD (1 024 on the MI355X) it fills the device by itself.  Measured (profiles/r07_cat_codec.txt): 200 slices 27.2 -> 14.1 ms and 29.5 -> 17.5 ms
# (attribute part, MLP flags off / on), 2 000 slices 112.5 / 104.5 ms and 112.1 / 111.3 ms with overlapping spreads -- no gain there.
CHAIN_AUTO_MAX_SLICES = 1024


# ---------------------------------------------------------------- the stages and their schedule (no device needed)
def stage_table(model):
    """One dict per stream of a slice, in coding order: feat groups, scaling, offsets.  A row of the context is
    [scales F | means F | mean_scaling 6 | scale_scaling 6 | mean_offsets 3K | scale_offsets 3K | Q_feat_adj, Q_scaling_adj, Q_offsets_adj] (:1227-1228).
    stem: the file is `<stem>_<slice>.b`; dep_ch: the decoded feat channels [0, dep_ch) the stage's MLP reads (0: no MLP); lag: the pipeline step
    offset of gsac_decode_normal_chain; feat_col: first feat channel the stage decodes (-1 for scaling / offsets)."""
    F, K = model.feat_dim, model.n_offsets
    groups = list(model.chcm_slices_list)
    assert len(groups) == model.num_feat_slices and sum(groups) == F
    G = len(groups)
    stages, c0 = [], 0
    for i, ch in enumerate(groups):
        stages.append(dict(name=f"feat{i}", stem=f"feat{i}", attr="feat", ch=ch, dep_ch=c0 if i else 0, lag=i, scale_col=c0, mean_col=F + c0,
                           out_col=c0, feat_col=c0, q_col=2 * F + 12 + 6 * K, mlp=model.mlp_chcm_list[i - 1] if i else None))
        c0 += ch
    on_s, on_o = bool(getattr(model, "chcm_for_scaling", False)), bool(getattr(model, "chcm_for_offsets", False))
    stages.append(dict(name="scaling", stem="scaling", attr="scaling", ch=6, dep_ch=F if on_s else 0, lag=G if on_s else 0, mean_col=2 * F,
                       scale_col=2 * F + 6, out_col=0, feat_col=-1, q_col=2 * F + 12 + 6 * K + 1, mlp=model.mlp_chcm_scaling if on_s else None))
    stages.append(dict(name="offsets", stem="offsets", attr="offsets", ch=3 * K, dep_ch=F if on_o else 0, lag=G if on_o else 0, mean_col=2 * F + 12,
                       scale_col=2 * F + 12 + 3 * K, out_col=0, feat_col=-1, q_col=2 * F + 12 + 6 * K + 2, mlp=model.mlp_chcm_offsets if on_o else None))
    return stages


def chain_steps(n_anchors, block_anchors, lags):
    """steps of the pipeline over one slice: its blocks, and the longest lag to drain"""
    return -(-n_anchors // block_anchors) + max(lags)


def chain_schedule(n_anchors, block_anchors, lags):
    """[step][stage] -> the block the stage decodes in that step, or None while it idles through the barrier (the kernel's loop, restated)"""
    nblocks = -(-n_anchors // block_anchors)
    return [[t - lag if 0 <= t - lag < nblocks else None for lag in lags] for t in range(chain_steps(n_anchors, block_anchors, lags))]


def slice_bounds(N, max_batch=MAX_BATCH_SIZE):
    """anchor_codec.slice_bounds at CAT-3DGS's slice size"""
    return anchor_codec.slice_bounds(N, max_batch)


def chain_eligible(stages):
    """whether gsac_decode_normal_chain takes this chain"""
    if len(stages) > CHAIN_MAX_STAGES:
        return False
    for st in stages:
        if st["ch"] > CHAIN_MAX_CH or st["dep_ch"] > CHAIN_MAX_CH:
            return False
        if st["mlp"] is not None:
            parts = mlp2_parts(st["mlp"])
            if parts is None or parts[4] != "relu" or parts[0].shape[0] > CHAIN_MAX_DH:
                return False
    return True


def _use_chain(chain, stages, N):
    if os.environ.get("GAUSPCC_DEV") == "1" and os.environ.get("GAUSPCC_CAT_CHAIN") in ("0", "1"):      # developer switch, as the kernel switches
        chain = os.environ["GAUSPCC_CAT_CHAIN"] == "1"
    if chain is None:
        return N > 0 and chain_eligible(stages) and n_slices(N, MAX_BATCH_SIZE) < CHAIN_AUTO_MAX_SLICES
    if chain and not chain_eligible(stages):
        raise ValueError("cat_codec: chain=True, but this model's stages are outside gsac_decode_normal_chain's class (at most 8 stages of at most 64 "
                         "channels, Linear - ReLU - Linear context MLPs of at most 128 hidden units)")
    return bool(chain) and N > 0


# ---------------------------------------------------------------- context
def _grid_features(grid, rows, levels):
    """TriPlaneField.forward at itr = -1 without its rate term, on the given planes: texels are read as round(v * 16) / 16"""
    from .cat_triplane import ms_triplane_sample
    if grid.contract:
        return ms_triplane_sample(rows, levels, level=2, quantise=True, contract=(grid.pca_mean, grid.rotation_matrix, grid.variance, grid.aabb, grid.con_aabb))
    return ms_triplane_sample(rows, levels, level=2, quantise=True, aabb=grid.aabb)


def _head(net, feat):
    """net.net(net.feature_out(feat)) (scene/attribute.py:41-58).  At net_depth 0 that is Linear - ReLU - Linear and goes through gshac_mlp2;
    anything else is called as it is."""
    fo, tail = net.feature_out, net.net
    fo_l, tail_l = (list(m) if isinstance(m, torch.nn.Sequential) else [] for m in (fo, tail))
    if len(fo_l) == 1 and isinstance(fo_l[0], torch.nn.Linear) and len(tail_l) == 2 and isinstance(tail_l[0], torch.nn.ReLU) and isinstance(tail_l[1], torch.nn.Linear):
        return mlp2_forward(feat, fo_l[0].weight, fo_l[0].bias, tail_l[1].weight, tail_l[1].bias)
    return tail(fo(feat))


def _context(model, anchor, planes=None):
    """feature_net(anchor, itr=-1)[0] for ALL anchors, in passes of bounded size: (N, 2 F + 12 + 6 K + 3), contiguous -- the stages address its
    columns.  planes: the levels decode_triplane returned (the decoder), or None for the model's own grids (the encoder)."""
    net = model.feature_net.attribute_net
    levels = [list(g) for g in (planes if planes is not None else net.grid.grids)]
    outs = [_head(net, _grid_features(net.grid, anchor[a:a + _CONTEXT_ROWS].contiguous(), levels)) for a in range(0, anchor.shape[0], _CONTEXT_ROWS)]
    if not outs:
        return torch.zeros(0, 2 * model.feat_dim + 12 + 6 * model.n_offsets + 3, device=anchor.device)
    return (torch.cat(outs, dim=0) if len(outs) != 1 else outs[0]).contiguous()


def _step_sizes(model, ctx):
    """the three step sizes of every anchor, (N, 1) each: Q0 * (1.1 + tanh(adj)) (:1233, :1329-1330)"""
    c = 2 * model.feat_dim + 12 + 6 * model.n_offsets
    return {"feat": Q_FEAT * (1.1 + torch.tanh(ctx[:, c:c + 1].contiguous())),
            "scaling": Q_SCALING * (1.1 + torch.tanh(ctx[:, c + 1:c + 2].contiguous())),
            "offsets": Q_OFFSETS * (1.1 + torch.tanh(ctx[:, c + 2:c + 3].contiguous()))}


def _stage_params(st, ctx, feat_decoded):
    """(mean, scale) of a stage, (N, ch) each: the base columns, plus the MLP of the decoded channels [0, dep_ch) (:1265-1267, :1313-1319)"""
    ch = st["ch"]
    mean, scale = ctx[:, st["mean_col"]:st["mean_col"] + ch], ctx[:, st["scale_col"]:st["scale_col"] + ch]
    if st["mlp"] is not None:
        d = run_mlp2(st["mlp"], feat_decoded[:, :st["dep_ch"]].contiguous())
        mean, scale = mean + d[:, :ch], scale + d[:, ch:]
    return mean.contiguous(), torch.clamp(scale, min=1e-9).contiguous()


def _flat_q(q, ch):
    return q.expand(q.shape[0], ch).reshape(-1)


# ---------------------------------------------------------------- encoder
def encode_stages(stages, ctx, Q, x, mask, bounds, pre_path_name, steps):
    """One encoder_gaussian_slices call per stage (the stages are independent once feat is quantised).  x: the quantised attributes {"feat" (N, F),
    "scaling" (N, 6), "offsets" (N, 3K)}; mask (N, 3K) bool: the offsets that are coded.  Returns ({stage: bits per slice}, mins, maxs)."""
    N = ctx.shape[0]
    bits, mins, maxs = {}, {}, {}
    with deferred_writes():      # the stages' slice files go to disk while the next stage is coded; all written when the block ends
        for st in stages:
            ch = st["ch"]
            mean, scale = _stage_params(st, ctx, x["feat"])
            xs = x[st["attr"]][:, st["out_col"]:st["out_col"] + ch].contiguous()
            q = _flat_q(Q[st["attr"]], ch)
            names = slice_file_names(pre_path_name, st["stem"], steps)
            if st["attr"] == "offsets":
                m = mask.reshape(-1)
                res = encoder_gaussian_slices(xs.reshape(-1)[m], mean.reshape(-1)[m], scale.reshape(-1)[m], q[m], offset_bounds(m, N, bounds), names)
            else:
                res = encoder_gaussian_slices(xs.reshape(-1), mean.reshape(-1), scale.reshape(-1), q, [b * ch for b in bounds], names)
            bits[st["name"]], mins[st["name"]], maxs[st["name"]] = res
    return bits, mins, maxs


@torch.no_grad()
def conduct_encoding(self, pre_path_name, weighted_mask, ckpt_path=None):
    t_codec = 0
    torch.cuda.synchronize(); t1 = time.time()
    print('Start encoding ...')
    mask_anchor = self.get_mask_anchor(weighted_mask)
    _anchor = self.get_anchor[mask_anchor]
    _feat = self._anchor_feat[mask_anchor]
    _grid_offsets = self._offset[mask_anchor]
    _scaling = self.get_scaling[mask_anchor]
    _mask = self.get_mask(weighted_mask)[mask_anchor]
    N = _anchor.shape[0]

    # AI-PCC (:1156-1169)
    _anchor, sorted_indices, bits_xyz = encode_anchors(_anchor, self.voxel_size, ckpt_path, pre_path_name)
    _feat = _feat[sorted_indices]
    _grid_offsets = _grid_offsets[sorted_indices]
    _scaling = _scaling[sorted_indices]
    _mask = _mask[sorted_indices]

    MAX_batch_size = MAX_BATCH_SIZE
    steps = n_slices(N, MAX_batch_size)
    n_off = self.n_offsets
    anchor_infos_list = [None] * steps                                   # (:1221-1222)
    masks_b_name = os.path.join(pre_path_name, 'masks.b')
    bounds = slice_bounds(N, MAX_batch_size)
    stages = stage_table(self)

    ctx = _context(self, _anchor)
    Q = _step_sizes(self, ctx)
    # the rate of the quantised planes does not depend on the points (:1226: the reference's value of the last slice)
    feat_rate = self.feature_net(_anchor[:1], itr=-1)[1]
    # the three attributes as they are coded (:1245, :1333, :1345: STE_multistep with the GLOBAL means)
    mask = offsets_mask(_mask).view(N, 3 * n_off)                      # [N, K*3]
    x = {"feat": ste_multistep(_feat, Q["feat"], _feat.mean()),
         "scaling": ste_multistep(_scaling, Q["scaling"], self.get_scaling.mean()),
         "offsets": ste_multistep(_grid_offsets.reshape(-1, 3 * n_off), Q["offsets"], self._offset.mean())}
    x["offsets"][~mask] = 0.0
    torch.cuda.synchronize(); t0 = time.time()
    bits, mins, maxs = encode_stages(stages, ctx, Q, x, mask, bounds, pre_path_name, steps)
    torch.cuda.synchronize(); t_codec += time.time() - t0

    G = self.num_feat_slices
    bit_anchor = bits_xyz
    bit_feat_list = [sum(bits[f"feat{i}"]) for i in range(G)]
    total_bit_feat = sum(bit_feat_list)
    bit2MB_feat_list = [round(b / bit2MB_scale, 4) for b in bit_feat_list]
    bit_scaling = sum(bits["scaling"])
    bit_offsets = sum(bits["offsets"])

    bit_masks, prob_masks = encode_mask_stream(_mask, masks_b_name)      # (:1370-1375)

    show_feat_bits = ' '
    for i in range(G):
        show_feat_bits += f'feat{i} {round(bit_feat_list[i]/bit2MB_scale, 4)}, '

    triplane_coder_list, triplane_byte = arm_codec.encode_triplane(self.feature_net.attribute_net.grid, pre_path_name)

    torch.cuda.synchronize(); t2 = time.time()
    print('encoding time:', t2 - t1)
    print('codec time:', t_codec)
    ftrirate = feat_rate / bit2MB_scale
    mlp_bits = self.get_mlp_size()[0]
    log_info = f"\nEncoded sizes in MB: " \
               f"anchor {round(bit_anchor/bit2MB_scale, 4)}, " \
               f"total_feat {round(total_bit_feat/bit2MB_scale, 4)}, " \
               f"{show_feat_bits}" \
               f"scaling {round(bit_scaling/bit2MB_scale, 4)}, " \
               f"offsets {round(bit_offsets/bit2MB_scale, 4)}, " \
               f"masks {round(bit_masks/bit2MB_scale, 4)}, " \
               f"MLPs {round(mlp_bits/bit2MB_scale, 4)}, " \
               f"Triplane_f {round(triplane_byte/(1024*1024), 4)}," \
               f"Total {round((bit_anchor + total_bit_feat + bit_scaling + bit_offsets + bit_masks + mlp_bits)/bit2MB_scale+ftrirate.item(), 4)}, " \
               f"EncTime {round(t2 - t1, 4)}"
    rate_set = [round(bit_anchor/bit2MB_scale, 4), round(total_bit_feat/bit2MB_scale, 4)] + bit2MB_feat_list + \
               [round(bit_scaling/bit2MB_scale, 4), round(bit_offsets/bit2MB_scale, 4), round(bit_masks/bit2MB_scale, 4), round(mlp_bits/bit2MB_scale, 4), ftrirate.item()]
    return [self._anchor.shape[0], N, MAX_batch_size, anchor_infos_list, [mins[f"feat{i}"] for i in range(G)], [maxs[f"feat{i}"] for i in range(G)],
            mins["scaling"], maxs["scaling"], mins["offsets"], maxs["offsets"], prob_masks, triplane_coder_list], log_info, rate_set


# ---------------------------------------------------------------- decoder
def decode_staged(stages, ctx, Q, keep, bounds, pre_path_name, steps, mins, maxs, N, F, n_off):
    """stage after stage: the expectation for the kernel, and the path of chains it does not take"""
    dev = ctx.device
    outs = {"feat": torch.zeros(N, F, device=dev), "scaling": torch.zeros(N, 6, device=dev), "offsets": torch.zeros(N, 3 * n_off, device=dev)}
    for st in stages:
        ch = st["ch"]
        mean, scale = _stage_params(st, ctx, outs["feat"])
        q = _flat_q(Q[st["attr"]], ch)
        names = slice_file_names(pre_path_name, st["stem"], steps)
        if st["attr"] == "offsets":
            m = keep.reshape(-1)
            vals = decoder_gaussian_slices(mean.reshape(-1)[m], scale.reshape(-1)[m], q[m], offset_bounds(m, N, bounds), names, mins[st["name"]], maxs[st["name"]])
            outs["offsets"].view(-1)[m] = vals
        else:
            vals = decoder_gaussian_slices(mean.reshape(-1), scale.reshape(-1), q, [b * ch for b in bounds], names, mins[st["name"]], maxs[st["name"]])
            outs[st["attr"]][:, st["out_col"]:st["out_col"] + ch] = vals.view(N, ch)
    return outs


def _read_streams(file_names):
    """(bytes, cnt): the files' contents back to back (a copy: the library's blob lives until this thread's next call) and their sizes"""
    import numpy as np
    blob, offs = _read_files(file_names)
    return blob.copy(), np.diff(offs).astype(np.int32)


def decode_chain(stages, ctx, Q, keep, pre_path_name, steps, mins, maxs, N, F, n_off, max_batch=MAX_BATCH_SIZE, block_anchors=0):
    """gsac_decode_normal_chain on the files of conduct_encoding: the three attribute matrices.  keep: (N, K) bool, the offsets a stream holds."""
    from . import _lib, runtime
    dev = ctx.device
    outs = {"feat": torch.zeros(N, F, device=dev), "scaling": torch.zeros(N, 6, device=dev), "offsets": torch.zeros(N, 3 * n_off, device=dev)}
    if N == 0:
        return outs
    recs = (_lib.ChainStage * len(stages))()
    alive = []                                              # what the records point to
    keep_u8 = keep.to(torch.uint8).contiguous()

    for r, st in zip(recs, stages):
        for k in ("ch", "dep_ch", "lag", "mean_col", "scale_col", "feat_col", "out_col"):
            setattr(r, k, st[k])
        out = outs[st["attr"]]
        r.out_pitch, r.out_dev = out.shape[1], out.data_ptr()
        q = Q[st["attr"]].reshape(-1).contiguous()
        r.q_dev = q.data_ptr()
        if st["mlp"] is not None:
            w = [t.detach().contiguous().float() for t in mlp2_parts(st["mlp"])[:4]]
            r.dh = w[0].shape[0]
            r.w1, r.b1, r.w2, r.b2 = (t.data_ptr() for t in w)
            alive.append(w)
        if st["attr"] == "offsets":
            r.keep_dev, r.keep_group = keep_u8.data_ptr(), 3
        blob, cnt = _read_streams(slice_file_names(pre_path_name, st["stem"], steps))
        mn, mx = host(mins[st["name"]]), host(maxs[st["name"]])
        if mn.size != steps or mx.size != steps:
            raise ValueError("cat_codec: one (min, max) per slice and stage")
        r.bytes, r.nbytes, r.cnt = (blob.ctypes.data if blob.size else None), blob.size, cnt.ctypes.data
        r.min_value, r.max_value = mn.ctypes.data, mx.ctypes.data
        alive.append((q, blob, cnt, mn, mx))
    _lib.check(_lib.lib().gsac_decode_normal_chain(runtime.context(dev), recs, len(stages), ctx.data_ptr(), ctx.shape[1], N, max_batch, steps, block_anchors,
                                                   runtime.stream_ptr(dev)))
    del alive
    return outs


@torch.no_grad()
def conduct_decoding(self, pre_path_name, patched_infos, weighted_mask, ckpt_path=None, chain=None):
    torch.cuda.synchronize(); t1 = time.time()
    print('Start decoding ...')
    [N_full, N, MAX_batch_size, anchor_infos_list, min_feat_lists, max_feat_lists, min_scaling_list, max_scaling_list, min_offsets_list, max_offsets_list,
     prob_masks, triplane_coder_list] = patched_infos
    steps = n_slices(N, MAX_batch_size)
    n_off, F = self.n_offsets, self.feat_dim
    dev = self._anchor_feat.device
    masks_b_name = os.path.join(pre_path_name, 'masks.b')

    planes = arm_codec.decode_triplane(self.feature_net.attribute_net.grid, pre_path_name, triplane_coder_list)       # (:1414)

    masks_decoded = decode_mask_stream(N, n_off, prob_masks, masks_b_name, dev)      # (:1417-1422) {0, 1}

    anchor_decoded = decode_anchors(pre_path_name, ckpt_path, self.voxel_size, dev)      # (:1440-1447)
    N = anchor_decoded.shape[0]

    stages = stage_table(self)
    ctx = _context(self, anchor_decoded, planes)
    Q = _step_sizes(self, ctx)
    bounds = slice_bounds(N, MAX_batch_size)
    mins = {f"feat{i}": min_feat_lists[i] for i in range(self.num_feat_slices)}
    maxs = {f"feat{i}": max_feat_lists[i] for i in range(self.num_feat_slices)}
    mins.update(scaling=min_scaling_list, offsets=min_offsets_list)
    maxs.update(scaling=max_scaling_list, offsets=max_offsets_list)
    keep = masks_decoded.view(N, n_off).to(torch.bool)
    if _use_chain(chain, stages, N):
        outs = decode_chain(stages, ctx, Q, keep, pre_path_name, steps, mins, maxs, N, F, n_off, MAX_batch_size)
    else:
        outs = decode_staged(stages, ctx, Q, offsets_mask(masks_decoded).view(N, 3 * n_off), bounds, pre_path_name, steps, mins, maxs, N, F, n_off)
    feat_decoded, scaling_decoded = outs["feat"], outs["scaling"]
    offsets_decoded = outs["offsets"].view(N, n_off, 3)  # [N, K, 3]

    torch.cuda.synchronize(); t2 = time.time()
    print('decoding time:', t2 - t1)

    # fill back N_full (:1581-1592)
    filled = [zero_filled(t) for t in (anchor_decoded, feat_decoded, offsets_decoded, scaling_decoded, masks_decoded)]

    print('Start replacing parameters with decoded ones...')
    install_decoded(self, *filled)      # (:1598-1608)
    print('Parameters are successfully replaced by decoded ones!')
    return f"\nDecTime {round(t2 - t1, 4)}"


# ---------------------------------------------------------------- rate estimate
def _binary_vxl_bits(binary_vxl):
    """get_binary_vxl_size(...)[1] (CAT-3DGS/utils/encodings.py:17-34)"""
    ttl_num = binary_vxl.numel()
    pos_num = torch.sum(binary_vxl)
    neg_num = ttl_num - pos_num
    Pg = torch.clamp(pos_num / ttl_num, min=1e-6, max=1 - 1e-6)
    return pos_num * (-torch.log2(Pg)) + neg_num * (-torch.log2(1 - Pg)) + 32


@torch.no_grad()
def estimate_final_bits(self, weighted_mask):
    """(:1056-1137) the same chain with entropy_models.Entropy_gaussian in place of the coder; STE_multistep WITHOUT a mean argument (input.mean()),
    as the reference calls it here."""
    from . import entropy_models
    mask_anchor = self.get_mask_anchor(weighted_mask)
    _anchor = self.get_anchor[mask_anchor]
    _feat = self._anchor_feat[mask_anchor]
    _grid_offsets = self._offset[mask_anchor]
    _scaling = self.get_scaling[mask_anchor]
    _mask = self.get_mask(weighted_mask)[mask_anchor]
    n_off = self.n_offsets
    ctx = _context(self, _anchor)
    feat_rate = self.feature_net(_anchor[:1], itr=-1)[1]
    Q = _step_sizes(self, ctx)
    entropy = getattr(self, "entropy_gaussian", None) or entropy_models.Entropy_gaussian(Q=1)
    feat_q = ste_multistep(_feat, Q["feat"], _feat.mean())
    xs = {"feat": feat_q, "scaling": ste_multistep(_scaling, Q["scaling"], _scaling.mean()),
          "offsets": ste_multistep(_grid_offsets, Q["offsets"].unsqueeze(1), _grid_offsets.mean()).view(-1, 3 * n_off)}
    bit = {}
    for st in stage_table(self):
        ch = st["ch"]
        mean, scale = _stage_params(st, ctx, feat_q)       # (the reference leaves the clamp to Entropy_gaussian, which applies the same one)
        b = entropy.forward(xs[st["attr"]][:, st["out_col"]:st["out_col"] + ch].contiguous(), mean, scale, Q[st["attr"]])
        if st["attr"] == "offsets":
            b = b * _mask.repeat(1, 1, 3).view(-1, 3 * n_off)
        bit[st["name"]] = torch.sum(b).item()
    bit_feat_list = [bit[f"feat{i}"] for i in range(self.num_feat_slices)]
    bit_scaling, bit_offsets = bit["scaling"], bit["offsets"]
    bit_anchor = _anchor.shape[0] * 3 * anchor_round_digits
    bit_masks = _binary_vxl_bits(_mask).item()
    ftrirate = feat_rate / bit2MB_scale
    mlp_bits = self.get_mlp_size()[0]
    log_info = f"\nEstimated sizes in MB: " \
               f"anchor {round(bit_anchor/bit2MB_scale, 4)}, " \
               f"total feat {round(sum(bit_feat_list)/bit2MB_scale, 4)}, " \
               f"scaling {round(bit_scaling/bit2MB_scale, 4)}, " \
               f"offsets {round(bit_offsets/bit2MB_scale, 4)}, " \
               f"masks {round(bit_masks/bit2MB_scale, 4)}, " \
               f"MLPs {round(mlp_bits/bit2MB_scale, 4)}, " \
               f"Triplane_f {round(ftrirate.item(),4)}," \
               f"Total {round((bit_anchor + sum(bit_feat_list) + bit_scaling + bit_offsets + bit_masks+ mlp_bits)/bit2MB_scale+ftrirate.item(), 4)}"
    return log_info
