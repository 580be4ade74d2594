"""GaussianModel.conduct_encoding / conduct_decoding / estimate_final_bits of TC-GS (src/gs_compress/TC-GS/scene/gaussian_model.py:1135-1311,
1313-1465, 1072-1133) on the gfx950 kernels.  The functions take the model as their first argument and touch it only through the attributes
the reference methods touch, so they bind as methods:

    from gauspcc_amd import tcgs_codec
    GaussianModel.conduct_encoding = tcgs_codec.conduct_encoding
    GaussianModel.conduct_decoding = tcgs_codec.conduct_decoding
    GaussianModel.estimate_final_bits = tcgs_codec.estimate_final_bits

Same files under `pre_path_name` (xyz_pcc.bin, feat_{s}.b, scaling_{s}.b, offsets_{s}.b, masks.b, and hash.b when `ste_binary`), each attribute
file ONE raw torchac stream per 1 000-anchor slice; the same twelve-element `patched_infos` (the per-slice min / max lists of 0-d tensors,
`prob_hash`, `prob_masks`), the same log strings, the same parameter replacement at the end of decoding.  What runs underneath:

    anchors     calculate_morton_order + compress / decompress_point_cloud      gauspcc_amd.pcc_utils (gpcc_encode / gpcc_decode)
    context     self.triplane(anchor.unsqueeze(1).repeat(1, K, 1), ...),        ONCE over all anchors, in the sampler's repeat form
                cat with the anchor, self.get_tri_mlp                           (gsge_plane_forward), then gshac_mlp2 (specified fp32 order:
                                                                                encoder and decoder see identical parameters)
    attributes  encoder_gaussian / decoder_gaussian per slice and attribute     torchac_encodings.encoder_gaussian_slices / decoder_gaussian_slices:
                                                                                every stream of an attribute in one device call, no CDF table
    bits        encoder / decoder (masks.b, hash.b: one stream each by format)  torchac_encodings.encoder / decoder

The reference's loop samples the planes, runs the MLP and builds, integerises and ships an n x (max - min + 2) table per slice and attribute
(3 000 tables and 3 000 serial host chains per million anchors); rows are independent, so the slices of the one context pass are the per-slice
results.  The attribute files are written and read by this pair (torchac_encodings.encoder_gaussian_slices has the reason).
`ckpt_path`: the GausPcgc checkpoint (the reference looks beside its own sources; here the argument or $GAUSPCGC_CKPT).
The steps shared with HAC, HAC++ and CAT-3DGS (slice geometry, xyz_pcc.bin, masks.b, fill back and parameter replacement, the MLP dispatch) are
gauspcc_amd.anchor_codec's.
"""
import os
import time

import torch

from .anchor_codec import (Q_FEAT, Q_OFFSETS, Q_SCALING, bit2MB_scale, decode_anchors, decode_mask_stream, encode_anchors, encode_mask_stream,
                           install_decoded, n_slices, offset_bounds, offsets_mask, run_mlp2, slice_bounds, slice_file_names, ste_multistep, zero_filled)
from .encodings_cuda import deferred_writes
from .torchac_encodings import decoder, decoder_gaussian_slices, encoder, encoder_gaussian_slices

K = 4                              # TC-GS/scene/gaussian_model.py:32
MAX_BATCH_SIZE = 1_000             # :1173
anchor_round_digits = 16           # TC-GS/utils/encodings.py:11
_CONTEXT_ROWS = 1 << 17            # anchors per pass of the context (603 floats of features each: 0.3 GB at a time, whatever the scene's size)


def tri_mlp(model, feat_context):
    """model.get_tri_mlp(feat_context): the nn.Sequential(Linear, ReLU, Linear) TC-GS builds on the device kernel (anchor_codec.run_mlp2)."""
    return run_mlp2(model.get_tri_mlp, feat_context)


def _context(model, anchor):
    """(:1215-1236 / :1379-1403) for ALL anchors: the 9 split outputs of mlp_triplane, flattened per attribute."""
    feat_dim, n_off = model.feat_dim, model.n_offsets
    outs = []
    for a in range(0, anchor.shape[0], _CONTEXT_ROWS):
        rows = anchor[a:a + _CONTEXT_ROWS].contiguous()
        feat_context = model.triplane(rows, model.x_bound_max, model.x_bound_min, repeat=K)      # == rows.unsqueeze(1).repeat(1, K, 1), sampled once
        outs.append(tri_mlp(model, torch.cat([feat_context, rows], dim=1)))
    out = torch.cat(outs, dim=0) if len(outs) != 1 else outs[0]
    mean, scale, mean_scaling, scale_scaling, mean_offsets, scale_offsets, qa_f, qa_s, qa_o = torch.split(
        out, split_size_or_sections=[feat_dim, feat_dim, 6, 6, 3 * n_off, 3 * n_off, 1, 1, 1], dim=-1)
    flat = lambda t: t.contiguous().view(-1)
    return {
        "mean": flat(mean), "scale": torch.clamp(flat(scale), min=1e-9),
        "mean_scaling": flat(mean_scaling), "scale_scaling": torch.clamp(flat(scale_scaling), min=1e-9),
        "mean_offsets": flat(mean_offsets), "scale_offsets": torch.clamp(flat(scale_offsets), min=1e-9),
        # one step size per anchor, repeated over the attribute's channels (:1225-1236)
        "Q_feat": Q_FEAT * (1 + torch.tanh(qa_f.contiguous().repeat(1, feat_dim).view(-1))),
        "Q_scaling": Q_SCALING * (1 + torch.tanh(qa_s.contiguous().repeat(1, 6).view(-1))),
        "Q_offsets": Q_OFFSETS * (1 + torch.tanh(qa_o.contiguous().repeat(1, 3 * n_off).view(-1))),
    }


@torch.no_grad()
def conduct_encoding(self, pre_path_name, ckpt_path=None):
    t_codec = 0
    torch.cuda.synchronize(); t1 = time.time()
    print('Start encoding ...')
    mask_anchor = self.get_mask_anchor
    _anchor = self.get_anchor[mask_anchor]
    _feat = self._anchor_feat[mask_anchor]
    _grid_offsets = self._offset[mask_anchor]
    _scaling = self.get_scaling[mask_anchor]
    _mask = self.get_mask[mask_anchor]
    N = _anchor.shape[0]

    # AI-PCC (:1155-1169)
    _anchor, sorted_indices, bits_xyz = encode_anchors(_anchor, self.voxel_size, ckpt_path, pre_path_name)
    _feat = _feat[sorted_indices]
    _grid_offsets = _grid_offsets[sorted_indices]
    _scaling = _scaling[sorted_indices]
    _mask = _mask[sorted_indices]

    MAX_batch_size = MAX_BATCH_SIZE
    steps = n_slices(N, MAX_batch_size)
    n_off = self.n_offsets
    anchor_infos_list = [None] * steps                                   # (:1211-1212)
    hash_b_name = os.path.join(pre_path_name, 'hash.b')
    masks_b_name = os.path.join(pre_path_name, 'masks.b')
    bounds = slice_bounds(N, MAX_batch_size)

    c = _context(self, _anchor)
    torch.cuda.synchronize(); t0 = time.time()
    with deferred_writes():      # the 3 x steps slice files go to disk while the next attribute is coded; all written when the block ends
        Q = c["Q_feat"]
        feat = ste_multistep(_feat.reshape(-1), Q, _feat.mean())
        bit_feat_list, min_feat_list, max_feat_list = encoder_gaussian_slices(
            feat, c["mean"], c["scale"], Q, [b * self.feat_dim for b in bounds], slice_file_names(pre_path_name, 'feat', steps))

        Q = c["Q_scaling"]
        scaling = ste_multistep(_scaling.reshape(-1), Q, _scaling.mean())
        bit_scaling_list, min_scaling_list, max_scaling_list = encoder_gaussian_slices(
            scaling, c["mean_scaling"], c["scale_scaling"], Q, [b * 6 for b in bounds], slice_file_names(pre_path_name, 'scaling', steps))

        mask = offsets_mask(_mask)   # [N*K*3]
        Q = c["Q_offsets"]
        offsets = ste_multistep(_grid_offsets.reshape(-1, 3 * n_off).reshape(-1), Q, _grid_offsets.mean())
        offsets[~mask] = 0.0
        bit_offsets_list, min_offsets_list, max_offsets_list = encoder_gaussian_slices(
            offsets[mask], c["mean_offsets"][mask], c["scale_offsets"][mask], Q[mask], offset_bounds(mask, N, bounds),
            slice_file_names(pre_path_name, 'offsets', steps))
    torch.cuda.synchronize(); t_codec += time.time() - t0

    bit_anchor = bits_xyz
    bit_feat = sum(bit_feat_list)
    bit_scaling = sum(bit_scaling_list)
    bit_offsets = sum(bit_offsets_list)

    hash_embeddings = self.get_encoding_params()  # {-1, 1}
    if self.ste_binary:
        p = torch.zeros_like(hash_embeddings).to(torch.float32)
        prob_hash = (((hash_embeddings + 1) / 2).sum() / hash_embeddings.numel()).item()
        p[...] = prob_hash
        bit_hash = encoder(hash_embeddings.view(-1), p.view(-1), file_name=hash_b_name)
    else:
        prob_hash = 0
        bit_hash = hash_embeddings.numel() * 32

    bit_masks, prob_masks = encode_mask_stream(_mask, masks_b_name)      # {0, 1}; the slices' indices concatenated are 0 .. N - 1 (:1289-1296)

    torch.cuda.synchronize(); t2 = time.time()
    print('encoding time:', t2 - t1)
    print('codec time:', t_codec)
    mlp_bits = self.get_mlp_size()[0] if hasattr(self, "get_mlp_size") else 0
    log_info = f"\nEncoded sizes in MB: " \
               f"anchor {round(bit_anchor/bit2MB_scale, 4)}, " \
               f"feat {round(bit_feat/bit2MB_scale, 4)}, " \
               f"scaling {round(bit_scaling/bit2MB_scale, 4)}, " \
               f"offsets {round(bit_offsets/bit2MB_scale, 4)}, " \
               f"triplane {round(bit_hash/bit2MB_scale, 4)}, " \
               f"masks {round(bit_masks/bit2MB_scale, 4)}, " \
               f"MLPs {round(mlp_bits/bit2MB_scale, 4)}, " \
               f"Total {round((bit_anchor + bit_feat + bit_scaling + bit_offsets + bit_hash + bit_masks + mlp_bits)/bit2MB_scale, 4)}, " \
               f"EncTime {round(t2 - t1, 4)}"
    return [self._anchor.shape[0], N, MAX_batch_size, anchor_infos_list, min_feat_list, max_feat_list, min_scaling_list, max_scaling_list,
            min_offsets_list, max_offsets_list, prob_hash, prob_masks], log_info


@torch.no_grad()
def conduct_decoding(self, pre_path_name, patched_infos, ckpt_path=None):
    torch.cuda.synchronize(); t1 = time.time()
    print('Start decoding ...')
    [N_full, N, MAX_batch_size, anchor_infos_list, min_feat_list, max_feat_list, min_scaling_list, max_scaling_list, min_offsets_list, max_offsets_list,
     prob_hash, prob_masks] = patched_infos
    steps = n_slices(N, MAX_batch_size)
    n_off = self.n_offsets
    dev = self._anchor_feat.device
    hash_b_name = os.path.join(pre_path_name, 'hash.b')
    masks_b_name = os.path.join(pre_path_name, 'masks.b')

    masks_decoded = decode_mask_stream(N, n_off, prob_masks, masks_b_name, dev)      # (:1326-1331) {0, 1}

    if self.ste_binary:
        p = torch.zeros_like(self.get_encoding_params()).to(torch.float32)
        p[...] = prob_hash
        hash_embeddings = decoder(p.view(-1), hash_b_name)  # {-1, 1}
        hash_embeddings = hash_embeddings.view(-1, self.feat_dim, self.resolution, self.resolution)

    anchor_decoded = decode_anchors(pre_path_name, ckpt_path, self.voxel_size, dev)      # (:1347-1354)
    N = anchor_decoded.shape[0]

    c = _context(self, anchor_decoded)
    bounds = slice_bounds(N, MAX_batch_size)
    feat_decoded = decoder_gaussian_slices(c["mean"], c["scale"], c["Q_feat"], [b * self.feat_dim for b in bounds], slice_file_names(pre_path_name, 'feat', steps),
                                           min_feat_list, max_feat_list).view(N, self.feat_dim)
    scaling_decoded = decoder_gaussian_slices(c["mean_scaling"], c["scale_scaling"], c["Q_scaling"], [b * 6 for b in bounds],
                                              slice_file_names(pre_path_name, 'scaling', steps), min_scaling_list, max_scaling_list).view(N, 6)
    mask = offsets_mask(masks_decoded)
    mo = c["mean_offsets"]
    offs = decoder_gaussian_slices(mo[mask], c["scale_offsets"][mask], c["Q_offsets"][mask], offset_bounds(mask, N, bounds),
                                   slice_file_names(pre_path_name, 'offsets', steps), min_offsets_list, max_offsets_list)
    offsets_decoded = torch.zeros_like(mo)
    offsets_decoded[mask] = offs
    offsets_decoded = offsets_decoded.view(N, -1).view(N, n_off, 3)  # [N, K, 3]

    torch.cuda.synchronize(); t2 = time.time()
    print('decoding time:', t2 - t1)

    # fill back N_full (:1429-1440)
    filled = [zero_filled(t) for t in (anchor_decoded, feat_decoded, offsets_decoded, scaling_decoded, masks_decoded)]

    print('Start replacing parameters with decoded ones...')
    install_decoded(self, *filled)      # (:1445-1455)
    if self.ste_binary:
        self.triplane.planes = torch.nn.Parameter(hash_embeddings)
    print('Parameters are successfully replaced by decoded ones!')
    return f"\nDecTime {round(t2 - t1, 4)}"


# ---------------------------------------------------------------- rate estimate
def _binary_vxl_bits(binary_vxl):
    """get_binary_vxl_size(...)[1] (TC-GS/utils/encodings.py:16-34)"""
    ttl_num = binary_vxl.numel()
    pos_num = torch.sum(binary_vxl)
    neg_num = ttl_num - pos_num
    Pg = torch.clamp(pos_num / ttl_num, min=1e-6, max=1 - 1e-6)
    return pos_num * (-torch.log2(Pg)) + neg_num * (-torch.log2(1 - Pg)) + 32


def update_knn(self):
    """(:1060-1069) on the device: the K nearest kept anchors of every kept anchor (gauspcc_amd.knn.kneighbors in place of sklearn on the
    host).  As in the reference the indices count the KEPT anchors and are then looked up in the full `self._anchor`."""
    from .knn import kneighbors
    _anchor = self.get_anchor[self.get_mask_anchor]
    self.knn_indices = kneighbors(_anchor.detach(), K).to(torch.long)
    self.knnanchor = self._anchor[self.knn_indices].detach()


@torch.no_grad()
def estimate_final_bits(self):
    """(:1072-1133) the rate estimate on the kept anchors: update_knn, the context rows of `knnanchor` in the (N, K, 3) form, the three
    STE_multistep calls WITHOUT a mean argument (input.mean()) in one launch (quantise_steps; Q_offsets is the codec's 0.2 here, :1077),
    entropy_models.Entropy_gaussian in place of the coder, the reference's `print` and log string.
    Side effect, as in the reference (:1094): `self.triplane.autoencoder.encoder` is None afterwards -- the encoder half of the plane
    autoencoder is not part of the shipped model, and `get_mlp_size` counts what is left."""
    from . import entropy_models
    from .neural_gaussians import quantise_steps
    from .tcgs_renderer import context_input
    mask_anchor = self.get_mask_anchor
    _anchor = self.get_anchor[mask_anchor]
    update_knn(self)
    knnanchor = self.knnanchor
    _feat = self._anchor_feat[mask_anchor]
    _grid_offsets = self._offset[mask_anchor]
    _scaling = self.get_scaling[mask_anchor]
    _mask = self.get_mask[mask_anchor]
    hash_embeddings = self.get_encoding_params()
    feat_dim, n_off = self.feat_dim, self.n_offsets
    outs = []
    for a in range(0, _anchor.shape[0], _CONTEXT_ROWS):
        rows = context_input(self, _anchor[a:a + _CONTEXT_ROWS].contiguous(), knnanchor[a:a + _CONTEXT_ROWS].contiguous(), False, 0)[0]
        outs.append(tri_mlp(self, rows))
    self.triplane.autoencoder.encoder = None
    ctx = torch.cat(outs, dim=0) if len(outs) != 1 else outs[0]
    mean, scale, mean_scaling, scale_scaling, mean_offsets, scale_offsets, _, _, _ = torch.split(
        ctx, split_size_or_sections=[feat_dim, feat_dim, 6, 6, 3 * n_off, 3 * n_off, 1, 1, 1], dim=-1)
    _feat, grid_scaling, offsets, Q = quantise_steps([_feat, _scaling, _grid_offsets], (Q_FEAT, Q_SCALING, Q_OFFSETS), ctx[:, -3:])
    offsets = offsets.view(-1, 3 * n_off)
    mask_tmp = _mask.repeat(1, 1, 3).view(-1, 3 * n_off)
    entropy = getattr(self, "entropy_gaussian", None) or entropy_models.Entropy_gaussian(Q=1)
    bit_feat = entropy.forward(_feat, mean, scale, Q[:, 0:1])
    bit_scaling = entropy.forward(grid_scaling, mean_scaling, scale_scaling, Q[:, 1:2])
    bit_offsets = entropy.forward(offsets, mean_offsets, scale_offsets, Q[:, 2:3])
    bit_offsets = bit_offsets * mask_tmp

    bit_anchor = _anchor.shape[0] * 3 * anchor_round_digits
    bit_feat = torch.sum(bit_feat).item()
    bit_scaling = torch.sum(bit_scaling).item()
    bit_offsets = torch.sum(bit_offsets).item()
    if self.ste_binary:
        bit_hash = _binary_vxl_bits((hash_embeddings + 1) / 2).item()
    else:
        bit_hash = hash_embeddings.numel() * 32
    bit_masks = _binary_vxl_bits(_mask).item()

    print(bit_anchor, bit_feat, bit_scaling, bit_offsets, bit_hash, bit_masks)
    mlp_bits = self.get_mlp_size()[0] if hasattr(self, "get_mlp_size") else 0
    log_info = f"\nEstimated sizes in MB: " \
               f"anchor {round(bit_anchor/bit2MB_scale, 4)}, " \
               f"feat {round(bit_feat/bit2MB_scale, 4)}, " \
               f"scaling {round(bit_scaling/bit2MB_scale, 4)}, " \
               f"offsets {round(bit_offsets/bit2MB_scale, 4)}, " \
               f"triplane {round(bit_hash/bit2MB_scale, 4)}, " \
               f"masks {round(bit_masks/bit2MB_scale, 4)}, " \
               f"MLPs {round(mlp_bits/bit2MB_scale, 4)}, " \
               f"Total {round((bit_anchor + bit_feat + bit_scaling + bit_offsets + bit_hash + bit_masks + mlp_bits)/bit2MB_scale, 4)}"
    return log_info
