"""GaussianModel.conduct_encoding / conduct_decoding of HAC (src/gs_compress/HAC/scene/gaussian_model.py:1090-1222,
1225-1366; the same loop in HAC-plus / TC-GS / CAT-3DGS) on the gfx950 kernels -- SURVEY.md §8(f) row 1.

Both functions take the model as their first argument and touch it only through the attributes the reference methods
touch, so they bind as methods:

    from gauspcc_amd import hac_codec
    GaussianModel.conduct_encoding = hac_codec.conduct_encoding
    GaussianModel.conduct_decoding = hac_codec.conduct_decoding

Same files under `pre_path_name` (xyz_pcc.bin, feat_{s}_0.b, scaling_{s}_0.b, offsets_{s}_0.b, hash.b, masks.b), same
`[N_full, N, MAX_batch_size]` patched-info contract, same log strings.  What runs underneath:

    anchors     calculate_morton_order + compress / decompress_point_cloud     gauspcc_amd.pcc_utils (gpcc_encode / gpcc_decode)
    context     calc_interp_feat (hash grids) -> mlp_grid                      gsge_forward, gshac_mlp2 (specified fp32 order:
                                                                                encoder and decoder see identical parameters)
    attributes  encoder_gaussian_chunk / decoder_gaussian_chunk                gsac_encode_gaussian / gsac_decode_gaussian
                                                                                (CDF entries evaluated inside the coder)
    bits        encoder / decoder (one global Bernoulli p)                     gsac_encode / gsac_decode

The context MLP runs ONCE over all anchors instead of once per 3000-anchor slice (rows are independent, so the slices of
the result are the per-slice results), and all slices of an attribute are coded in ONE device call
(gsac_encode_gaussian_slices / gsac_decode_gaussian_slices): the slices only decide which elements share a `.b` file and
its min / max.  Per million anchors the reference issues ~1000 coder calls, each a serial chain of 10000-symbol chunks.

The steps this loop shares with HAC++, TC-GS and CAT-3DGS (slice geometry, xyz_pcc.bin, parameter replacement, the MLP
dispatch) are gauspcc_amd.anchor_codec's; `mlp2` stays here as the name tests and tools call.
"""
import os
import time

import torch

from .anchor_codec import (Q_FEAT, Q_OFFSETS, Q_SCALING, bit2MB_scale, decode_anchors, encode_anchors, install_decoded, n_slices, offset_bounds,
                           offsets_mask, run_mlp2, slice_bounds, slice_file_names, ste_multistep)
from .encodings_cuda import decoder, decoder_gaussian_slices_multi, deferred_writes, encoder, encoder_gaussian_slices
from .mlp import mlp2_forward

MAX_BATCH_SIZE = 3_000             # HAC/scene/gaussian_model.py:1123


def mlp2(x, w1, b1, w2, b2):
    """Linear - ReLU - Linear on the device, specified fp32 order (gshac_mlp2_act).  x (n, din) -> (n, dout)."""
    return mlp2_forward(x, w1, b1, w2, b2, "relu", 0.0)


def grid_mlp(model, feat_context):
    """model.get_grid_mlp(feat_context): the nn.Sequential(Linear, ReLU, Linear) HAC builds (:258-262) on the device kernel (anchor_codec.run_mlp2)."""
    return run_mlp2(model.get_grid_mlp, feat_context)


def _context(model, anchor):
    """(:1152-1172 / :1281-1302) for ALL anchors at once: the 9 split outputs of mlp_grid, flattened per attribute."""
    feat_dim, n_off = model.feat_dim, model.n_offsets
    out = grid_mlp(model, model.calc_interp_feat(anchor))
    mean, scale, mean_scaling, scale_scaling, mean_offsets, scale_offsets, qa_f, qa_s, qa_o = torch.split(
        out, split_size_or_sections=[feat_dim, feat_dim, 6, 6, 3 * n_off, 3 * n_off, 1, 1, 1], dim=-1)
    ctx = {
        "mean": mean.contiguous(), "scale": torch.clamp(scale.contiguous(), min=1e-9),
        "mean_scaling": mean_scaling.contiguous(), "scale_scaling": torch.clamp(scale_scaling.contiguous(), min=1e-9),
        "mean_offsets": mean_offsets.contiguous(), "scale_offsets": torch.clamp(scale_offsets.contiguous(), min=1e-9),
        # one step size per anchor, repeated over the attribute's channels (:1158-1172)
        "Q_feat": (Q_FEAT * (1 + torch.tanh(qa_f.contiguous()))).repeat(1, feat_dim),
        "Q_scaling": (Q_SCALING * (1 + torch.tanh(qa_s.contiguous()))).repeat(1, 6),
        "Q_offsets": (Q_OFFSETS * (1 + torch.tanh(qa_o.contiguous()))).repeat(1, 3 * n_off),
    }
    return ctx


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

    # AI-PCC (:1106-1117)
    _anchor, sorted_indices, bits_xyz = encode_anchors(_anchor, self.voxel_size, ckpt_path, pre_path_name)
    _feat = _feat[sorted_indices]
    _grid_offsets = _grid_offsets[sorted_indices]
    _scaling = _scaling[sorted_indices]
    _mask = _mask[sorted_indices]

    N = _anchor.shape[0]
    steps = n_slices(N, MAX_BATCH_SIZE)
    n_off = self.n_offsets
    c = _context(self, _anchor)
    feat_mean, scaling_mean, offsets_mean = _feat.mean(), _scaling.mean(), _grid_offsets.mean()
    hash_b_name = os.path.join(pre_path_name, 'hash.b')
    masks_b_name = os.path.join(pre_path_name, 'masks.b')
    names = lambda stem: slice_file_names(pre_path_name, stem, steps)
    bounds = slice_bounds(N, MAX_BATCH_SIZE)

    torch.cuda.synchronize(); t0 = time.time()
    with deferred_writes():      # the 3 x 334 slice files are written while the next attribute is coded; all on disk when the block ends
        Q = c["Q_feat"].reshape(-1)
        feat = ste_multistep(_feat.reshape(-1), Q, feat_mean)
        bit_feat_list = encoder_gaussian_slices(feat, c["mean"].reshape(-1), c["scale"].reshape(-1), Q, [b * self.feat_dim for b in bounds], names('feat'))

        Q = c["Q_scaling"].reshape(-1)
        scaling = ste_multistep(_scaling.reshape(-1), Q, scaling_mean)
        bit_scaling_list = encoder_gaussian_slices(scaling, c["mean_scaling"].reshape(-1), c["scale_scaling"].reshape(-1), Q, [b * 6 for b in bounds], names('scaling'))

        mask = offsets_mask(_mask)        # [N*K*3]
        Q = c["Q_offsets"].reshape(-1)
        offsets = ste_multistep(_grid_offsets.reshape(-1, 3 * n_off).reshape(-1), Q, offsets_mean)
        bit_offsets_list = encoder_gaussian_slices(offsets[mask], c["mean_offsets"].reshape(-1)[mask], c["scale_offsets"].reshape(-1)[mask], Q[mask],
                                                   offset_bounds(mask, N, bounds), names('offsets'))
    torch.cuda.synchronize(); t_codec += time.time() - t0

    bit_anchor = bits_xyz
    bit_feat, bit_scaling, bit_offsets = sum(bit_feat_list), sum(bit_scaling_list), sum(bit_offsets_list)
    hash_embeddings = self.get_encoding_params()  # {-1, 1}
    if self.ste_binary:
        bit_hash = encoder(((hash_embeddings.view(-1) + 1) / 2), file_name=hash_b_name)
    else:
        bit_hash = hash_embeddings.numel() * 32
    bit_masks = encoder(_mask, file_name=masks_b_name)

    torch.cuda.synchronize(); t2 = time.time()
    print('encoding time:', t2 - t1)
    print('codec time:', t_codec)
    mlp_bits = self.get_mlp_size()[0] if hasattr(self, "get_mlp_size") else 0
    log_info = f"\nEncoded sizes in MB: " \
               f"anchor {round(bit_anchor/bit2MB_scale, 4)}, " \
               f"feat {round(bit_feat/bit2MB_scale, 4)}, " \
               f"scaling {round(bit_scaling/bit2MB_scale, 4)}, " \
               f"offsets {round(bit_offsets/bit2MB_scale, 4)}, " \
               f"hash {round(bit_hash/bit2MB_scale, 4)}, " \
               f"masks {round(bit_masks/bit2MB_scale, 4)}, " \
               f"MLPs {round(mlp_bits/bit2MB_scale, 4)}, " \
               f"Total {round((bit_anchor + bit_feat + bit_scaling + bit_offsets + bit_hash + bit_masks + mlp_bits)/bit2MB_scale, 4)}, " \
               f"EncTime {round(t2 - t1, 4)}"
    return [self._anchor.shape[0], N, MAX_BATCH_SIZE], log_info


@torch.no_grad()
def conduct_decoding(self, pre_path_name, patched_infos, ckpt_path=None):
    torch.cuda.synchronize(); t1 = time.time()
    print('Start decoding ...')
    [N_full, N, max_batch] = patched_infos
    steps = n_slices(N, max_batch)
    n_off = self.n_offsets
    dev = self._anchor_feat.device
    hash_b_name = os.path.join(pre_path_name, 'hash.b')
    masks_b_name = os.path.join(pre_path_name, 'masks.b')

    masks_decoded = decoder(N * n_off, masks_b_name, device=dev).to(torch.float32).view(-1, n_off, 1)   # {0, 1}

    if self.ste_binary:
        N_hash = torch.zeros_like(self.get_encoding_params()).numel()
        hash_embeddings = decoder(N_hash, hash_b_name, device=dev)  # {0, 1}
        hash_embeddings = (hash_embeddings * 2 - 1).to(torch.float32).view(-1, self.n_features_per_level)
        _install_hash(self, hash_embeddings)      # the context below must run on the decoded tables (bit-identical for {-1, 1})

    anchor_decoded = decode_anchors(pre_path_name, ckpt_path, self.voxel_size, dev)      # (:1250-1256)
    N = anchor_decoded.shape[0]

    c = _context(self, anchor_decoded)
    names = lambda stem: slice_file_names(pre_path_name, stem, steps)
    bounds = slice_bounds(N, max_batch)
    mask = offsets_mask(masks_decoded)
    mo = c["mean_offsets"].reshape(-1)
    # the three attributes in ONE device call: their chunks side by side (encodings_cuda.decoder_gaussian_slices_multi); the reference decodes
    # slice after slice, attribute after attribute (:1304-1331)
    feat_decoded, scaling_decoded, offs = decoder_gaussian_slices_multi([
        (c["mean"].reshape(-1), c["scale"].reshape(-1), c["Q_feat"].reshape(-1), [b * self.feat_dim for b in bounds], names('feat')),
        (c["mean_scaling"].reshape(-1), c["scale_scaling"].reshape(-1), c["Q_scaling"].reshape(-1), [b * 6 for b in bounds], names('scaling')),
        (mo[mask], c["scale_offsets"].reshape(-1)[mask], c["Q_offsets"].reshape(-1)[mask], offset_bounds(mask, N, bounds), names('offsets'))])
    feat_decoded = feat_decoded.view(N, self.feat_dim)
    scaling_decoded = scaling_decoded.view(N, 6)
    offsets_decoded = torch.zeros_like(mo)
    offsets_decoded[mask] = offs
    offsets_decoded = offsets_decoded.view(N, n_off, 3)

    torch.cuda.synchronize(); t2 = time.time()
    print('decoding time:', t2 - t1)

    print('Start replacing parameters with decoded ones...')
    install_decoded(self, anchor_decoded, feat_decoded, offsets_decoded, scaling_decoded, masks_decoded)      # (:1342-1348)
    print('Parameters are successfully replaced by decoded ones!')
    return f"\nDecTime {round(t2 - t1, 4)}"


def _install_hash(self, hash_embeddings):
    """(:1341-1352) put the decoded hash tables back into the encoders."""
    nn = torch.nn
    enc = self.encoding_xyz
    if getattr(self, "use_2D", False):
        len_3D = enc.encoding_xyz.params.shape[0]
        len_2D = enc.encoding_xy.params.shape[0]
        enc.encoding_xyz.params = nn.Parameter(hash_embeddings[0:len_3D])
        enc.encoding_xy.params = nn.Parameter(hash_embeddings[len_3D:len_3D + len_2D])
        enc.encoding_xz.params = nn.Parameter(hash_embeddings[len_3D + len_2D:len_3D + len_2D * 2])
        enc.encoding_yz.params = nn.Parameter(hash_embeddings[len_3D + len_2D * 2:len_3D + len_2D * 3])
    else:
        enc.params = nn.Parameter(hash_embeddings)
