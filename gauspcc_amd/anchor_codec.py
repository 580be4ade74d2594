"""What the four conduct_encoding / conduct_decoding drop-ins (hac_codec, hac_plus_codec, tcgs_codec, cat_codec) have in common: all four
references descend from Scaffold-GS's loop over anchors, and these are the host steps that loop repeats in each of them.  Plain functions; every
conduct_* stays a top-to-bottom restatement of its own reference method and calls these where the references agree.

    constants       default_ckpt_path, ste_multistep, bit2MB_scale, Q_FEAT / Q_SCALING / Q_OFFSETS
    slices          n_slices, slice_bounds, slice_file_names, offset_bounds, offsets_mask
    anchors         encode_anchors / decode_anchors (xyz_pcc.bin)
    masks           encode_mask_stream / decode_mask_stream (masks.b, torchac flavour: TC-GS and CAT-3DGS)
    parameters      zero_filled, install_decoded
    context MLPs    mlp2_parts, run_mlp2 (Sequential(Linear, ReLU | LeakyReLU, Linear) on gshac_mlp2_act)
"""
import os

import torch

from .mlp import mlp2_forward
from .pcc_utils import calculate_morton_order, compress_point_cloud, decompress_point_cloud
from .torchac_encodings import decoder, encoder

bit2MB_scale = 8 * 1024 * 1024     # HAC/scene/gaussian_model.py:30 (HAC-plus :41, TC-GS :33, CAT-3DGS :51)
Q_FEAT, Q_SCALING, Q_OFFSETS = 1, 0.001, 0.2   # HAC :1147-1149 (HAC-plus :1277-1279, TC-GS :1206-1208, CAT-3DGS :1216-1218)
USE_CLAMP = True                   # HAC/utils/encodings.py:11 (use_clamp)


def default_ckpt_path():
    """HAC looks for <repo>/GausPcgc/best_model_ue_4stage_conv.pt (gaussian_model.py:1110-1112); here: $GAUSPCGC_CKPT."""
    p = os.environ.get("GAUSPCGC_CKPT")
    if not p:
        raise FileNotFoundError("pass ckpt_path=... or set GAUSPCGC_CKPT to best_model_ue_4stage_conv.pt (the reference ships no checkpoint)")
    return p


def ste_multistep(x, Q, input_mean):
    """STE_multistep.forward (HAC/utils/encodings.py:55-67)."""
    if USE_CLAMP:
        x = torch.clamp(x, min=(input_mean - 15_000 * Q).detach(), max=(input_mean + 15_000 * Q).detach())
    return torch.round(x / Q) * Q


# ---------------------------------------------------------------- slices
def n_slices(N, max_batch):
    return (N // max_batch) if (N % max_batch) == 0 else (N // max_batch + 1)


def slice_bounds(N, max_batch):
    """anchor index at every slice boundary: n_slices + 1 entries"""
    return [min(s * max_batch, N) for s in range(n_slices(N, max_batch) + 1)]


def slice_file_names(pre_path_name, stem, steps):
    """`<stem>_<s>.b` for every slice, built as the references build it"""
    return [os.path.join(pre_path_name, f'{stem}.b').replace('.b', f'_{s}.b') for s in range(steps)]


def offsets_mask(mask):
    """(N, K, 1) mask {0, 1} -> flat (N * K * 3) bool: the offset elements that are coded"""
    return mask.repeat(1, 1, 3).reshape(-1).to(torch.bool)


def offset_bounds(mask, N, bounds):
    """kept (masked-in) offset elements up to each slice boundary, mask the flat bool of offsets_mask: only the sums at the boundaries leave the
    device (a million-entry .tolist() was 10 ms)"""
    if N == 0:
        return [0] * len(bounds)
    kept = torch.cumsum(mask.view(N, -1).sum(dim=1), dim=0)
    # (dtype: the index of an empty list is float32 otherwise and cannot index)
    return [0] + kept[torch.tensor([b - 1 for b in bounds[1:]], dtype=torch.long, device=kept.device)].cpu().tolist()


# ---------------------------------------------------------------- anchors
def encode_anchors(anchor, voxel_size, ckpt_path, pre_path_name):
    """The AI-PCC block of conduct_encoding (HAC :1106-1117): the anchors on the voxel grid, in Morton order, to xyz_pcc.bin.  Returns (the anchors
    as the decoder will see them, the order to apply to the attributes, the file's size in bits)."""
    _anchor_int = torch.round(anchor / voxel_size)
    sorted_indices = calculate_morton_order(_anchor_int)
    _anchor_int = _anchor_int[sorted_indices]
    npz_path = os.path.join(pre_path_name, 'xyz_pcc.bin')
    out = compress_point_cloud(_anchor_int, ckpt_path or default_ckpt_path(), npz_path)
    return _anchor_int * voxel_size, sorted_indices, out['file_size_bits']


def decode_anchors(pre_path_name, ckpt_path, voxel_size, device):
    """The inverse in conduct_decoding (HAC :1250-1256): xyz_pcc.bin to the anchors, in Morton order"""
    npz_path = os.path.join(pre_path_name, 'xyz_pcc.bin')
    anchor_decoded = decompress_point_cloud(npz_path, ckpt_path or default_ckpt_path())
    _anchor_int_dec = anchor_decoded['point_cloud'].to(device)
    sorted_indices = calculate_morton_order(_anchor_int_dec)
    _anchor_int_dec = _anchor_int_dec[sorted_indices]
    return _anchor_int_dec * voxel_size


# ---------------------------------------------------------------- masks, torchac flavour
def encode_mask_stream(mask, file_name):
    """masks.b of TC-GS (:1289-1296) and CAT-3DGS (:1370-1375): mask {0, 1} as one Bernoulli stream under its own mean.  Returns (bits, prob_masks)."""
    p = torch.zeros_like(mask).to(torch.float32)
    prob_masks = (mask.sum() / mask.numel()).item()
    p[...] = prob_masks
    return encoder((mask * 2 - 1).view(-1), p.view(-1), file_name=file_name), prob_masks


def decode_mask_stream(N, n_off, prob_masks, file_name, device):
    """The inverse (TC-GS :1326-1331, CAT-3DGS :1417-1422): (N, n_off, 1) in {0, 1}"""
    p = torch.zeros(size=[N, n_off, 1], device=device).to(torch.float32)
    p[...] = prob_masks
    masks_decoded = decoder(p.view(-1), file_name)  # {-1, 1}
    masks_decoded = (masks_decoded + 1) / 2  # {0, 1}
    return masks_decoded.view(N, n_off, 1)


# ---------------------------------------------------------------- decoded parameters
def zero_filled(x):
    """TC-GS's and CAT-3DGS's "fill back N_full" (TC-GS :1429-1440, CAT-3DGS :1581-1592): a float32 zero tensor of x's shape with x copied in"""
    out = torch.zeros(size=list(x.shape), device=x.device)
    out[:x.shape[0]] = x
    return out


def install_decoded(model, anchor, feat, offsets, scaling, mask):
    """Replace the model's parameters with the decoded ones, in the references' order (HAC :1342-1348, HAC-plus :1554-1559, TC-GS :1445-1455, CAT-3DGS :1598-1608)"""
    nn = torch.nn
    model._anchor_feat = nn.Parameter(feat)
    model._offset = nn.Parameter(offsets)
    model.decoded_version = True      # the accessors stop applying activations / quantisers (HAC :1344)
    model._anchor = nn.Parameter(anchor)
    model._scaling = nn.Parameter(scaling)
    model._mask = nn.Parameter(mask)


# ---------------------------------------------------------------- context MLPs
def mlp2_parts(m):
    """(w1, b1, w2, b2, act, slope) of an nn.Sequential(Linear, ReLU | LeakyReLU, Linear) with both biases -- what the references build for
    mlp_grid, mlp_triplane, MLP_d*, mlp_chcm_* -- with act 'relu' (slope 0.0) or 'leaky_relu'; None for anything else."""
    mods = list(m) if isinstance(m, torch.nn.Sequential) else []
    if len(mods) != 3 or not isinstance(mods[0], torch.nn.Linear) or not isinstance(mods[2], torch.nn.Linear) or mods[0].bias is None or mods[2].bias is None:
        return None
    if isinstance(mods[1], torch.nn.ReLU):
        act, slope = "relu", 0.0
    elif isinstance(mods[1], torch.nn.LeakyReLU):
        act, slope = "leaky_relu", mods[1].negative_slope
    else:
        return None
    return mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, act, slope


def run_mlp2(m, x):
    """m(x).  A module mlp2_parts recognises goes through gshac_mlp2_act (specified fp32 order: encoder and decoder see identical parameters);
    anything else is called as it is."""
    parts = mlp2_parts(m)
    return m(x) if parts is None else mlp2_forward(x, *parts)
