"""generate_neural_gaussians of TC-GS (src/gs_compress/TC-GS/gaussian_renderer/__init__.py:22-206), training branch included: the import a
TC-GS checkout swaps in at gaussian_renderer/__init__.py:22, beside tcgs_codec as hac_plus_renderer is beside hac_plus_codec.

    from gauspcc_amd.tcgs_renderer import generate_neural_gaussians

`is_training=True` returns the reference's 12-tuple (:204, `lae` last), built from the library's pieces:

  visible_rows       the six `tensor[visible_mask]` gathers (none when visible_mask is None, as train.py calls it) and, through the same
                     select_rows, ONE gather by `choose_idx` of the noisy attributes, the context, the steps and the masks
  context_rows       the (N, K 3 C + 3) input of mlp_triplane -- the tri-plane features of pc.knnanchor (step > 15000) or of the anchor
                     written K times (the repeat form), with the anchor behind them -- in one kernel when pc.triplane is the library's
                     Triplane: no torch.cat, and the backward reads the MLP's input gradient in place.  Any other pc.triplane is called as
                     the reference calls it, followed by torch.cat
  the model's own    pc.get_tri_mlp, called as the model's module whatever it is (nn.Sequential or gauspcc_amd.mlp.ContextMLP), and
                     pc.entropy_gaussian.forward for the three rate terms with the reference's means
  attribute_noise    x + U(-0.5, 0.5) * Q0 * (1 + tanh(adj)) on feat, scaling and offsets in one launch (quant_noise), the adjustments read in
                     place from the last three columns of the context; in (3000, 10000] the constant step Q0
  the core           neural_gaussians_train(..., mask_after_opacity=False): TC-GS multiplies the mask into the opacity before the test (:152-162)

Where TC-GS differs from HAC's branch: Q_offsets is 0.3 here (:44; the codec's and estimate_final_bits' 0.2 is anchor_codec.Q_OFFSETS); 15 % of
the anchors are priced, not 5 %; step 10000 calls pc.updatebbox() and step 15000 pc.init_knn_indice(K) (that step still samples the repeat
form); the autoencoder loss `lae` = l1_loss(pc.triplane.planes, reconstruction) rides at the end of the training tuple.  pc.get_mask_anchor is a
bool (N,) property.  With step > 15000, pc.knnanchor must have one row per gathered anchor: the reference fails in torch.cat otherwise, here a
ValueError says so.

`is_training=False` returns the 6-tuple (:206).  An un-decoded model is quantised as the encoder would (:105-121, no step gate): the context of
the gathered anchors in repeat form, then quantise_steps -- the three STE_multistep calls in one launch -- with the means of the full tensors,
bracketed by the reference's two synchronisations for time_sub.  A decoded model runs no context and hands the visible anchors over as an index
list (neural_gaussians.rows_in_place).  Both end in gsnn_generate (neural_gaussians.emit_gaussians).

The random draws are the reference's, in its order (feat, scaling, offsets, then the rand_like), with its shapes, dtypes and devices, through
the two hooks below (tests replace them to replay recorded draws): under one torch.manual_seed the noise and the chosen anchors are the
reference's.
"""
import time

import torch

from .densify import select_rows
from .neural_gaussians import (attribute_noise, check_context_width, emit_gaussians, gathered_rows, neural_gaussians_train, quantise_steps, rate_means,
                               rows_in_place, visible_rows)
from .triplane import Triplane

Q_FEAT, Q_SCALING, Q_OFFSETS = 1, 0.001, 0.3      # :42-44; not anchor_codec.Q_OFFSETS, the codec's 0.2
Q0 = (Q_FEAT, Q_SCALING, Q_OFFSETS)
K = 4                                             # :21
CHOOSE = 0.15                                     # :78


def _uniform_like(t):
    return torch.empty_like(t).uniform_(-0.5, 0.5)


def _rand_like(t):
    return torch.rand_like(t)


def l1_loss(network_output, gt):
    """utils/loss_utils.py's l1_loss"""
    return torch.abs((network_output - gt)).mean()


def _noise(feat, scaling, offsets, adj):
    return attribute_noise(_uniform_like, feat, scaling, offsets, Q0, adj)


def context_input(pc, anchor, knnanchor, is_training, step):
    """(the (n, K 3 C + 3) input of mlp_triplane, compressed, reconstructed) for these anchors; knnanchor (n, K, 3), or None for the anchor
    itself K times.  Evaluation (is_training false) has no autoencoder pass: (rows, None, None)."""
    tri = pc.triplane
    if knnanchor is not None and knnanchor.shape[0] != anchor.shape[0]:
        raise ValueError(f"tcgs_renderer: pc.knnanchor has {knnanchor.shape[0]} rows, the gathered anchors {anchor.shape[0]}: the context is the "
                         f"neighbours' features beside the anchor, row by row (the reference fails here in torch.cat)")
    if isinstance(tri, Triplane):
        if knnanchor is None:
            out = tri.context_rows(anchor, anchor, pc.x_bound_max, pc.x_bound_min, is_training, step=step, repeat=K)
        else:
            out = tri.context_rows(knnanchor, anchor, pc.x_bound_max, pc.x_bound_min, is_training, step=step)
        return out if is_training else (out, None, None)
    if knnanchor is None:
        knnanchor = anchor.unsqueeze(1).repeat(1, K, 1)
    if is_training:
        feat_context, compressed, reconstructed = tri(knnanchor, pc.x_bound_max, pc.x_bound_min, is_training, step=step)
    else:
        feat_context, compressed, reconstructed = tri(knnanchor, pc.x_bound_max, pc.x_bound_min, is_training), None, None
    return torch.cat([feat_context, anchor], dim=1), compressed, reconstructed


def _context(pc, rows):
    ctx = pc.get_tri_mlp(rows)
    check_context_width("tcgs_renderer", "get_tri_mlp", "TC-GS's nine-way", ctx.shape, pc)
    return ctx


def generate_neural_gaussians(viewpoint_camera, pc, visible_mask=None, is_training=False, step=0):
    if not is_training:
        return _generate_inference(viewpoint_camera, pc, visible_mask)
    F, n_off = pc.feat_dim, pc.n_offsets
    model = (pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc.get_mask)
    mask_anchor = pc.get_mask_anchor
    anchor, feat, grid_offsets, grid_scaling, binary_grid_masks = visible_rows(visible_mask, *model)
    if visible_mask is not None:
        mask_anchor = mask_anchor[visible_mask]
    mask_anchor_bool = mask_anchor.detach().to(torch.bool).view(-1)
    mask_anchor_rate = (mask_anchor.sum() / mask_anchor.numel()).detach()
    bit_per_param = bit_per_feat_param = bit_per_scaling_param = bit_per_offsets_param = None
    lae = None
    if 3000 < step <= 10000:
        feat, grid_scaling, grid_offsets, _ = _noise(feat, grid_scaling, grid_offsets, None)
    if step == 10000:
        pc.updatebbox()
    if step == 15000:
        pc.init_knn_indice(K)
    if step > 10000:
        rows, _, reconstructed = context_input(pc, anchor, pc.knnanchor if step > 15000 else None, is_training, step)
        if reconstructed is not None:
            lae = l1_loss(pc.triplane.planes, reconstructed)
        ctx = _context(pc, rows)
        feat, grid_scaling, grid_offsets, Q = _noise(feat, grid_scaling, grid_offsets, ctx[:, -3:])
        choose_idx = (_rand_like(anchor[:, 0]) <= CHOOSE) & mask_anchor_bool
        feat_c, scaling_c, offsets_c, ctx_c, Q_c, masks_c = select_rows(choose_idx, feat, grid_scaling, grid_offsets, ctx, Q, binary_grid_masks)
        mean, scale, mean_scaling, scale_scaling, mean_offsets, scale_offsets, _, _, _ = torch.split(
            ctx_c, [F, F, 6, 6, 3 * n_off, 3 * n_off, 1, 1, 1], dim=-1)
        masks_c = masks_c.repeat(1, 1, 3).view(-1, 3 * n_off)
        bit_feat = pc.entropy_gaussian.forward(feat_c, mean, scale, Q_c[:, 0:1], pc._anchor_feat.mean())
        bit_scaling = pc.entropy_gaussian.forward(scaling_c, mean_scaling, scale_scaling, Q_c[:, 1:2], pc.get_scaling.mean())
        bit_offsets = pc.entropy_gaussian.forward(offsets_c.view(-1, 3 * n_off), mean_offsets, scale_offsets, Q_c[:, 2:3], pc._offset.mean())
        bit_offsets = bit_offsets * masks_c
        bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param = rate_means(bit_feat, bit_scaling, bit_offsets, mask_anchor_rate)
    xyz, color, opacity, scaling, rot, neural_opacity, keep = neural_gaussians_train(anchor, feat, grid_offsets, grid_scaling, binary_grid_masks,
                                                                                     viewpoint_camera.camera_center, pc, mask_after_opacity=False)
    return (xyz, color, opacity, scaling, rot, neural_opacity, keep, bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param,
            lae)


@torch.no_grad()
def _generate_inference(viewpoint_camera, pc, visible_mask):
    if pc.decoded_version:      # no context
        tensors, rows, n = rows_in_place(pc, visible_mask, pc.get_mask)
        return (*emit_gaussians(viewpoint_camera, pc, n, rows, *tensors), 0)
    anchor, feat, grid_offsets, grid_scaling, binary_grid_masks = gathered_rows(pc, visible_mask, pc.get_mask)
    n = anchor.shape[0]
    time_sub = 0
    if n:       # quantise as the encoder would (:105-121); nothing visible runs no context and is not timed
        torch.cuda.synchronize(); t1 = time.time()
        ctx = _context(pc, context_input(pc, anchor, None, False, 0)[0])
        feat, grid_scaling, grid_offsets, _ = quantise_steps([feat, grid_scaling, grid_offsets], Q0, ctx[:, -3:],
                                                             means=(pc._anchor_feat.mean(), pc.get_scaling.mean(), pc._offset.mean()))
        torch.cuda.synchronize(); time_sub = time.time() - t1
    return (*emit_gaussians(viewpoint_camera, pc, n, None, anchor, feat, grid_offsets, grid_scaling, binary_grid_masks), time_sub)
