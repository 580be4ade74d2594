"""generate_neural_gaussians of CAT-3DGS (src/gs_compress/CAT-3DGS/gaussian_renderer/__init__.py:25-213), training branch included: the
import a CAT-3DGS checkout swaps in at gaussian_renderer/__init__.py:25, beside cat_codec as hac_plus_renderer is beside hac_plus_codec.

    from gauspcc_amd.cat_renderer import generate_neural_gaussians

`is_training=True` returns the reference's 12-tuple (:211), built from the library's pieces:

  visible_rows       the six `tensor[visible_mask]` gathers (none when visible_mask is None) and, through the same select_rows, the gathers
                     by `choose_idx`: one call per set
  attribute_noise    x + U(-0.5, 0.5) * Q0 * (1.1 + tanh(adj)) on feat, scaling and offsets in one launch (quant_noise, base = 1.1), the
                     adjustments read in place from the last three columns of feature_net's output; in (3000, 10000] the constant step
                     Q0 * 1.1
  the model's own    feature_net (called as the model's module, its own random draws first: it trains too) and the channel-context MLPs
                     get_chcm_mlp_list / _scaling / _offsets, called as modules on feat_chosen[:, :dep_ch]
  chain_rate         every stage of the channel-wise context chain -- the feat groups, scaling, offsets -- priced in one launch and
                     differentiated in one (gsac_chain_rate_forward / _backward); the row layout is cat_codec.stage_table's
  the core           neural_gaussians_train(..., mask_after_opacity=False): CAT-3DGS multiplies the mask into the opacity before the test

Where CAT-3DGS differs from HAC's branch: the context is feature_net(anchor, itr=step) -> (ctx, feat_rate) with the SCALES first in a row;
the step rule is 1.1 + tanh; the rate branch also runs at step == -1; the chosen anchors are priced by the channel-wise context model;
get_mask and get_mask_anchor are methods that take the `mask=` argument; feat_rate rides at the end of both tuples.

`is_training=False` returns the 7-tuple (:213).  An un-decoded model from step 10000 on (or at -1) is quantised as the encoder would
(:139-151: the context, the three steps, STE_multistep with the means of the full tensors), bracketed by the reference's two
synchronisations for time_sub; below that the attributes go in as they are.  A decoded model runs no context, feat_rate = 0, and hands
the visible anchors over as an index list (neural_gaussians.rows_in_place).  Both end in gsnn_generate (neural_gaussians.emit_gaussians).

The random draws are the reference's, in its order, with its shapes, dtypes and devices, through the two hooks below (tests replace them
to replay recorded draws): under one torch.manual_seed the noise and the chosen anchors are the reference's.
"""
import time
import types

import torch

from .anchor_codec import Q_FEAT, Q_OFFSETS, Q_SCALING, ste_multistep
from .cat_codec import stage_table
from .densify import select_rows
from .entropy_models import chain_rate
from .neural_gaussians import (attribute_noise, check_context_width, emit_gaussians, gathered_rows, neural_gaussians_train, rate_means, rows_in_place,
                               visible_rows)

Q0 = (Q_FEAT, Q_SCALING, Q_OFFSETS)
BASE = 1.1


def _uniform_like(t):
    return torch.empty_like(t).uniform_(-0.5, 0.5)


def _rand_like(t):
    return torch.rand_like(t)


def _stages(pc):
    """cat_codec.stage_table on what the renderer reads of the model (the get_chcm_* accessors)"""
    view = types.SimpleNamespace(feat_dim=pc.feat_dim, n_offsets=pc.n_offsets, chcm_slices_list=pc.chcm_slices_list, num_feat_slices=len(pc.chcm_slices_list),
                                 chcm_for_scaling=pc.chcm_for_scaling, chcm_for_offsets=pc.chcm_for_offsets, mlp_chcm_list=pc.get_chcm_mlp_list,
                                 mlp_chcm_scaling=pc.get_chcm_mlp_scaling, mlp_chcm_offsets=pc.get_chcm_mlp_offsets)
    return stage_table(view)


def _context(pc, anchor, step):
    ctx, feat_rate = pc.feature_net(anchor, itr=step)
    check_context_width("cat_renderer", "feature_net", "CAT-3DGS's nine-way", ctx.shape, pc)
    return ctx, feat_rate


def generate_neural_gaussians(viewpoint_camera, pc, visible_mask=None, is_training=False, step=0, mask=None):
    if not is_training:
        return _generate_inference(viewpoint_camera, pc, visible_mask, step, mask)
    F, K = pc.feat_dim, pc.n_offsets
    model = (pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc.get_mask(mask), pc.get_mask_anchor(mask).to(torch.float32).unsqueeze(1))
    anchor, feat, grid_offsets, grid_scaling, binary_grid_masks, mask_anchor = visible_rows(visible_mask, *model)
    mask_anchor_bool = mask_anchor.detach()[:, 0] != 0
    mask_anchor_rate = (mask_anchor_bool.sum() / mask_anchor_bool.numel()).detach()
    feat_rate = 0
    bit_per_param = bit_per_feats_param = bit_per_scaling_param = bit_per_offsets_param = None
    if 3000 < step <= 10000:    # (u * Q0) * 1.1 in the reference: the constant step Q0 * 1.1, formed in double
        feat, grid_scaling, grid_offsets, _ = attribute_noise(_uniform_like, feat, grid_scaling, grid_offsets, [q * BASE for q in Q0])
    if step == 10000:       # the tri-plane's bound
        pc.update_anchor_bound()
    if step > 10000 or step == -1:
        ctx, feat_rate = _context(pc, anchor, step)
        feat, grid_scaling, grid_offsets, Q = attribute_noise(_uniform_like, feat, grid_scaling, grid_offsets, Q0, ctx[:, -3:], base=BASE)
        choose_idx = (_rand_like(anchor[:, 0]) <= 0.05) & mask_anchor_bool
        feat_c, scaling_c, offsets_c, ctx_c, Q_c, masks_c = select_rows(choose_idx, feat, grid_scaling, grid_offsets, ctx, Q, binary_grid_masks)
        stages = _stages(pc)
        m = feat_c.shape[0]
        residuals = [st["mlp"](feat_c[:, :st["dep_ch"]]) if st["mlp"] is not None and m else None for st in stages]
        x_means = (pc._anchor_feat.mean(), pc.get_scaling.mean(), pc._offset.mean())
        bits = chain_rate(ctx_c, feat_c, scaling_c, offsets_c, Q_c, x_means, stages, residuals, offset_mask=masks_c,
                          q_floor=getattr(pc.entropy_gaussian, "q_floor", None) or 1e-9)
        bit_feats, bit_scaling, bit_offsets = bits[:, :F], bits[:, F:F + 6], bits[:, F + 6:]
        bit_per_param, bit_per_feats_param, bit_per_scaling_param, bit_per_offsets_param = rate_means(bit_feats, bit_scaling, bit_offsets, mask_anchor_rate)
    xyz, color, opacity, scaling, rot, neural_opacity, keep = neural_gaussians_train(anchor, feat, grid_offsets, grid_scaling, binary_grid_masks,
                                                                                     viewpoint_camera.camera_center, pc, mask_after_opacity=False)
    return (xyz, color, opacity, scaling, rot, neural_opacity, keep, bit_per_param, bit_per_feats_param, bit_per_scaling_param, bit_per_offsets_param,
            feat_rate)


@torch.no_grad()
def _generate_inference(viewpoint_camera, pc, visible_mask, step, mask):
    if pc.decoded_version:      # no context, feat_rate = 0
        tensors, rows, n = rows_in_place(pc, visible_mask, pc.get_mask(mask))
        return (*emit_gaussians(viewpoint_camera, pc, n, rows, *tensors), 0, 0)
    anchor, feat, grid_offsets, grid_scaling, binary_grid_masks = gathered_rows(pc, visible_mask, pc.get_mask(mask))
    n = anchor.shape[0]
    time_sub, feat_rate = 0, 0
    if step >= 10000 or step == -1:     # quantise as the encoder would (:139-151); feature_net runs and is timed on an empty set too, as there
        torch.cuda.synchronize(); t1 = time.time()
        ctx, feat_rate = _context(pc, anchor, step)
        adj = ctx[:, -3:]
        q_feat, q_scaling, q_offsets = (q0 * (BASE + torch.tanh(adj[:, j:j + 1])) for j, q0 in enumerate(Q0))
        if n:
            feat = ste_multistep(feat, q_feat, pc._anchor_feat.mean())
            grid_scaling = ste_multistep(grid_scaling, q_scaling, pc.get_scaling.mean())
            grid_offsets = ste_multistep(grid_offsets, q_offsets.unsqueeze(1), pc._offset.mean())
        torch.cuda.synchronize(); time_sub = time.time() - t1
    return (*emit_gaussians(viewpoint_camera, pc, n, None, anchor, feat, grid_offsets, grid_scaling, binary_grid_masks), time_sub, feat_rate)
