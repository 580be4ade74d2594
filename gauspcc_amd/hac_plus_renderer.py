"""generate_neural_gaussians of HAC++ (src/gs_compress/HAC-plus/gaussian_renderer/__init__.py:25-207), training branch included: the
import a HAC++ checkout swaps in at gaussian_renderer/__init__.py:25, beside hac_plus_codec as neural_gaussians is beside hac_codec.

    from gauspcc_amd.hac_plus_renderer import generate_neural_gaussians

`is_training=False` is neural_gaussians.generate_neural_gaussians, which serves HAC++ inference.  `is_training=True` is the reference's
branch (:46-119 and the 11-tuple of :207) built from the library's pieces:

  visible_rows       the five `tensor[visible_mask]` gathers (none when visible_mask is None) and, through the same select_rows, the six
                     `tensor[choose_idx]` gathers: one scan, one launch and one wait per set (gpcc_compact_rows), one launch without a
                     wait in the backward (gpcc_expand_rows)
  attribute_noise    x + U(-0.5, 0.5) * Q0 * (1 + tanh(adj)) on feat, scaling and offsets in one launch per set (quant_noise:
                     gsnn_noise_forward); the adjustments are read in place from mlp_grid's output, the per-row steps go to the rate
                     modules as (n, 1) operands
  the model's own    calc_interp_feat, get_grid_mlp, get_deform_mlp, EG_mix_prob_2, entropy_gaussian, called as modules (they train too)
  the core           neural_gaussians_train(..., mask_after_opacity=True)

Where HAC++ differs from HAC's branch (neural_gaussians.generate_neural_gaussians with is_training=True): the ten-way mlp_grid split with
`prob` third; the 5 % of anchors for the rate terms are drawn over ALL anchors, not intersected with mask_anchor, gathered from the full model, put through the
context a second time and given their own noise; the feat rate is the two-component mixture with the channel-context MLP's second
component; mask_anchor (n, 1) multiplies the bits instead of a mask-rate factor on the means.

The random draws are the reference's, in its order, with its shapes, dtypes and devices, through the two hooks below (tests replace them
to replay recorded draws): under one torch.manual_seed the noise and the chosen anchors are the reference's.  The chosen set's three noise
tensors are drawn together before the channel-context MLP runs; the reference draws two of them after it, with no draw in between.
"""
import torch

from . import neural_gaussians
from .densify import select_rows
from .neural_gaussians import attribute_noise, check_context_width, neural_gaussians_train, out_columns, rate_means, visible_rows

Q0 = (1, 0.001, 0.2)


def _uniform_like(t):
    return torch.empty_like(t).uniform_(-0.5, 0.5)


def _rand_like(t):
    return torch.rand_like(t)


def _context(pc, anchor, width):
    """mlp_grid's output for these anchors; an empty set runs nothing"""
    if anchor.shape[0] == 0:
        return anchor.new_zeros(0, width)
    return pc.get_grid_mlp(pc.calc_interp_feat(anchor))


def _noise(feat, scaling, offsets, adj):
    return attribute_noise(_uniform_like, feat, scaling, offsets, Q0, adj)


def generate_neural_gaussians(viewpoint_camera, pc, visible_mask=None, is_training=False, step=0):
    if not is_training:
        return neural_gaussians.generate_neural_gaussians(viewpoint_camera, pc, visible_mask, is_training=False, step=step)
    F, K = pc.feat_dim, pc.n_offsets
    width = check_context_width("hac_plus_renderer", "get_grid_mlp", "HAC++'s ten-way", (pc.get_anchor.shape[0], out_columns(pc.get_grid_mlp)), pc, heads=3,
                                hint="; HAC's branch is gauspcc_amd.neural_gaussians.generate_neural_gaussians")
    split = [F, F, F, 6, 6, 3 * K, 3 * K, 1, 1, 1]
    model = (pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, pc.get_mask)
    anchor, feat, grid_offsets, grid_scaling, binary_grid_masks = visible_rows(visible_mask, *model)
    bit_per_param = bit_per_feat_param = bit_per_scaling_param = bit_per_offsets_param = None
    if 3000 < step <= 10000:
        feat, grid_scaling, grid_offsets, _ = _noise(feat, grid_scaling, grid_offsets, None)
    if step == 10000:
        pc.update_anchor_bound()
    if step > 10000:
        # for rendering: the visible anchors' three step adjustments
        feat, grid_scaling, grid_offsets, _ = _noise(feat, grid_scaling, grid_offsets, _context(pc, anchor, width)[:, -3:])
        # for entropy: 5 % of ALL anchors, through the context again, with their own noise
        choose_idx = _rand_like(pc.get_anchor[:, 0]) <= 0.05
        anchor_c, feat_c, offsets_c, scaling_c, masks_c, mask_anchor_c = select_rows(choose_idx, *model, pc.get_mask_anchor)
        ctx = _context(pc, anchor_c, width)
        mean, scale, prob, mean_scaling, scale_scaling, mean_offsets, scale_offsets, _, _, _ = torch.split(ctx, split, dim=-1)
        feat_c, scaling_c, offsets_c, Q = _noise(feat_c, scaling_c, offsets_c, ctx[:, -3:])
        mean_adj, scale_adj, prob_adj = pc.get_deform_mlp.forward(feat_c, ctx[:, :3 * F])
        probs = torch.softmax(torch.stack([prob, prob_adj], dim=-1), dim=-1)
        masks_c = masks_c.repeat(1, 1, 3).view(-1, 3 * K)
        bit_feat = pc.EG_mix_prob_2.forward(feat_c, mean, mean_adj, scale, scale_adj, probs[..., 0], probs[..., 1], Q=Q[:, 0:1], x_mean=pc._anchor_feat.mean())
        bit_feat = bit_feat * mask_anchor_c
        bit_scaling = pc.entropy_gaussian.forward(scaling_c, mean_scaling, scale_scaling, Q[:, 1:2], pc.get_scaling.mean())
        bit_scaling = bit_scaling * mask_anchor_c
        bit_offsets = pc.entropy_gaussian.forward(offsets_c.view(-1, 3 * K), mean_offsets, scale_offsets, Q[:, 2:3], pc._offset.mean())
        bit_offsets = bit_offsets * mask_anchor_c * masks_c
        bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param = rate_means(bit_feat, bit_scaling, bit_offsets)
    xyz, color, opacity, scaling, rot, neural_opacity, keep = neural_gaussians_train(anchor, feat, grid_offsets, grid_scaling, binary_grid_masks,
                                                                                     viewpoint_camera.camera_center, pc, mask_after_opacity=True)
    return xyz, color, opacity, scaling, rot, neural_opacity, keep, bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param
