"""Plain torch restatement of TC-GS's generate_neural_gaussians (the contract of gauspcc_amd.tcgs_renderer) and of its estimate_final_bits
(gauspcc_amd.tcgs_codec), written from the branch's definition; both run in the dtype and on the device of the model they are given (float64
or float32).  The core is tests/ng_train_ref.py (mask_after=False), the rate terms tests/rate_ref.py's rate_torch.  The random draws come from
the renderer's two hooks (looked up at call time, so a test that replaces them replays the same draws into both programs), in the branch's
order: feat / scaling / offsets noise of the gathered anchors, then the rand_like over them.

pc.triplane is called as the reference calls it, on the materialised (n, K, 3) neighbours, followed by torch.cat: for the library's Triplane
in float32 that is the parent's sampler + cat.  PlaneRef is a torch statement of the sampler itself (grid_sample on the three planes) for
float64.

ShadowModel copies a model (gauspcc_amd.synth.SyntheticGaussianModelTC or the object of tests/tcgs_train_cases.py) into another dtype with
every trainable tensor a fresh leaf, so that the restatement's gradients can be read off it.
"""
import torch

from tests import branch_common
from tests.branch_common import core_params
from tests.ng_train_ref import ng_train_ref
from tests.rate_ref import rate_torch

Q0 = (1, 0.001, 0.3)
Q0_ESTIMATE = (1, 0.001, 0.2)
K = 4
CHOOSE = 0.15


def _hooks():
    from gauspcc_amd import tcgs_renderer
    return tcgs_renderer._uniform_like, tcgs_renderer._rand_like


def _ste(x, q, xm):
    return torch.round(torch.clamp(x, min=(xm - 15000 * q).detach(), max=(xm + 15000 * q).detach()) / q) * q


def tcgs_branch_ref(cam, pc, visible_mask, step, is_training=True, mutate=None):
    """The 12-tuple (training) or the 6-tuple.  mutate (the generator's sensitivity checks, restated): 'q_offsets02' uses the codec's 0.2,
    'threshold005' HAC's 5 %, 'no_mask_anchor' leaves the intersection with mask_anchor out, 'drop_offset_mask' the offsets mask,
    'repeat_form' samples the anchor K times past step 15000 too, 'no_rate_factor' drops mask_anchor_rate."""
    uniform_like, rand_like = _hooks()
    F, n_off = pc.feat_dim, pc.n_offsets
    q0 = (Q0[0], Q0[1], 0.2) if mutate == "q_offsets02" else Q0
    if visible_mask is None:
        visible_mask = torch.ones(pc.get_anchor.shape[0], dtype=torch.bool, device=pc.get_anchor.device)
    anchor, feat, offs = pc.get_anchor[visible_mask], pc._anchor_feat[visible_mask], pc._offset[visible_mask]
    scl, masks = pc.get_scaling[visible_mask], pc.get_mask[visible_mask]
    mask_anchor = pc.get_mask_anchor[visible_mask].to(torch.bool)
    ma_rate = 1.0 if mutate == "no_rate_factor" else (mask_anchor.sum() / mask_anchor.numel()).detach().to(feat.dtype)
    W = 2 * F + 12 + 6 * n_off + 3
    steps = lambda ctx: [q * (1 + torch.tanh(ctx[:, W - 3 + j:W - 2 + j])) for j, q in enumerate(q0)]   # noqa: E731
    bits, lae, time_sub = [None] * 4, None, 0
    if is_training:
        if 3000 < step <= 10000:
            feat = feat + uniform_like(feat) * q0[0]
            scl = scl + uniform_like(scl) * q0[1]
            offs = offs + uniform_like(offs) * q0[2]
        if step == 10000:
            pc.updatebbox()
        if step == 15000:
            pc.init_knn_indice(K)
        if step > 10000:
            knn = pc.knnanchor if step > 15000 and mutate != "repeat_form" else anchor.unsqueeze(1).repeat(1, K, 1)
            f, _, rec = pc.triplane(knn, pc.x_bound_max, pc.x_bound_min, is_training, step=step)
            if rec is not None:
                lae = torch.abs(pc.triplane.planes - rec).mean()
            ctx = pc.get_tri_mlp(torch.cat([f, anchor], dim=1))
            qf, qs, qo = steps(ctx)
            feat = feat + uniform_like(feat) * qf
            scl = scl + uniform_like(scl) * qs
            offs = offs + uniform_like(offs) * qo.unsqueeze(1)
            ch = rand_like(anchor[:, 0]) <= (0.05 if mutate == "threshold005" else CHOOSE)
            if mutate != "no_mask_anchor":
                ch = ch & mask_anchor
            mean, scale, mean_s, scale_s, mean_o, scale_o, _, _, _ = torch.split(ctx[ch], [F, F, 6, 6, 3 * n_off, 3 * n_off, 1, 1, 1], dim=-1)
            bf = rate_torch(feat[ch], [mean], [scale], None, qf[ch], pc._anchor_feat.mean())
            bs = rate_torch(scl[ch], [mean_s], [scale_s], None, qs[ch], pc.get_scaling.mean())
            bo = rate_torch(offs[ch].view(-1, 3 * n_off), [mean_o], [scale_o], None, qo[ch], pc._offset.mean())
            if mutate != "drop_offset_mask":
                bo = bo * masks[ch].repeat(1, 1, 3).view(-1, 3 * n_off)
            bits = [(bf.sum() + bs.sum() + bo.sum()) / (bf.numel() + bs.numel() + bo.numel()) * ma_rate, bf.sum() / bf.numel() * ma_rate,
                    bs.sum() / bs.numel() * ma_rate, bo.sum() / bo.numel() * ma_rate]
    elif not pc.decoded_version:
        f = pc.triplane(anchor.unsqueeze(1).repeat(1, K, 1), pc.x_bound_max, pc.x_bound_min, is_training)
        qf, qs, qo = steps(pc.get_tri_mlp(torch.cat([f, anchor], dim=1)))
        feat, scl, offs = _ste(feat, qf, pc._anchor_feat.mean()), _ste(scl, qs, pc.get_scaling.mean()), _ste(offs, qo.unsqueeze(1), pc._offset.mean())
    out = ng_train_ref(anchor, feat, offs, scl, masks, cam.camera_center, core_params(pc), False)
    if is_training:
        return (*out, *bits, lae)
    return (*out[:5], time_sub)


@torch.no_grad()
def estimate_bits_ref(pc, knn_indices):
    """(bit_feat, bit_scaling, bit_offsets) of estimate_final_bits, from `knn_indices` (n_kept, K) as update_knn leaves them"""
    F, n_off = pc.feat_dim, pc.n_offsets
    keep = pc.get_mask_anchor
    anchor, feat, offs, scl, mask = pc.get_anchor[keep], pc._anchor_feat[keep], pc._offset[keep], pc.get_scaling[keep], pc.get_mask[keep]
    knn = pc._anchor[knn_indices]
    f = pc.triplane(knn, pc.x_bound_max, pc.x_bound_min)
    ctx = pc.get_tri_mlp(torch.cat([f, anchor], dim=1))
    mean, scale, mean_s, scale_s, mean_o, scale_o, af, a_s, ao = torch.split(ctx, [F, F, 6, 6, 3 * n_off, 3 * n_off, 1, 1, 1], dim=-1)
    qf, qs, qo = (q * (1 + torch.tanh(adj)) for q, adj in zip(Q0_ESTIMATE, (af, a_s, ao)))
    feat, scl, offs = _ste(feat, qf, feat.mean()), _ste(scl, qs, scl.mean()), _ste(offs, qo.unsqueeze(1), offs.mean()).view(-1, 3 * n_off)
    bf, bs = rate_torch(feat, [mean], [scale], None, qf, None), rate_torch(scl, [mean_s], [scale_s], None, qs, None)
    bo = rate_torch(offs, [mean_o], [scale_o], None, qo, None) * mask.repeat(1, 1, 3).view(-1, 3 * n_off)
    return float(bf.sum()), float(bs.sum()), float(bo.sum())


class PlaneRef(torch.nn.Module):
    """utils/triplane.py's Triplane restated on torch's grid_sample, in the dtype of `planes`: the sampler's contract of include/gauspcc.h
    (box_warp 1, the three fixed axes, bilinear, zero padding) with the reference's call signature and return convention."""

    def __init__(self, planes, radii, autoencoder=None):
        super().__init__()
        self.planes = torch.nn.Parameter(planes.detach().clone())
        self.radii = radii
        self.autoencoder = autoencoder          # Triplane's conv autoencoder (a copy in this module's dtype), or None: no reconstruction

    def forward(self, coords, max_coords, min_coords, is_training=0, step=0):
        n, k, _ = coords.shape
        mx, mn = max_coords.reshape(3), min_coords.reshape(3)
        r2 = torch.as_tensor((0.5 * self.radii) ** 2, dtype=coords.dtype, device=coords.device)
        pairs = ((0, 1), (0, 2), (2, 0))                       # the bounds' projections: (x, y), (x, z), (z, x)
        comps = ((1, 2), (0, 2), (0, 1))                       # the coordinate's: (y, z), (x, z), (x, y)
        outs = []
        for p in range(3):
            i, j = pairs[p]
            mag = torch.sqrt(torch.minimum(torch.minimum(mx[i] ** 2 + mx[j] ** 2, mn[i] ** 2 + mn[j] ** 2), r2))
            u = 2 * coords[..., list(comps[p])]
            x = 6 * (u / mag * 2 - 1)
            m = torch.clamp((x * x).sum(-1, keepdim=True), min=torch.finfo(torch.float32).eps)
            z = torch.where(m <= 1, x, (2 * torch.sqrt(m) - 1) / m * x)
            g = (z / 2).reshape(1, n * k, 1, 2)
            s = torch.nn.functional.grid_sample(self.planes[p:p + 1], g, mode="bilinear", padding_mode="zeros", align_corners=False)
            outs.append(s.reshape(self.planes.shape[1], n * k).t())           # (n k, C)
        out = torch.stack(outs, dim=1).reshape(n, -1)                         # (n, k 3 C)
        if is_training and step > 15000 and self.autoencoder is not None:
            pairs = [self.autoencoder(self.planes[i].unsqueeze(0)) for i in range(3)]
            return out, torch.stack([c for c, _ in pairs], dim=0), torch.stack([r for _, r in pairs], dim=0)
        return (out, None, None) if is_training else out


class ShadowModel(branch_common.ShadowModel):
    """branch_common.ShadowModel with TC-GS's modules and the anchor as a leaf too; `triplane` the given module (it must run in `dtype`) or a
    deep copy of pc's, `tri_mlp` likewise."""

    def __init__(self, pc, dtype, device=None, triplane=None, tri_mlp=None):
        super().__init__(pc, dtype, device)
        self.decoded_version = pc.decoded_version
        self.get_anchor = self.leaf(pc.get_anchor)
        self._anchor = self.get_anchor
        self._mask01 = None if self._mask is not None else self.value(pc._mask01)
        self.triplane = triplane if triplane is not None else self.mod(pc.triplane)
        self.get_tri_mlp = tri_mlp if tri_mlp is not None else self.mod(pc.get_tri_mlp)
        self.x_bound_max, self.x_bound_min = (self.value(b).reshape(3) for b in (pc.x_bound_max, pc.x_bound_min))
        self.knnanchor = self.value(pc.knnanchor)
        self.entropy_gaussian = getattr(pc, "entropy_gaussian", None)
        self.hooks = []

    def updatebbox(self):
        self.hooks.append("updatebbox")

    def init_knn_indice(self, k):
        self.hooks.append(("init_knn_indice", k))

    @property
    def get_mask(self):
        return self._mask01 if self._mask is None else self.straight_through(torch.sigmoid(self._mask))

    @property
    def get_mask_anchor(self):
        with torch.no_grad():
            return torch.sum(self.get_mask, dim=1)[:, 0] > 0

    def trainable(self):
        """name -> tensor of everything the branch's gradients reach, in a fixed order"""
        leaves = {"anchor": self.get_anchor, "_anchor_feat": self._anchor_feat, "_offset": self._offset, "_scaling": self.scaling_leaf}
        mods = [("triplane", self.triplane), ("tri_mlp", self.get_tri_mlp), ("opacity", self.get_opacity_mlp), ("cov", self.get_cov_mlp),
                ("color", self.get_color_mlp)]
        if self.use_feat_bank:
            mods.append(("bank", self.get_featurebank_mlp))
        return {k: p for k, p in self.walk(leaves, mods).items() if not k.startswith("triplane.autoencoder")}
