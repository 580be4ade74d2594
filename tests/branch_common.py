"""What the three training-branch pins (HAC++, TC-GS, CAT-3DGS) share on the test side: the replay of recorded random draws
(tests/*_train_cases.py), the walk over the core MLPs' parameters and the base of the shadow models (tests/*_branch_ref.py).  The
restatements themselves stay in their own files, independent of the library and of each other: they are the references.
"""
import copy

import torch


class Replay:
    """Stand-ins for a renderer's two hooks that hand out `draws` -- the recorded draws of a run in the branch's order, the fourth the
    rand_like -- checking shape and kind of each request.  `torch`: the module the caller runs on (the generators pass a CPU build)."""

    def __init__(self, draws, torch):
        self.torch, self.queue, self.served = torch, list(enumerate(draws)), 0

    def _next(self, t, is_rand):
        assert self.queue, "more draws than recorded"
        i, d = self.queue.pop(0)
        assert (i == 3) == is_rand and tuple(d.shape) == tuple(t.shape), (i, is_rand, d.shape, tuple(t.shape))
        self.served += 1
        return self.torch.tensor(d).to(device=t.device, dtype=t.dtype)

    def uniform_like(self, t):
        return self._next(t, False)

    def rand_like(self, t):
        return self._next(t, True)


def _linears(seq):
    out = []
    for m in seq:
        if isinstance(m, torch.nn.Linear):
            out += [m.weight, m.bias]
    return out


def core_params(pc):
    """the 16 tensors tests/ng_train_ref.py takes: the feature bank's (None x 4 without one), opacity's, cov's, colour's"""
    bank = _linears(pc.get_featurebank_mlp) if getattr(pc, "use_feat_bank", False) else [None] * 4
    return bank + _linears(pc.get_opacity_mlp) + _linears(pc.get_cov_mlp) + _linears(pc.get_color_mlp)


class ShadowModel:
    """What the three shadow models agree on: pc in `dtype` on `device` (default: pc's) with _anchor_feat, _offset, the scaling and _mask
    (where pc has them as parameters) as leaves that require grad and the three core MLPs (and the feature bank) as deep copies.  The
    subclasses add their model's modules, hooks and mask accessors (a property in HAC++ and TC-GS, a method in CAT-3DGS)."""

    def __init__(self, pc, dtype, device=None):
        self.dev = device or pc.get_anchor.device
        self.src, self.dtype = pc, dtype
        self.feat_dim, self.n_offsets, self.use_feat_bank = pc.feat_dim, pc.n_offsets, bool(getattr(pc, "use_feat_bank", False))
        self._anchor_feat, self._offset = self.leaf(pc._anchor_feat), self.leaf(pc._offset)
        self._scaling = self.leaf(pc._scaling) if hasattr(pc, "_scaling") else None
        self._scaling_value = None if self._scaling is not None else self.leaf(pc.get_scaling)
        self._mask = self.leaf(pc._mask) if hasattr(pc, "_mask") else None
        self.get_opacity_mlp, self.get_cov_mlp, self.get_color_mlp = self.mod(pc.get_opacity_mlp), self.mod(pc.get_cov_mlp), self.mod(pc.get_color_mlp)
        if self.use_feat_bank:
            self.get_featurebank_mlp = self.mod(pc.get_featurebank_mlp)

    def value(self, t):
        return t.detach().to(device=self.dev, dtype=self.dtype)

    def leaf(self, t):
        return self.value(t).clone().requires_grad_(True)

    def mod(self, m):
        return None if m is None else copy.deepcopy(m).to(device=self.dev, dtype=self.dtype)

    @property
    def get_scaling(self):
        return torch.exp(self._scaling) if self._scaling is not None else self._scaling_value

    @property
    def scaling_leaf(self):
        """the leaf behind get_scaling: pc's _scaling parameter or, where it has none, a copy of the scaling values"""
        return self._scaling if self._scaling is not None else self._scaling_value

    @staticmethod
    def straight_through(s):
        """the binary mask of sigmoid values s with the gradient of s"""
        return ((s > 0.01).to(s.dtype) - s).detach() + s

    def walk(self, leaves, mods):
        """name -> tensor in a fixed order: `leaves`, the mask parameter, then every parameter of `mods`, a list of (name, module or None)"""
        out = dict(leaves)
        if self._mask is not None:
            out["_mask"] = self._mask
        for name, m in mods:
            if m is not None:
                for k, p in m.named_parameters():
                    out[f"{name}.{k}"] = p
        return out
