"""generate_neural_gaussians of HAC (src/gs_compress/HAC/gaussian_renderer/__init__.py:25-172) and of HAC++
(src/gs_compress/HAC-plus/gaussian_renderer/__init__.py:25-205) for RD evaluation -- SURVEY.md §8(f) row 2: anchors -> the
Gaussians the rasteriser draws.  The two differ in two places, both handled here: an un-decoded HAC++ model's mlp_grid has the extra
`prob` head (a TEN-way split, :121-123, against HAC's nine, :103-105), and HAC++ applies the binary offset masks AFTER the opacity
test (:188-205) where HAC multiplies them into the opacity before it (:136-137) -- the same set of Gaussians with the same values
(the masks are {0, 1}), which is what gsnn_generate computes.

    from gauspcc_amd.neural_gaussians import generate_neural_gaussians
    xyz, color, opacity, scaling, rot, time_sub = generate_neural_gaussians(viewpoint_camera, pc, visible_mask)

`is_training=True` serves HAC's training branch (:47-98 and the 11-tuple of :170): the gathers, the quantisation noise, the
context model's rate terms on the 5 % chosen anchors (the model's own torch modules: they train too) and then the differentiable core
neural_gaussians_train (gsnn_forward_train / gsnn_backward), which HAC++, TC-GS and CAT-3DGS callers can use after their own rate code.
HAC++'s training branch is gauspcc_amd.hac_plus_renderer, CAT-3DGS's renderer gauspcc_amd.cat_renderer, TC-GS's gauspcc_amd.tcgs_renderer, all built on that core, on quant_noise
below (gsnn_noise_forward_b / _backward_b) and on the frame the four renderers share (the section after quantise_steps): the row sets
of inference (gathered_rows, rows_in_place) and its end (emit_gaussians), the visible rows of training (visible_rows), the attribute noise
(attribute_noise), the four rate means (rate_means), the context-width check (check_context_width) and the walk over the MLPs' parameters
(mlp_tensors).  What stays in each renderer is what its model does differently: its context, its quantisation with the time_sub bracket
and its rule for an empty set, its rate terms.
The model `pc` is used through the attributes the reference uses.  When `pc.decoded_version` is false the attributes are first quantised
with the context model's step sizes exactly as the reference does (:103-114); everything after that -- view vectors,
feature bank, the three MLPs, masking, assembly -- is ONE call into libgauspcc (gsnn_generate: two kernels and a scan
instead of ~40 PyTorch kernels and an (n K, 22) concatenate / mask / split).  For a decoded model the visible anchors go in as an
index list: the kernels read those rows of the model's tensors in place instead of five `tensor[visible_mask]` copies.
"""
import ctypes as C
import math
import time

import torch
from torch.autograd.function import once_differentiable

from . import _lib, runtime
from .runtime import ptr, ptrs
from .anchor_codec import Q_FEAT, Q_OFFSETS, Q_SCALING, run_mlp2, ste_multistep
from .densify import select_rows


def quant_steps(pc, anchor):
    """Step sizes of the three attributes from the context model, for an un-decoded model (HAC :103-111, HAC++ :121-132): the last three
    columns of mlp_grid's output whatever heads sit in front of them -- nine-way split (HAC: mean, scale, 2 x scaling, 2 x offsets) or
    ten-way (HAC++: + prob).  Returns (Q_feat (N, F), Q_scaling (N, 6), Q_offsets (N, 3 K)); HAC++ views the last as (N, K, 3), the same values."""
    F, K = pc.feat_dim, pc.n_offsets
    out = run_mlp2(pc.get_grid_mlp, pc.calc_interp_feat(anchor))
    nine, ten = 2 * F + 12 + 6 * K + 3, 3 * F + 12 + 6 * K + 3
    if out.shape[1] not in (nine, ten):
        raise ValueError(f"mlp_grid returns {out.shape[1]} columns; HAC has {nine} (feat_dim {F}, {K} offsets), HAC++ {ten}")
    qa_f, qa_s, qa_o = out[:, -3:-2], out[:, -2:-1], out[:, -1:]
    return ((Q_FEAT * (1 + torch.tanh(qa_f.contiguous()))).repeat(1, F), (Q_SCALING * (1 + torch.tanh(qa_s.contiguous()))).repeat(1, 6),
            (Q_OFFSETS * (1 + torch.tanh(qa_o.contiguous()))).repeat(1, 3 * K))


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


class _NeuralGaussians(torch.autograd.Function):
    """gsnn_forward_train / gsnn_backward.  The backward's state is the scan of the keep flags, (n K + 1) uint32 in a tensor on the autograd
    context (through the library's allocator callback): the hidden layers are recomputed, so other library calls may run in between."""

    @staticmethod
    def forward(ctx, mask_after, anchor, feat, grid_offsets, grid_scaling, masks, cam, *params):
        dev = anchor.device
        n, F = feat.shape
        K = grid_offsets.shape[1]
        ins = [_f32(anchor), _f32(feat), _f32(grid_offsets), _f32(grid_scaling), _f32(masks).view(n, K), _f32(cam).view(3)]
        ws = [None if p is None else _f32(p) for p in params]
        nk = n * K
        xyz, color, scaling = (torch.empty(nk, 3, device=dev) for _ in range(3))
        opacity, rot = torch.empty(nk, 1, device=dev), torch.empty(nk, 4, device=dev)
        nopa = torch.empty(nk, 1, device=dev)
        keep = torch.empty(nk, dtype=torch.bool, device=dev)
        work = runtime.Workspace(dev)
        pos, m = C.c_void_p(), C.c_int64()
        _lib.check(_lib.lib().gsnn_forward_train(runtime.context(dev), n, F, K, *[t.data_ptr() for t in ins], ptrs(ws, 16), int(bool(mask_after)), xyz.data_ptr(),
                                                 color.data_ptr(), opacity.data_ptr(), scaling.data_ptr(), rot.data_ptr(), nopa.data_ptr(), keep.data_ptr(),
                                                 work.fn(), None, C.byref(pos), C.byref(m), runtime.stream_ptr(dev)))
        m = m.value
        ctx.state = (work, pos.value, bool(mask_after), n, F, K, masks.shape, grid_offsets.shape)
        ctx.save_for_backward(*ins, *ws)
        ctx.mark_non_differentiable(keep)
        return xyz[:m], color[:m], opacity[:m], scaling[:m], rot[:m], nopa, keep

    @staticmethod
    @once_differentiable
    def backward(ctx, g_xyz, g_color, g_opacity, g_scaling, g_rot, g_nopa, g_keep):
        _, pos, mask_after, n, F, K, mshape, oshape = ctx.state
        saved = ctx.saved_tensors
        ins, ws = saved[:6], list(saved[6:])
        dev = ins[0].device
        gs = [_f32(g) for g in (g_xyz, g_color, g_opacity, g_scaling, g_rot, g_nopa)]
        d_anchor, d_feat = torch.empty(n, 3, device=dev), torch.empty(n, F, device=dev)
        d_off, d_sc, d_mask = torch.empty(n, K, 3, device=dev), torch.empty(n, 6, device=dev), torch.empty(n, K, device=dev)
        d_ws = [None if w is None else torch.empty_like(w) for w in ws]
        _lib.check(_lib.lib().gsnn_backward(runtime.context(dev), n, F, K, *[t.data_ptr() for t in ins], ptrs(ws, 16), int(mask_after), pos,
                                            *[g.data_ptr() for g in gs], d_anchor.data_ptr(), d_feat.data_ptr(), d_off.data_ptr(), d_sc.data_ptr(),
                                            d_mask.data_ptr(), ptrs(d_ws, 16), runtime.Workspace(dev).fn(), None, runtime.stream_ptr(dev)))
        return (None, d_anchor, d_feat, d_off.view(oshape), d_sc, d_mask.view(mshape), None, *d_ws)


def neural_gaussians_train(anchor, feat, grid_offsets, grid_scaling, masks, cam_center, pc, mask_after_opacity=False):
    """The differentiable core of the training branch: anchors (n, 3), feat (n, F), grid_offsets (n, K, 3), grid_scaling (n, 6) and
    masks (n, K, 1) -- used as given, the straight-through value included -- to the kept Gaussians.  Returns (xyz, color, opacity, scaling,
    rot, neural_opacity (n K, 1), keep (n K) bool).  mask_after_opacity=False: HAC (:134-141, the mask in the opacity before the test);
    True: HAC++ (HAC-plus/gaussian_renderer/__init__.py:158-203: keep = tanh > 0, the mask multiplies the kept rows' opacity and scaling).
    Gradients reach the five attribute tensors and every Linear of the three or four MLPs; camera centre and keep get none."""
    F, K = feat.shape[1], grid_offsets.shape[1]
    if F not in (32, 50) or not 1 <= K <= 64:
        raise _lib.GpccError(-1, f"neural_gaussians_train: feat_dim must be 32 or 50 and n_offsets 1..64 (got {F}, {K})")
    cam = cam_center.reshape(3)
    return _NeuralGaussians.apply(bool(mask_after_opacity), anchor, feat, grid_offsets, grid_scaling, masks, cam, *mlp_tensors(pc))


def _noise_args(xs, us, q0s, adj, cols):
    """(n, widths, the ctypes arrays gsnn_noise_* share) after the argument checks"""
    who = "quant_noise"
    T = len(xs)
    if not 1 <= T <= 3 or len(us) != T or len(q0s) != T:
        raise ValueError(f"{who}: xs, us and q0s must hold the same number (1..3) of entries, got {len(xs)}, {len(us)}, {len(q0s)}")
    n = xs[0].shape[0] if isinstance(xs[0], torch.Tensor) and xs[0].dim() >= 1 else -1
    for name, ts in (("xs", xs), ("us", us)):
        for j, t in enumerate(ts):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
                raise ValueError(f"{who}: {name}[{j}] must be a float32 CUDA tensor")
            if t.dim() < 2 or t.shape != xs[j].shape or t.shape[0] != n or t.device != xs[0].device:
                raise ValueError(f"{who}: {name}[{j}] of shape {tuple(t.shape)}: every attribute is (n, ...) and its noise has its shape")
    widths = [math.prod(x.shape[1:]) for x in xs]
    if any(w < 1 for w in widths):
        raise ValueError(f"{who}: xs must have at least one column each")
    if adj is not None:
        if not isinstance(adj, torch.Tensor) or adj.dtype != torch.float32 or not adj.is_cuda or adj.device != xs[0].device:
            raise ValueError(f"{who}: adj must be a float32 CUDA tensor on the attributes' device")
        cols = list(range(T)) if cols is None else [int(c) for c in cols]
        if adj.dim() != 2 or adj.shape[0] != n or len(cols) != T or any(not 0 <= c < adj.shape[1] for c in cols):
            raise ValueError(f"{who}: adj must be ({n}, >= {T}) and cols name {T} of its columns, got {tuple(adj.shape)} and {cols}")
    elif cols is not None:
        raise ValueError(f"{who}: cols without adj")
    return n, widths, (C.c_int64 * T)(*widths), (C.c_double * T)(*[float(q) for q in q0s]), None if adj is None else (C.c_int * T)(*cols)


def _adj_view(adj):
    """adj as the kernels read it in place: unit column stride and rows that do not overlap (a column slice of mlp_grid's output is one)"""
    return adj if adj.stride(1) == 1 and adj.stride(0) >= adj.shape[1] else adj.contiguous()


class _QuantNoise(torch.autograd.Function):
    """gsnn_noise_forward / gsnn_noise_backward.  Inputs: adj (or None), then the attributes; the noise and the rest ride on `cfg`."""

    @staticmethod
    def forward(ctx, cfg, adj, *xs):
        us, q0s, cols, base = cfg
        n, widths, c_w, c_q, c_cols = _noise_args(xs, us, q0s, adj, cols)
        dev, T = xs[0].device, len(xs)
        xc = [x.detach().contiguous() for x in xs]
        uc = [u.detach().contiguous() for u in us]
        ys = [torch.empty_like(x) for x in xc]
        q = torch.empty(n, T, device=dev)
        a = None if adj is None else _adj_view(adj.detach())
        if n:
            _lib.check(_lib.lib().gsnn_noise_forward_b(runtime.context(dev), n, T, ptrs(xc), ptrs(uc), c_w, c_q, ptr(a), a.stride(0) if a is not None else 0, c_cols,
                                                       base, ptrs(ys), q.data_ptr(), runtime.stream_ptr(dev)))
        ctx.cfg = (n, T, c_w, c_q, c_cols, uc, a, base)
        return (*ys, q)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        n, T, c_w, c_q, c_cols, uc, a, base = ctx.cfg
        gs, gq = grads[:T], grads[T]
        d_adj = None
        if a is not None and ctx.needs_input_grad[1]:
            dev = uc[0].device
            gc = [torch.zeros_like(u) if g is None else g.detach().contiguous() for g, u in zip(gs, uc)]
            d = torch.empty(n, T, device=dev)
            gqc = None if gq is None else gq.detach().contiguous()
            if n:
                _lib.check(_lib.lib().gsnn_noise_backward_b(runtime.context(dev), n, T, ptrs(gc), ptrs(uc), c_w, c_q, a.data_ptr(), a.stride(0), c_cols, base,
                                                            ptr(gqc), d.data_ptr(), runtime.stream_ptr(dev)))
            cols = list(c_cols)
            if a.shape[1] == T and cols == list(range(T)):
                d_adj = d
            else:
                d_adj = torch.zeros(a.shape, device=dev)
                d_adj[:, cols] = d
        return (None, d_adj, *gs)       # dx_j is the incoming gradient itself


def quant_noise(xs, us, q0s, adj=None, cols=None, base=1.0):
    """The adaptive-step quantisation noise on up to three row-aligned attributes in one launch (gsnn_noise_forward_b):
    y_j = xs[j] + us[j] * Q_j with Q_j[r] = q0s[j] * (base + tanh(adj[r, cols[j]])), or the constant q0s[j] without adj.  base is 1 for the
    HAC family and 1.1 for CAT-3DGS; CAT-3DGS's constant regime, x + (u * Q0) * 1.1, is this without adj and with q0s[j] = Q0 * 1.1 formed in
    double: one rounding where the reference's expression has two, a difference below an ulp of the noise term.  us are the caller's
    U(-0.5, 0.5) draws, shaped as xs.  adj is read in place: a column slice of mlp_grid's output costs no copy (cols default to 0, 1, ...).
    Returns (y_0, ..., Q) with Q (n, len(xs)) the per-row steps, which the rate modules take as (n, 1) operands.  Differentiable in xs (the
    gradient is the incoming tensor itself) and adj (gsnn_noise_backward, bitwise reproducible).  Float32 CUDA tensors only."""
    _noise_args(xs, us, q0s, adj, cols)
    return _QuantNoise.apply((list(us), list(q0s), cols, float(base)), adj, *xs)


def fixed_order_mean(*xs):
    """The means of up to three float32 CUDA tensors as a (len(xs),) device tensor, each a double sum in a fixed order rounded once
    (gsnn_mean): bitwise reproducible, within float32 rounding of `x.mean()`.  What `quantise_steps` uses when it is given no means."""
    if not 1 <= len(xs) <= 3 or any(not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda for x in xs):
        raise ValueError("fixed_order_mean: one to three float32 CUDA tensors")
    dev = xs[0].device
    xc = [x.detach().contiguous() for x in xs]
    T = len(xc)
    partials = torch.empty(T * 256, dtype=torch.float64, device=dev)
    means = torch.empty(T, device=dev)
    _lib.check(_lib.lib().gsnn_mean(runtime.context(dev), T, ptrs(xc), (C.c_int64 * T)(*[x.numel() for x in xc]), partials.data_ptr(), means.data_ptr(),
                                    runtime.stream_ptr(dev)))
    return means


@torch.no_grad()
def quantise_steps(xs, q0s, adj, cols=None, base=1.0, means=None):
    """STE_multistep's forward on up to three row-aligned attributes in one launch (gsnn_quantise), the evaluation side of `quant_noise`:
    y_j = round(clamp(xs[j], m_j - 15000 Q_j, m_j + 15000 Q_j) / Q_j) * Q_j with Q_j[r] = q0s[j] * (base + tanh(adj[r, cols[j]])); adj is read
    in place (a column slice of the context MLP's output costs no copy).  means: one 0-d tensor or number per attribute (the reference's
    `pc._anchor_feat.mean()`, ...), or None for the means of the xs themselves (STE_multistep's default `input.mean()`), which
    `fixed_order_mean` forms in two more launches.  The clamp follows anchor_codec.USE_CLAMP.  Returns (y_0, ..., Q) with Q (n, len(xs)) as
    quant_noise returns it.  Detached: no backward (every caller of the reference detaches the result).  Float32 CUDA tensors only."""
    from . import anchor_codec
    if adj is None:
        raise ValueError("quantise_steps: adj is required (the step is Q0 * (base + tanh(adj)))")
    n, widths, c_w, c_q, c_cols = _noise_args(xs, xs, q0s, adj, cols)
    dev, T = xs[0].device, len(xs)
    xc = [x.detach().contiguous() for x in xs]
    if means is None:
        m = fixed_order_mean(*xc)
    else:
        if len(means) != T:
            raise ValueError(f"quantise_steps: {len(means)} means for {T} attributes")
        m = torch.stack([torch.as_tensor(v, dtype=torch.float32, device=dev).detach().reshape(()) for v in means])
    ys = [torch.empty_like(x) for x in xc]
    q = torch.empty(n, T, device=dev)
    a = _adj_view(adj.detach())
    if n:
        _lib.check(_lib.lib().gsnn_quantise(runtime.context(dev), n, T, ptrs(xc), c_w, c_q, a.data_ptr(), a.stride(0), c_cols, float(base), m.data_ptr(),
                                            int(bool(anchor_codec.USE_CLAMP)), ptrs(ys), q.data_ptr(), runtime.stream_ptr(dev)))
    return (*ys, q)


# ---- the frame the four renderers share (this module's, hac_plus_renderer, tcgs_renderer, cat_renderer) ------------------------------------

def mlp_tensors(pc, convert=None):
    """{w1, b1, w2, b2} of mlp_feature_bank (None x 4 without the bank), mlp_opacity, mlp_cov, mlp_color: the 16 parameters themselves, so
    that autograd delivers their gradients, or each through `convert` (inference reads detached float32 contiguous copies)."""
    def walk(seq):
        mods = [m for m in seq if isinstance(m, torch.nn.Linear)]
        if len(mods) != 2:
            raise TypeError("expected nn.Sequential(Linear, ReLU, Linear, ...) as built in HAC/scene/gaussian_model.py:229-256")
        params = (mods[0].weight, mods[0].bias, mods[1].weight, mods[1].bias)
        return list(params) if convert is None else [convert(p) for p in params]
    bank = walk(pc.get_featurebank_mlp) if getattr(pc, "use_feat_bank", False) else [None] * 4
    return bank + walk(pc.get_opacity_mlp) + walk(pc.get_cov_mlp) + walk(pc.get_color_mlp)


def gathered_rows(pc, visible_mask, masks):
    """Inference on an un-decoded model: (anchor, feat, grid_offsets, grid_scaling, binary_grid_masks) as the reference's five
    `tensor[visible_mask]` gathers (:54-58), on which it then quantises.  `masks` is the model's offset-mask tensor (a property in HAC, HAC++
    and TC-GS, `pc.get_mask(mask)` in CAT-3DGS); visible_mask None is the all-ones mask."""
    if visible_mask is None:
        visible_mask = torch.ones(pc.get_anchor.shape[0], dtype=torch.bool, device=pc.get_anchor.device)
    return pc.get_anchor[visible_mask], pc._anchor_feat[visible_mask], pc._offset[visible_mask], pc.get_scaling[visible_mask], masks[visible_mask]


def rows_in_place(pc, visible_mask, masks):
    """Inference on a decoded model: ((the five tensors of the model as they are), rows, n) with `rows` the visible anchors as an int32 index
    list (None: all of them) and n their number.  The kernels read those rows in place: the reference's five gathers are 0.8 GB of copies
    per million anchors."""
    rows, n = None, pc.get_anchor.shape[0]
    if visible_mask is not None:
        rows = torch.nonzero(visible_mask).view(-1).to(torch.int32)
        n = rows.numel()
    return (pc.get_anchor, pc._anchor_feat, pc._offset, pc.get_scaling, masks), rows, n


@torch.no_grad()
def emit_gaussians(viewpoint_camera, pc, n, rows, anchor, feat, grid_offsets, grid_scaling, binary_grid_masks):
    """The end of every inference path: gsnn_generate on n anchors -- the rows `rows` (int32 index list) of the tensors, or all of them (rows
    None) -- to (xyz, color, opacity, scaling, rot).  n == 0 gives five empty tensors: the reference's tensor program runs on empty tensors
    (:33-38, 115-167), here there is no device buffer to hand over."""
    dev = anchor.device
    if n == 0:
        return tuple(torch.empty(0, c, device=dev) for c in (3, 3, 1, 3, 4))
    K, F = pc.n_offsets, pc.feat_dim
    tensors = mlp_tensors(pc, _f32)
    anchor, feat, grid_offsets, grid_scaling = _f32(anchor), _f32(feat), _f32(grid_offsets), _f32(grid_scaling)
    mask = _f32(binary_grid_masks).view(-1, K)
    cam = _f32(viewpoint_camera.camera_center).view(3)
    xyz = torch.empty(n * K, 3, device=dev); color = torch.empty(n * K, 3, device=dev); opacity = torch.empty(n * K, 1, device=dev)
    scaling = torch.empty(n * K, 3, device=dev); rot = torch.empty(n * K, 4, device=dev)
    m = C.c_int64()
    _lib.check(_lib.lib().gsnn_generate(runtime.context(dev), n, ptr(rows), F, K, anchor.data_ptr(), feat.data_ptr(),
                                        grid_offsets.data_ptr(), grid_scaling.data_ptr(), mask.data_ptr(), cam.data_ptr(), ptrs(tensors, 16), xyz.data_ptr(), color.data_ptr(),
                                        opacity.data_ptr(), scaling.data_ptr(), rot.data_ptr(), C.byref(m), runtime.stream_ptr(dev)))
    m = m.value
    return xyz[:m], color[:m], opacity[:m], scaling[:m], rot[:m]


def visible_rows(visible_mask, *model):
    """Training: the model's tensors at the visible anchors, differentiably (densify.select_rows: one scan, one launch and one wait for the
    set).  visible_mask None is every anchor, as train.py calls it: the tensors as given, nothing to gather."""
    return model if visible_mask is None else select_rows(visible_mask, *model)


def attribute_noise(draw, feat, scaling, offsets, q0s, adj=None, base=1.0):
    """The three attributes with their quantisation noise and the (n, 3) steps: fresh draws through `draw` -- the calling module's
    U(-0.5, 0.5) hook, which the caller fetches from its module's globals at call time so that tests can replace it -- in the reference's
    order feat, scaling, offsets, then quant_noise."""
    us = [draw(feat), draw(scaling), draw(offsets)]
    return quant_noise([feat, scaling, offsets], us, q0s, adj, base=base)


def rate_means(bit_feat, bit_scaling, bit_offsets, factor=None):
    """(bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param) of the three bit tables, each sum / numel in the
    reference's expression order, times `factor` (the mask-anchor rate of HAC, TC-GS and CAT-3DGS; HAC++ has none and multiplies nothing)."""
    scaled = (lambda m: m) if factor is None else (lambda m: m * factor)
    per_attribute = [scaled(torch.sum(b) / b.numel()) for b in (bit_feat, bit_scaling, bit_offsets)]
    total = scaled((torch.sum(bit_feat) + torch.sum(bit_scaling) + torch.sum(bit_offsets)) / (bit_feat.numel() + bit_scaling.numel() + bit_offsets.numel()))
    return (total, *per_attribute)


def out_columns(mlp):
    """the width of what an nn.Sequential context MLP returns, before it runs: its last Linear's"""
    return [m for m in mlp if isinstance(m, torch.nn.Linear)][-1].out_features


def check_context_width(who, accessor, split, shape, pc, heads=2, hint=""):
    """The context's width against the model's: `shape` is the shape of what pc.<accessor> returns (or will return) for the anchors,
    `heads` the F-wide heads of a row (mean and scale; HAC++'s ten-way split has `prob` too) in front of the 12 + 6 K + 3 other columns."""
    F, K = pc.feat_dim, pc.n_offsets
    width = heads * F + 12 + 6 * K + 3
    if len(shape) != 2 or shape[1] != width:
        raise ValueError(f"{who}: pc.{accessor} returns a context of shape {tuple(shape)}, {split} split has {width} columns "
                         f"(feat_dim {F}, {K} offsets){hint}")
    return width


# ---- HAC's renderer (and HAC++'s inference) ------------------------------------------------------------------------------------------------

def generate_neural_gaussians(viewpoint_camera, pc, visible_mask=None, is_training=False, step=0):
    if is_training:
        return _generate_training(viewpoint_camera, pc, visible_mask, step)
    return _generate_inference(viewpoint_camera, pc, visible_mask)


@torch.no_grad()
def _generate_inference(viewpoint_camera, pc, visible_mask):
    if pc.decoded_version:
        tensors, rows, n = rows_in_place(pc, visible_mask, pc.get_mask)
        return (*emit_gaussians(viewpoint_camera, pc, n, rows, *tensors), 0)
    anchor, feat, grid_offsets, grid_scaling, binary_grid_masks = gathered_rows(pc, visible_mask, pc.get_mask)
    n = anchor.shape[0]
    time_sub = 0
    if n:       # quantise as the encoder would (:103-114), on the gathered rows; nothing visible runs no context and is not timed
        torch.cuda.synchronize(); t1 = time.time()
        q_feat, q_scaling, q_offsets = quant_steps(pc, anchor)
        feat = ste_multistep(feat, q_feat, pc._anchor_feat.mean())
        grid_scaling = ste_multistep(grid_scaling, q_scaling, pc.get_scaling.mean())
        grid_offsets = ste_multistep(grid_offsets.reshape(n, -1), q_offsets, pc._offset.mean()).view_as(grid_offsets)
        torch.cuda.synchronize(); time_sub = time.time() - t1
    return (*emit_gaussians(viewpoint_camera, pc, n, None, anchor, feat, grid_offsets, grid_scaling, binary_grid_masks), time_sub)


def _generate_training(viewpoint_camera, pc, visible_mask, step):
    """HAC's training branch (:25-98, 170): noise, rate terms, then the core.  The random draws are the reference's, in its order, with its
    shapes, dtypes and devices, so that under one torch.manual_seed the noise and the chosen anchors are the reference's."""
    F, K = pc.feat_dim, pc.n_offsets
    if out_columns(pc.get_grid_mlp) != 2 * F + 12 + 6 * K + 3:
        raise NotImplementedError("generate_neural_gaussians(is_training=True) serves HAC's rate branch (nine-way mlp_grid split); for HAC++ call "
                                  "gauspcc_amd.neural_gaussians.neural_gaussians_train(..., mask_after_opacity=True) after the model's own rate code")
    if visible_mask is None:
        visible_mask = torch.ones(pc.get_anchor.shape[0], dtype=torch.bool, device=pc.get_anchor.device)
    anchor = pc.get_anchor[visible_mask]
    feat = pc._anchor_feat[visible_mask]
    grid_offsets = pc._offset[visible_mask]
    grid_scaling = pc.get_scaling[visible_mask]
    binary_grid_masks = pc.get_mask[visible_mask]
    mask_anchor = pc.get_mask_anchor[visible_mask]
    mask_anchor_bool = mask_anchor.to(torch.bool)
    mask_anchor_rate = (mask_anchor.sum() / mask_anchor.numel()).detach()
    bit_per_param = bit_per_feat_param = bit_per_scaling_param = bit_per_offsets_param = None
    Q_feat, Q_scaling, Q_offsets = 1, 0.001, 0.2
    if 3000 < step <= 10000:
        feat = feat + torch.empty_like(feat).uniform_(-0.5, 0.5) * Q_feat
        grid_scaling = grid_scaling + torch.empty_like(grid_scaling).uniform_(-0.5, 0.5) * Q_scaling
        grid_offsets = grid_offsets + torch.empty_like(grid_offsets).uniform_(-0.5, 0.5) * Q_offsets
    if step == 10000:
        pc.update_anchor_bound()
    if step > 10000:
        ctxf = pc.get_grid_mlp(pc.calc_interp_feat(anchor))
        mean, scale, mean_scaling, scale_scaling, mean_offsets, scale_offsets, qf, qs, qo = torch.split(ctxf, [F, F, 6, 6, 3 * K, 3 * K, 1, 1, 1], dim=-1)
        Q_feat = Q_feat * (1 + torch.tanh(qf))
        Q_scaling = Q_scaling * (1 + torch.tanh(qs))
        Q_offsets = Q_offsets * (1 + torch.tanh(qo))
        feat = feat + torch.empty_like(feat).uniform_(-0.5, 0.5) * Q_feat
        grid_scaling = grid_scaling + torch.empty_like(grid_scaling).uniform_(-0.5, 0.5) * Q_scaling
        grid_offsets = grid_offsets + torch.empty_like(grid_offsets).uniform_(-0.5, 0.5) * Q_offsets.unsqueeze(1)
        choose = (torch.rand_like(anchor[:, 0]) <= 0.05) & mask_anchor_bool
        masks_chosen = binary_grid_masks[choose].repeat(1, 1, 3).view(-1, 3 * K)
        bit_feat = pc.entropy_gaussian.forward(feat[choose], mean[choose], scale[choose], Q_feat[choose], pc._anchor_feat.mean())
        bit_scaling = pc.entropy_gaussian.forward(grid_scaling[choose], mean_scaling[choose], scale_scaling[choose], Q_scaling[choose], pc.get_scaling.mean())
        bit_offsets = pc.entropy_gaussian.forward(grid_offsets[choose].view(-1, 3 * K), mean_offsets[choose], scale_offsets[choose], Q_offsets[choose],
                                                  pc._offset.mean())
        bit_offsets = bit_offsets * masks_chosen
        bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param = rate_means(bit_feat, bit_scaling, bit_offsets, mask_anchor_rate)
    xyz, color, opacity, scaling, rot, neural_opacity, keep = neural_gaussians_train(anchor, feat, grid_offsets, grid_scaling, binary_grid_masks,
                                                                                     viewpoint_camera.camera_center, pc)
    return xyz, color, opacity, scaling, rot, neural_opacity, keep, bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param
