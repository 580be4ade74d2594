"""GausPcgc's context network as a trainable nn.Module (src/ai_pcc/GausPcgc/network_ue_4stage_conv.py:11-182).

`Network(channels, kernel_size)` has exactly the upstream state-dict keys and shapes, so `torch.save(net.state_dict(), p)` writes a
checkpoint that `model.load_state_dict`, `compress_point_cloud` / `decompress_point_cloud` and the CLIs take unchanged, and its
`forward(x)` returns the reference's training loss: bits per input point, sum clamp(-log2(p_gt + 1e-10), 0, 50) / N.

The 18 sparse convolutions run on the codec's gfx950 kernels through the octree frame of one cloud (include/gauspcc.h,
gpcc_train_*): one launch per layer over a whole set of levels, the encoder's teacher-forced layout.  Their backward is HIP too
(the input gradient is the same kernel with mirrored weights, the weight gradient a fixed-order MFMA reduction).  Embeddings, the
child-feature gather, the heads and the loss are plain torch.  Convolution rows stay in the library's physical channel order from the
first embedding to the heads: the embedding tables and the heads' first layers are indexed by that permutation instead, so no
activation is ever permuted.  32 channels only (the MFMA path).
"""
import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib, runtime


def _logical_of(p: int) -> int:   # csrc/network.hpp: physical column -> logical channel
    kk = 4 * (p >> 4) + (p & 3)
    return 4 * kk + ((p & 15) >> 2)


PHYS_TO_LOGICAL = tuple(_logical_of(p) for p in range(32))


class _Frame:
    """The octree and tile lists of one cloud in caller (torch) memory, plus its nodes as tensors."""

    def __init__(self, xyz: torch.Tensor, kernel_size: int):
        dev = xyz.device
        self.device = dev
        self.work = runtime.Workspace(dev)
        self.state = (C.c_uint64 * _lib.GPCC_TRAIN_STATE_WORDS)()
        L = C.c_int32()
        nodes = (C.c_int64 * 24)()
        xyz = xyz.to(torch.int32).contiguous()
        _lib.check(_lib.lib().gpcc_train_frame(runtime.context(dev), xyz.data_ptr(), xyz.shape[0], int(kernel_size), self.work.fn(), None, self.state,
                                               C.byref(L), nodes, runtime.stream_ptr(dev)))
        self.L = L.value
        self.level_nodes = [int(nodes[d]) for d in range(self.L)]
        total = sum(self.level_nodes)
        self.n0 = self.level_nodes[0]
        self.nP = total - self.level_nodes[-1] if self.L > 1 else 0
        self.nC = total - self.n0 if self.L > 1 else 0
        self.occ = torch.empty(total, dtype=torch.uint8, device=dev)
        self.coords = torch.empty((total, 3), dtype=torch.int32, device=dev)
        self.parent = torch.empty(max(self.nC, 1), dtype=torch.int32, device=dev)
        self.octant = torch.empty(max(self.nC, 1), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().gpcc_train_frame_nodes(runtime.context(dev), self.state, self.occ.data_ptr(), self.parent.data_ptr(),
                                                     self.octant.data_ptr(), self.coords.data_ptr(), runtime.stream_ptr(dev)))
        self.parent, self.octant = self.parent[: self.nC].long(), self.octant[: self.nC].long()

    def rows(self, s: int) -> int:
        return self.nC if s else self.nP


def _frags(w: torch.Tensor, mirror: int) -> torch.Tensor:
    K = w.shape[0]
    k = round(K ** (1.0 / 3.0))
    out = torch.empty(K * 2048, dtype=torch.float32, device=w.device)
    _lib.check(_lib.lib().gpcc_train_weights(runtime.context(w.device), w.data_ptr(), int(w.shape[1]), k, mirror, out.data_ptr(),
                                             runtime.stream_ptr(w.device)))
    return out


class _SparseConvFn(torch.autograd.Function):
    """out = conv(x) (+ res) (ReLU): rows of one set of a frame, physical channel order; w (K, 32, 32) upstream layout."""

    @staticmethod
    def forward(ctx, x, w, res, frame, s, relu):
        x = x.contiguous()
        w = w.detach().contiguous()
        r = None if res is None else res.contiguous()
        out = torch.empty_like(x)
        _lib.check(_lib.lib().gpcc_train_conv(runtime.context(x.device), frame.state, s, x.data_ptr(), _frags(w, 0).data_ptr(),
                                              None if r is None else r.data_ptr(), int(bool(relu)), out.data_ptr(), runtime.stream_ptr(x.device)))
        ctx.frame, ctx.s, ctx.relu, ctx.has_res = frame, s, bool(relu), res is not None
        ctx.save_for_backward(x, w, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, out = ctx.saved_tensors
        frame, s = ctx.frame, ctx.s
        dev = x.device
        if ctx.relu:
            g = g * (out > 0)
        g = g.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.check(_lib.lib().gpcc_train_conv(runtime.context(dev), frame.state, s, g.data_ptr(), _frags(w, 1).data_ptr(), None, 0,
                                                  dx.data_ptr(), runtime.stream_ptr(dev)))
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            _lib.check(_lib.lib().gpcc_train_wgrad(runtime.context(dev), frame.state, s, x.data_ptr(), g.data_ptr(), runtime.Workspace(dev).fn(), None,
                                                   dw.data_ptr(), runtime.stream_ptr(dev)))
        return dx, dw, (g if ctx.has_res else None), None, None, None


def sparse_conv(x, w, frame, s, res=None, relu=False):
    """Differentiable convolution over set s (0 = prior, 1 = target) of `frame`; rows in the physical channel order."""
    if x.shape[1] != 32 or tuple(w.shape[1:]) != (32, 32):
        raise ValueError("the training convolution runs 32 channels")
    return _SparseConvFn.apply(x, w, res, frame, s, relu)


class SparseConv3d(nn.Module):
    """spnn.Conv3d(C, C, k), stride 1, no bias: the parameter is `kernel` (k^3, Cin, Cout), this library's offset enumeration."""

    def __init__(self, channels, kernel_size):
        super().__init__()
        K = kernel_size ** 3
        bound = 1.0 / np.sqrt(channels * K)
        self.kernel = nn.Parameter(torch.empty(K, channels, channels).uniform_(-bound, bound))

    def forward(self, x, frame, s, res=None, relu=False):
        return sparse_conv(x, self.kernel, frame, s, res, relu)


class _ReLU(nn.Module):   # keeps the upstream Sequential indices (spnn.ReLU at 1); the ReLU itself is fused into the convolution
    def forward(self, x):
        return x


class ResNet(nn.Module):
    def __init__(self, channels, k):
        super().__init__()
        self.conv0 = SparseConv3d(channels, k)
        self.conv1 = SparseConv3d(channels, k)

    def forward(self, x, frame, s):   # kit/nn.py:18-22: relu(conv1(relu(conv0(x))) + x)
        return self.conv1(self.conv0(x, frame, s, relu=True), frame, s, res=x, relu=True)


class TargetEmbedding(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.target_res_embedding = nn.Embedding(8, channels)


class _FogConv(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("kernel", torch.ones(8, 1, 1))   # FOG's constant (8, 1, 1) kernel of ones (kit/nn.py:31-34): state only


class FOG(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = _FogConv()


def _trunk(seq, x, frame, s):   # Conv-ReLU-ResNet-ResNet (network_ue_4stage_conv.py:17-33)
    x = seq[0](x, frame, s, relu=True)
    return seq[3](seq[2](x, frame, s), frame, s)


def _head(channels, m):
    return nn.Sequential(nn.Linear(channels, channels), nn.ReLU(True), nn.Linear(channels, m), nn.Softmax(dim=-1))


def _cloud_coords(x):
    """(N, 3) points, (N, 4) [batch, x, y, z] rows, or anything with `.coords` -> [(N_b, 3) int tensors] one per batch id."""
    c = x.coords if hasattr(x, "coords") else x
    if not torch.is_tensor(c):
        c = torch.as_tensor(np.asarray(c))
    if c.dim() != 2 or c.shape[1] not in (3, 4):
        raise ValueError("expected (N, 3) points or (N, 4) [batch, x, y, z] coordinates")
    if c.shape[1] == 3:
        return [c]
    b = c[:, 0]
    return [c[b == v, 1:] for v in torch.unique(b).tolist()]


class Network(nn.Module):
    """network_ue_4stage_conv.Network with the sparse convolutions on this library's gfx950 kernels."""

    def __init__(self, channels: int = 32, kernel_size: int = 5):
        super().__init__()
        if channels != 32:
            raise ValueError("the trainable network runs 32 channels (the MFMA path)")
        if kernel_size not in (3, 5, 7):
            raise ValueError("kernel_size must be 3, 5 or 7")
        C_, k = channels, kernel_size
        self.channels, self.kernel_size = C_, k
        self.prior_embedding = nn.Embedding(256, C_)
        self.prior_resnet = nn.Sequential(SparseConv3d(C_, k), _ReLU(), ResNet(C_, k), ResNet(C_, k))
        self.target_embedding = TargetEmbedding(C_)
        self.target_resnet = nn.Sequential(SparseConv3d(C_, k), _ReLU(), ResNet(C_, k), ResNet(C_, k))
        for s in range(4):
            setattr(self, f"spatial_conv_s{s}", nn.Sequential(SparseConv3d(C_, k), _ReLU(), SparseConv3d(C_, k)))
        self.pred_head_s0 = _head(C_, 2)
        self.pred_head_s1_emb = nn.Embedding(2, C_)
        self.pred_head_s1 = _head(C_, 2)
        self.pred_head_s2_emb = nn.Embedding(4, C_)
        self.pred_head_s2 = _head(C_, 4)
        self.pred_head_s3_emb = nn.Embedding(16, C_)
        self.pred_head_s3 = _head(C_, 16)
        self.fog = FOG()
        self.register_buffer("_perm", torch.tensor(PHYS_TO_LOGICAL, dtype=torch.long), persistent=False)

    def load_state_dict(self, state_dict, strict: bool = True):
        """Also takes numpy arrays (synth.synthetic_state_dict) and the "module." prefix of DataParallel checkpoints."""
        sd = {(k[7:] if k.startswith("module.") else k): (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))) for k, v in state_dict.items()}
        return super().load_state_dict(sd, strict)

    def cloud_bits(self, xyz: torch.Tensor) -> torch.Tensor:
        """Total ideal code length in bits of one cloud (N, 3) -- the reference's loss numerator."""
        dev = self._perm.device
        if dev.type != "cuda":
            raise RuntimeError("Network runs on the GPU: move it with .to('cuda')")
        frame = _Frame(xyz.to(dev), self.kernel_size)
        if frame.L < 2:   # no coded level: a zero that still reaches every parameter
            return sum(p.sum() for p in self.parameters()) * 0.0
        perm = self._perm
        occ = frame.occ.long()
        occP, occC = occ[: frame.nP], occ[frame.n0:]
        emb = nn.functional.embedding   # (its backward is a sorted segment sum; indexing's accumulate path serialises on tables this small)
        x = emb(occP, self.prior_embedding.weight[:, perm])
        x = _trunk(self.prior_resnet, x, frame, 0)
        x = x[frame.parent] + emb(frame.octant, self.target_embedding.target_res_embedding.weight[:, perm])   # FCG + TargetEmbedding
        X = _trunk(self.target_resnet, x, frame, 1)
        sym = ((occC >> 7) & 1, (occC >> 6) & 1, (occC >> 4) & 3, occC & 15)
        prev = (None, sym[0], sym[0] * 2 + sym[1], (sym[0] * 2 + sym[1]) * 4 + sym[2])
        bits = X.new_zeros(())
        for s in range(4):
            u = X if s == 0 else X + emb(prev[s], getattr(self, f"pred_head_s{s}_emb").weight[:, perm])
            sc = getattr(self, f"spatial_conv_s{s}")
            y = sc[2](sc[0](u, frame, 1, relu=True), frame, 1)
            hd = getattr(self, f"pred_head_s{s}")
            h = torch.relu(nn.functional.linear(y, hd[0].weight[:, perm], hd[0].bias))
            p = torch.softmax(hd[2](h), dim=-1).gather(1, sym[s].view(-1, 1))
            bits = bits + torch.clamp(-torch.log2(p + 1e-10), 0, 50).sum()
        return bits

    def forward(self, x):
        """bpp = sum of bits / sum of points over the clouds of `x` (one per batch id), one cloud after the other."""
        total, n = None, 0
        for c in _cloud_coords(x):
            b = self.cloud_bits(c)
            total = b if total is None else total + b
            n += int(c.shape[0])
        return total / max(n, 1)

