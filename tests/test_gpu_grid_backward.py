"""GPU checks of the hash-grid encoder's training path (gsge_forward_train, gsge_backward, grid_encode under autograd, GridEncoder /
mix_3D2D_encoding(differentiable=True) and the _gridencoder drop-in) against the float64 restatement of tests/grid_ref.py."""
import pytest
import torch

from tests import grid_ref as gr

pytestmark = pytest.mark.gpu

RES3 = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)      # HAC: 12 3-D levels, log2 13
RES2 = (130, 258, 514, 1026)                                       # HAC: 4 2-D levels, log2 15

CASES = [  # num_dim, n_features, resolutions, log2 table size
    (3, 4, RES3, 13), (3, 2, RES3, 13), (3, 1, RES3[:6], 13), (3, 8, RES3[:4], 13),
    (2, 4, RES2, 15), (2, 2, RES2, 15), (2, 1, RES2[:2], 15), (2, 8, RES2[:2], 15),
]


def _encoder(num_dim, n_features, res, log2_size, seed, **kw):
    from gauspcc_amd.gridencoder import GridEncoder

    torch.manual_seed(seed)
    enc = GridEncoder(num_dim=num_dim, n_features=n_features, resolutions_list=res, log2_hashmap_size=log2_size, ste_binary=False, **kw).cuda()
    enc.params.data.uniform_(-1, 1)
    return enc


def _points(n, num_dim, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, num_dim, generator=g)
    x[:4] = torch.tensor([[0.0] * num_dim, [1.0] * num_dim, [1.25] * num_dim, [-0.1] + [0.5] * (num_dim - 1)])
    # a cluster: the coarse levels' rows collect thousands of contributions (runs longer than a chunk)
    x[4:n // 4] = 0.5 + 0.02 * torch.randn(n // 4 - 4, num_dim, generator=g).clamp(-3, 3)
    return x


def _mode(mode, N, num_dim, nl):
    rb, bv, ml, nlc = 128, None, None, nl
    if mode == "binary_vxl":
        rb = 32
        bv = torch.rand(*([rb] * num_dim), generator=torch.Generator().manual_seed(3)) < 0.3
    if mode == "min_level_id":
        nlc = nl - 1
        ml = torch.randint(0, 2, (N,), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    return rb, bv, ml, nlc


def _device(enc, x, grad, bv, ml, nlc, want_inputs=True):
    """grid_encode under autograd: (outputs (N, nlc F), grad_embeddings, grad_inputs)."""
    from gauspcc_amd.gridencoder import grid_encode

    xi = x.cuda().requires_grad_(want_inputs)
    emb = enc.params.detach().clone().requires_grad_(True)
    lo = 0 if ml is None else ml.cuda()
    y = grid_encode(xi, emb, enc.offsets_list, enc.resolutions_list, want_inputs, lo, nlc, None if bv is None else bv.cuda())
    y.backward(grad.permute(1, 0, 2).reshape(x.shape[0], -1).cuda())
    return y.detach(), emb.grad, xi.grad if want_inputs else None


def _close(got, ref, scale, tol=1e-5):
    err = (got.double().cpu() - ref).abs()
    bound = tol * scale + 1e-12
    assert torch.all(err <= bound), f"max excess {float((err - bound).max()):.3g}, max err {float(err.max()):.3g}"


@pytest.mark.parametrize("num_dim,n_features,res,log2_size", CASES)
@pytest.mark.parametrize("mode", ["plain", "binary_vxl", "min_level_id"])
def test_gradients_match_restatement(num_dim, n_features, res, log2_size, mode):
    N = 6000
    enc = _encoder(num_dim, n_features, res, log2_size, seed=num_dim * 10 + n_features)
    x = _points(N, num_dim, seed=n_features)
    rb, bv, ml, nlc = _mode(mode, N, num_dim, len(res))
    grad = torch.randn(nlc, N, n_features, generator=torch.Generator().manual_seed(7))
    y, ge, gi = _device(enc, x, grad, bv, ml, nlc)
    emb = enc.params.detach().cpu()
    off, rs = enc.offsets_list.cpu(), enc.resolutions_list.cpu()
    ref_ge, abs_ge = gr.grad_embeddings(x, emb, off, rs, nlc, grad, rb=rb, binary_vxl=bv, min_level_id=ml)
    _close(ge, ref_ge, abs_ge)
    assert torch.count_nonzero(ge) > 0
    dydx = gr.dy_dx(x, emb, off, rs, nlc, min_level_id=ml)
    ref_gi, abs_gi = gr.grad_inputs(grad, dydx, gr.dy_dx(x, emb, off, rs, nlc, min_level_id=ml, magnitude=True))
    _close(gi, ref_gi, abs_gi)
    assert torch.all(gi[2:4].cpu() == 0)                # out of range: no input gradient
    # forward under autograd: the bits of the inference path (gsge_forward)
    with torch.no_grad():
        from gauspcc_amd.gridencoder import grid_encode

        y0 = grid_encode(x.cuda(), enc.params.detach(), enc.offsets_list, enc.resolutions_list, False, 0 if ml is None else ml.cuda(), nlc,
                         None if bv is None else bv.cuda())
    assert torch.equal(y, y0)


@pytest.mark.parametrize("num_dim,n_features,res,log2_size", CASES)
@pytest.mark.parametrize("mode", ["plain", "min_level_id"])
def test_forward_train_outputs_and_dy_dx(num_dim, n_features, res, log2_size, mode):
    from gauspcc_amd import _gridencoder

    N = 3000
    enc = _encoder(num_dim, n_features, res, log2_size, seed=5)
    x = _points(N, num_dim, seed=6)
    rb, bv, ml, nlc = _mode(mode, N, num_dim, len(res))
    off = enc.offsets_list.int() if ml is not None else enc.offsets_list[:nlc + 1].int().contiguous()
    rs = enc.resolutions_list.int() if ml is not None else enc.resolutions_list[:nlc].int().contiguous()
    xc, emb = x.cuda(), enc.params.detach().contiguous()
    mlc = None if ml is None else ml.cuda()
    out0 = torch.empty(nlc, N, n_features, device="cuda")
    out1 = torch.full((nlc, N, n_features), 7.0, device="cuda")
    dydx = torch.full((N, nlc * num_dim * n_features), 7.0, device="cuda")
    _gridencoder.grid_encode_forward(xc, emb, off, rs, out0, N, num_dim, n_features, nlc, 0, rb, 0, None, None, mlc)
    _gridencoder.grid_encode_forward(xc, emb, off, rs, out1, N, num_dim, n_features, nlc, 0, rb, 0, dydx, None, mlc)
    assert torch.equal(out0, out1)
    ref = gr.dy_dx(x, emb.cpu(), enc.offsets_list.cpu(), enc.resolutions_list.cpu(), nlc, min_level_id=ml)
    mag = gr.dy_dx(x, emb.cpu(), enc.offsets_list.cpu(), enc.resolutions_list.cpu(), nlc, min_level_id=ml, magnitude=True)
    _close(dydx.view(N, nlc, num_dim, n_features), ref, mag)


@pytest.mark.parametrize("n_features", [2, 4])
def test_differentiable_encoder_forward_is_bit_identical(n_features):
    from gauspcc_amd.gridencoder import mix_3D2D_encoding

    kw = dict(n_features=n_features, resolutions_list=RES3, log2_hashmap_size=13, resolutions_list_2D=RES2, log2_hashmap_size_2D=15,
              ste_binary=True, ste_multistep=False, add_noise=False, Q=1)
    torch.manual_seed(1)
    a = mix_3D2D_encoding(**kw).cuda()
    b = mix_3D2D_encoding(**kw, differentiable=True).cuda()
    b.load_state_dict(a.state_dict())
    for p in a.parameters():
        p.data.uniform_(-1, 1)
    b.load_state_dict(a.state_dict())
    assert not a.differentiable and b.differentiable and b.encoding_xyz.differentiable
    x = torch.rand(5000, 3, device="cuda").requires_grad_(True)
    ya = a(x)
    yb = b(x)
    assert not ya.requires_grad and yb.requires_grad
    assert torch.equal(ya, yb.detach())
    yb.sum().backward()
    assert x.grad is not None and all(p.grad is not None for p in b.parameters())
    for ste in ("ste_multistep", "add_noise_test"):     # the STE_multistep branch too
        kw2 = dict(kw, ste_binary=False, ste_multistep=ste == "ste_multistep", add_noise=ste != "ste_multistep", Q=0.3)
        a2, b2 = mix_3D2D_encoding(**kw2).cuda(), mix_3D2D_encoding(**kw2, differentiable=True).cuda()
        b2.load_state_dict(a.state_dict())
        a2.load_state_dict(a.state_dict())
        e2 = b2.encoding_xyz
        assert torch.equal(a2.encoding_xyz(x, test_phase=True), e2(x, test_phase=True).detach())


def test_backward_is_deterministic_across_runs_and_streams():
    from gauspcc_amd import _gridencoder

    N, F = 200000, 4
    enc = _encoder(3, F, RES3, 13, seed=2)
    x = _points(N, 3, seed=3).cuda()
    grad = torch.randn(len(RES3), N, F, device="cuda")
    off, rs = enc.offsets_list.int(), enc.resolutions_list.int()
    emb = enc.params.detach().contiguous()

    def run(stream):
        with torch.cuda.stream(stream):
            ge = torch.zeros_like(emb)
            gi = torch.empty(N, 3, device="cuda")
            _gridencoder.grid_encode_backward(grad, x, emb, off, rs, ge, N, 3, F, len(RES3), 0, 128, torch.empty(1, device="cuda"), gi, None, None)
        return ge, gi

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    a = run(torch.cuda.current_stream())
    b = run(torch.cuda.current_stream())
    c = run(s1)
    d = run(s2)
    torch.cuda.synchronize()
    for r in (b, c, d):
        assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1])
    assert torch.count_nonzero(a[0]) > 0


_DROP_IN = {}


class _RefGridEncode(torch.autograd.Function):
    """The reference's _grid_encode (encodings.py:92-218) on the drop-in, with its argument order and in-place tensors."""

    @staticmethod
    def forward(ctx, inputs, embeddings, offsets_list, resolutions_list, calc_grad_inputs=False, min_level_id=None, n_levels_calc=1, binary_vxl=None, PV=0):
        from gauspcc_amd import _gridencoder as _backend

        inputs = inputs.contiguous()
        Rb = 128
        if binary_vxl is not None:
            binary_vxl = binary_vxl.contiguous()
            Rb = binary_vxl.shape[-1]
        N, num_dim = inputs.shape
        n_features = embeddings.shape[1]
        outputs = torch.empty(n_levels_calc, N, n_features, device=inputs.device, dtype=embeddings.dtype)
        dy_dx = torch.empty(N, n_levels_calc * num_dim * n_features, device=inputs.device) if calc_grad_inputs else None
        if isinstance(min_level_id, int):
            lo, hi = min_level_id, min_level_id + n_levels_calc
            off, res, ml = offsets_list[lo:hi + 1], resolutions_list[lo:hi], None
        else:
            off, res, ml = offsets_list, resolutions_list, min_level_id
        _backend.grid_encode_forward(inputs, embeddings, off, res, outputs, N, num_dim, n_features, n_levels_calc, 0, Rb, PV, dy_dx, binary_vxl, ml)
        ctx.save_for_backward(inputs, embeddings, dy_dx)
        ctx.rest = (off, res, ml, binary_vxl, N, num_dim, n_features, n_levels_calc, Rb)
        return outputs.permute(1, 0, 2).reshape(N, n_levels_calc * n_features)

    @staticmethod
    def backward(ctx, grad):
        from gauspcc_amd import _gridencoder as _backend

        inputs, embeddings, dy_dx = ctx.saved_tensors
        off, res, ml, binary_vxl, N, num_dim, n_features, n_levels_calc, Rb = ctx.rest
        grad = grad.view(N, n_levels_calc, n_features).permute(1, 0, 2).contiguous()
        grad_embeddings = _DROP_IN["seed"].clone()
        grad_inputs = torch.zeros_like(inputs) if dy_dx is not None else None
        _backend.grid_encode_backward(grad, inputs, embeddings, off, res, grad_embeddings, N, num_dim, n_features, n_levels_calc, 0, Rb, dy_dx,
                                      grad_inputs, binary_vxl, ml)
        _DROP_IN["filled"] = grad_embeddings
        return grad_inputs, grad_embeddings, None, None, None, None, None, None, None


@pytest.mark.parametrize("ml_kind", ["int", "tensor"])
def test_gridencoder_drop_in(ml_kind):
    from gauspcc_amd import _gridencoder

    N, F = 4000, 4
    enc = _encoder(3, F, RES3, 13, seed=11)
    x = _points(N, 3, seed=12)
    off32, res32 = enc.offsets_list.int(), enc.resolutions_list.int()
    if ml_kind == "int":
        ml, nlc, ml_ref = 2, 8, torch.full((N,), 2, dtype=torch.int32)
    else:
        ml_ref = torch.randint(0, 3, (N,), dtype=torch.int32)
        ml, nlc = ml_ref.cuda(), 8
    xi = x.cuda().requires_grad_(True)
    emb = enc.params.detach().clone().requires_grad_(True)
    seed = torch.randn_like(emb)                       # the backward ADDS into grad_embeddings
    _DROP_IN["seed"] = seed
    y = _RefGridEncode.apply(xi, emb, off32, res32, True, ml, nlc, None, 0)
    g = torch.randn(N, nlc * F, device="cuda")
    y.backward(g)
    gl = g.view(N, nlc, F).permute(1, 0, 2).cpu()
    ref_ge, abs_ge = gr.grad_embeddings(x, emb.detach().cpu(), off32.cpu(), res32.cpu(), nlc, gl, min_level_id=ml_ref)
    filled, sd = _DROP_IN["filled"].cpu(), seed.cpu().double()
    assert torch.equal(filled[abs_ge == 0], seed.cpu()[abs_ge == 0])           # rows without contributions: untouched
    _close(filled, sd + ref_ge, abs_ge + (sd + ref_ge).abs() * 2e-2)          # + one float32 rounding of the final add (2^-23 = 1e-5 x 1.2e-2)
    assert torch.equal(emb.grad, _DROP_IN["filled"])
    dargs = (x, emb.detach().cpu(), off32.cpu(), res32.cpu(), nlc)
    ref_gi, abs_gi = gr.grad_inputs(gl, gr.dy_dx(*dargs, min_level_id=ml_ref), gr.dy_dx(*dargs, min_level_id=ml_ref, magnitude=True))
    _close(xi.grad, ref_gi, abs_gi)
    # what the extension refuses
    out = torch.empty(nlc, N, F, device="cuda")
    e = emb.detach()
    args = (off32, res32, out, N, 3, F, nlc, 0, 128, 0, None, None, None)
    with pytest.raises((TypeError, ValueError)):
        _gridencoder.grid_encode_forward(x.cuda(), e.half(), *args)
    with pytest.raises((TypeError, ValueError)):
        _gridencoder.grid_encode_forward(x.cuda().t().contiguous().t(), e, *args)
    with pytest.raises((TypeError, ValueError)):
        _gridencoder.grid_encode_forward(x, e, *args)                         # a CPU tensor
    with pytest.raises((TypeError, ValueError)):
        ge_nc = torch.zeros(e.shape[1], e.shape[0], device="cuda").t()
        _gridencoder.grid_encode_backward(out, x.cuda(), e, off32, res32, ge_nc, N, 3, F, nlc, 0, 128, None, None, None, None)
    # binary_vxl as bool or uint8
    bv = torch.rand(32, 32, 32, device="cuda") < 0.3
    o1, o2 = torch.empty_like(out), torch.empty_like(out)
    a8 = (off32[:nlc + 1].contiguous(), res32[:nlc].contiguous())
    _gridencoder.grid_encode_forward(x.cuda(), e, *a8, o1, N, 3, F, nlc, 0, 32, 0, None, bv, None)
    _gridencoder.grid_encode_forward(x.cuda(), e, *a8, o2, N, 3, F, nlc, 0, 32, 0, None, bv.to(torch.uint8), None)
    assert torch.equal(o1, o2)


def test_ste_binary_gradient_mask():
    from gauspcc_amd.gridencoder import STE_binary

    p = torch.tensor([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5], device="cuda", requires_grad=True)
    y = STE_binary.apply(p)
    assert torch.equal(y.detach().cpu(), torch.tensor([-1.0, -1, -1, 1, 1, 1, 1]))
    y.backward(torch.full_like(p, 3.0))
    assert torch.equal(p.grad.cpu(), torch.tensor([0.0, 3, 3, 3, 3, 3, 0]))


def test_it_trains_hac_rate_term():
    """mix_3D2D_encoding(differentiable=True) + a linear head fit the Gaussian bits of a fixed target (HAC's rate term)."""
    from gauspcc_amd.gridencoder import mix_3D2D_encoding

    torch.manual_seed(0)
    enc = mix_3D2D_encoding(n_features=4, resolutions_list=RES3, log2_hashmap_size=13, resolutions_list_2D=RES2, log2_hashmap_size_2D=15,
                            ste_binary=True, ste_multistep=False, add_noise=False, Q=1, differentiable=True).cuda()
    head = torch.nn.Linear(enc.output_dim, 2).cuda()
    N = 20000
    x = torch.rand(N, 3, device="cuda")
    target = torch.sin(6 * x[:, :1]) * 2 + torch.cos(5 * x[:, 1:2]) + x[:, 2:3]       # a smooth field the grid can carry

    def bits():
        mean, s = head(enc(x)).chunk(2, -1)
        scale = torch.nn.functional.softplus(s) + 1e-3
        d = torch.distributions.Normal(mean, scale)
        p = (d.cdf(target + 0.5) - d.cdf(target - 0.5)).clamp_min(1e-9)
        return -torch.log2(p).mean()

    opt = torch.optim.Adam([{"params": enc.parameters(), "lr": 5e-3}, {"params": head.parameters(), "lr": 5e-3}])
    first = None
    for _ in range(200):
        opt.zero_grad()
        loss = bits()
        loss.backward()
        for p in enc.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all()
        opt.step()
        first = first if first is not None else float(loss.detach())
    last = float(bits())
    assert last < first / 3, (first, last)


def test_hac_call_shape_on_synth_model():
    """On the synth.py model: calc_interp_feat(anchor) with the anchor requiring grad, mlp_grid, the 5 % choose_idx subset, .backward()."""
    from gauspcc_amd.synth import SyntheticGaussianModel

    m = SyntheticGaussianModel(30000, seed=2, device="cuda:0")
    mix = m.encoding_xyz
    encs = (mix.encoding_xyz, mix.encoding_xy, mix.encoding_xz, mix.encoding_yz)
    for e in (mix,) + encs:
        e.differentiable = True
    anchor = m._anchor.clone().requires_grad_(True)
    feat = m.calc_interp_feat(anchor)
    torch.manual_seed(5)
    choose = torch.rand(anchor.shape[0], device="cuda") <= 0.05
    out = m.get_grid_mlp(feat[choose])
    w = torch.randn_like(out)
    (out * w).sum().backward()
    # the same chain with the encoders replaced by the float64 restatement: d loss / d feat from torch, then the restatement's backward
    f2 = feat.detach().requires_grad_(True)
    (m.get_grid_mlp(f2[choose]) * w).sum().backward()
    span = (m.x_bound_max - m.x_bound_min).cpu().double()
    xn = ((anchor.detach() - m.x_bound_min) / (m.x_bound_max - m.x_bound_min)).cpu()
    ga, aa = torch.zeros_like(xn, dtype=torch.float64), torch.zeros_like(xn, dtype=torch.float64)
    col = 0
    for e, dims in zip(encs, ([0, 1, 2], [0, 1], [0, 2], [1, 2])):
        L, F = e.n_levels, e.n_features
        gl = f2.grad[:, col:col + L * F].reshape(-1, L, F).permute(1, 0, 2).cpu()
        col += L * F
        p = e.params.detach().cpu()
        emb = torch.where(p >= 0, 1.0, -1.0)
        x = xn[:, dims].contiguous()
        ref_ge, abs_ge = gr.grad_embeddings(x, emb, e.offsets_list.cpu(), e.resolutions_list.cpu(), L, gl)
        _close(e.params.grad, ref_ge * ((p >= -1) & (p <= 1)), abs_ge)      # STE_binary: zero outside [-1, 1]
        dargs = (x, emb, e.offsets_list.cpu(), e.resolutions_list.cpu(), L)
        gx, ax = gr.grad_inputs(gl, gr.dy_dx(*dargs), gr.dy_dx(*dargs, magnitude=True))
        ga[:, dims] += gx
        aa[:, dims] += ax
    _close(anchor.grad, ga / span, aa / span)
    assert torch.count_nonzero(anchor.grad) > 0
