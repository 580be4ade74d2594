"""The GausPcgc training path on gfx950 (gauspcc_amd.pcgc_net, gpcc_train_*): the training convolution against the codec's, its two
gradients against float64, the whole loss and its 39 gradients against tests/pcgc_ref.py and the encoder's ideal bits, determinism,
the frame's lifetime, edge cases, and a short training run whose checkpoint the codec takes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gauspcc_amd import _lib, runtime
from gauspcc_amd.model import tensor_table
from gauspcc_amd.pcgc_net import PHYS_TO_LOGICAL, Network, _Frame, sparse_conv
from gauspcc_amd.synth import peaky_state_dict, stage_symbol_frequencies, synthetic_cloud, synthetic_state_dict

from . import gpu_helpers as gh
from . import pcgc_ref as ref

pytestmark = pytest.mark.gpu
PERM = torch.tensor(PHYS_TO_LOGICAL)
INV = torch.argsort(PERM)   # logical -> physical column


def _net(sd, k):
    net = Network(32, k).cuda()
    net.load_state_dict(sd)
    return net


def _level_rows(frame, d):
    """(first row in the target set, rows) of stored level d >= 1."""
    base = sum(frame.level_nodes[1:d])
    return base, frame.level_nodes[d]


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("res_relu", [False, True])
def test_training_conv_is_bit_identical_to_the_codec_conv(k, res_relu):
    pts = synthetic_cloud(30000, seed=21)
    frame = _Frame(torch.tensor(pts, device="cuda"), k)
    g = torch.Generator().manual_seed(k)
    x = torch.randn(frame.nC, 32, generator=g)
    r = torch.randn(frame.nC, 32, generator=g) if res_relu else None
    w = (torch.randn(k ** 3, 32, 32, generator=g) * 0.1)
    out = sparse_conv(x[:, PERM].cuda(), w.cuda(), frame, 1, None if r is None else r[:, PERM].cuda(), res_relu)[:, INV].cpu().numpy()
    for d in (frame.L - 1, frame.L - 2):
        b, n = _level_rows(frame, d)
        coords = frame.coords[frame.n0 + b: frame.n0 + b + n].cpu().numpy()
        perm = gh.sort_zyx(coords)
        want, _ = gh.conv3d(coords[perm], x[b: b + n].numpy()[perm], w.numpy(), k, None if r is None else r[b: b + n].numpy()[perm], res_relu)
        assert np.array_equal(out[b: b + n][perm], want)


def test_conv_gradients_against_float64_and_the_adjoint():
    pts = synthetic_cloud(20000, seed=4)
    k = 3
    frame = _Frame(torch.tensor(pts, device="cuda"), k)
    d = frame.L - 1
    b, n = _level_rows(frame, d)
    coords = frame.coords[frame.n0 + b: frame.n0 + b + n].cpu().numpy()
    nb = ref.neighbours(coords.astype(np.int64), k)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(frame.nC, 32, generator=g)
    dy = torch.randn(frame.nC, 32, generator=g)
    w = torch.randn(k ** 3, 32, 32, generator=g) * 0.1
    xc = x[:, PERM].cuda().requires_grad_(True)
    wc = w.cuda().requires_grad_(True)
    y = sparse_conv(xc, wc, frame, 1)
    (y * dy[:, PERM].cuda()).sum().backward()
    dx, dw = xc.grad[:, INV].cpu().double(), wc.grad.cpu().double()
    x64 = x[b: b + n].double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    (ref.conv(x64, nb, w64) * dy[b: b + n].double()).sum().backward()
    assert torch.linalg.norm(dx[b: b + n] - x64.grad) <= 1e-5 * torch.linalg.norm(x64.grad)
    # the weight gradient sums over every level of the set: the float64 one of all levels
    w64b = w.double().requires_grad_(True)
    tot = 0.0
    for dd in range(1, frame.L):
        bb, nn_ = _level_rows(frame, dd)
        cc = frame.coords[frame.n0 + bb: frame.n0 + bb + nn_].cpu().numpy().astype(np.int64)
        tot = tot + (ref.conv(x[bb: bb + nn_].double(), ref.neighbours(cc, k), w64b) * dy[bb: bb + nn_].double()).sum()
    tot.backward()
    err = float(torch.linalg.norm(dw - w64b.grad) / torch.linalg.norm(w64b.grad))
    print(f"wgrad relative error {err:.2e}")
    assert err <= 1e-5
    lhs = float((y.detach()[:, INV].cpu().double() * dy.double()).sum())
    rhs = float((x.double() * xc.grad[:, INV].cpu().double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + 1e-30) * 10 or abs(lhs - rhs) <= 1e-5 * float(torch.linalg.norm(x) * torch.linalg.norm(dy))


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("peaky", [False, True])
def test_network_loss_and_gradients(k, peaky):
    pts = synthetic_cloud(8000, seed=13)
    sd = (peaky_state_dict if peaky else synthetic_state_dict)(32, k, seed=5)
    net = _net(sd, k)
    loss = net(torch.tensor(pts))
    loss.backward()
    bits = float(loss.detach()) * len(pts)
    _, st = gh.encode(runtime.Model(sd, 32, k), pts, 11, ideal_bits=True)
    assert abs(bits - st.ideal_bits) <= 1e-5 * st.ideal_bits
    p64 = ref.params(sd, requires_grad=True)
    tb = ref.total_bits(p64, pts, k)
    assert abs(bits - float(tb)) <= 1e-5 * float(tb)
    tb.backward()
    worst = 0.0
    for name, prm in net.named_parameters():
        want = p64[name].grad
        got = prm.grad.cpu().double() * len(pts)   # the loss is bits / N
        e = float(torch.linalg.norm(got - want) / max(float(torch.linalg.norm(want)), 1e-30))
        worst = max(worst, e)
        assert e <= 1e-4, name
    print(f"k {k} peaky {peaky}: bits {bits:.2f}, worst relative gradient error {worst:.2e}")


def _grads(net, pts):
    net.zero_grad()
    net(pts).backward()
    return [p.grad.clone() for p in net.parameters()]


def test_gradients_are_bitwise_reproducible_across_runs_and_streams():
    pts = torch.tensor(synthetic_cloud(20000, seed=8))
    net = _net(synthetic_state_dict(32, 5, seed=2), 5)
    a = _grads(net, pts)
    b = _grads(net, pts)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = _grads(net, pts)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


def test_an_encode_between_forward_and_backward_changes_nothing():
    pts = synthetic_cloud(20000, seed=9)
    sd = synthetic_state_dict(32, 3, seed=4)
    net = _net(sd, 3)
    a = _grads(net, torch.tensor(pts))
    net.zero_grad()
    loss = net(torch.tensor(pts))
    gh.encode(runtime.Model(sd, 32, 3), synthetic_cloud(50000, seed=1), 11)
    loss.backward()
    assert all(torch.equal(x, p.grad) for x, p in zip(a, net.parameters()))


def test_edge_cases():
    net = _net(synthetic_state_dict(32, 3, seed=4), 3)
    neg = synthetic_cloud(5000, seed=2, negative=True)
    p64 = ref.params(synthetic_state_dict(32, 3, seed=4))
    assert abs(float(net(torch.tensor(neg))) * len(neg) - float(ref.total_bits(p64, neg, 3))) <= 1e-5 * float(ref.total_bits(p64, neg, 3))
    one = (2 * np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing='ij'), -1).reshape(-1, 3)).astype(np.int32)   # 27 <- 125 nodes: one coded level
    assert len(ref.build_levels(one)) == 2
    assert abs(float(net(torch.tensor(one))) * len(one) - float(ref.total_bits(p64, one, 3))) <= 1e-5 * float(ref.total_bits(p64, one, 3))
    few = np.arange(30 * 3, dtype=np.int32).reshape(30, 3)   # no coded level
    net.zero_grad()
    z = net(torch.tensor(few))
    z.backward()
    assert float(z) == 0.0 and all(p.grad is not None and not p.grad.any() for p in net.parameters())
    dup = np.concatenate([neg[:100], neg[:1]])
    with pytest.raises(_lib.GpccError):
        net(torch.tensor(dup))
    w = torch.zeros(27 * 16 * 16, device="cuda")
    with pytest.raises(_lib.GpccError):
        _lib.check(_lib.lib().gpcc_train_weights(runtime.context(0), w.data_ptr(), 16, 3, 0, w.data_ptr(), runtime.stream_ptr(0)))


def _context_free_bits(pts):
    fr = stage_symbol_frequencies(pts)
    total = 0.0
    for lv in ref.build_levels(pts)[1:]:
        o = lv[1]
        for s, sym in enumerate((o >> 7 & 1, o >> 6 & 1, o >> 4 & 3, o & 15)):
            total += float(-np.log2(fr[s][sym]).sum())
    return total


def test_training_beats_the_context_free_bound_and_the_codec_takes_the_checkpoint(tmp_path):
    from gauspcc_amd.pcc_utils import compress_point_cloud, decompress_point_cloud

    pts = synthetic_cloud(20000, seed=31)
    bound = _context_free_bits(pts) / len(pts)
    torch.manual_seed(0)
    net = Network(32, 3).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=3e-3)
    x = torch.tensor(pts)
    curve = []
    for step in range(300):
        opt.zero_grad()
        loss = net(x)
        loss.backward()
        opt.step()
        curve.append(float(loss))
        if step >= 20 and float(loss) < 0.97 * bound:
            break
    print(f"context-free bound {bound:.4f} bpp; loss {curve[0]:.3f} -> {curve[-1]:.4f} in {len(curve)} steps")
    assert curve[-1] < bound
    ckpt = tmp_path / "net.pt"
    torch.save(net.state_dict(), ckpt)
    with torch.no_grad():
        loss = float(net(x))
    for chunk in (0, 11):
        bin_path = str(tmp_path / f"c{chunk}.bin")
        compress_point_cloud(pts, str(ckpt), bin_path, 32, 3, chunk_log2=chunk)
        dec = decompress_point_cloud(bin_path, str(ckpt), None, 32, 3)["point_cloud"].cpu().numpy()
        assert np.array_equal(np.unique(np.round(dec).astype(np.int64), axis=0), np.unique(pts.astype(np.int64), axis=0))
        if chunk == 0:
            payload = os.path.getsize(bin_path)
            print(f"payload {payload} B vs loss x N / 8 = {loss * len(pts) / 8:.0f} B")
            assert abs(payload - loss * len(pts) / 8) <= 0.05 * loss * len(pts) / 8 + 64


def test_cli_train_leaves_a_loadable_checkpoint(tmp_path):
    pts = synthetic_cloud(6000, seed=3)
    ply = tmp_path / "a.ply"
    with open(ply, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        np.savetxt(f, pts, fmt="%d")
    out = tmp_path / "m"
    subprocess.run([sys.executable, "-m", "gauspcc_amd.cli.train", "--training_data", str(ply), "--model_save_folder", str(out), "--max_steps", "5",
                    "--log_interval", "1", "--val_interval", "5", "--is_data_pre_quantized", "True", "--kernel_size", "3"], check=True, timeout=600)
    sd = torch.load(out / "final_model_ue_4stage_conv.pt")
    assert len(tensor_table(sd, 32, 3)) == 39 and (out / "ckpt_ue_4stage_conv.pt").exists()
