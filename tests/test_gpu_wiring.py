"""The HIP codec, the plugin API and the HIP training path against what the reference's own Python computed
(tests/golden/wiring_*.npz; tests/golden/make_wiring.py, tests/test_wiring_cpu.py): the encoder's ideal bits and level structure, the
points compress_point_cloud -> decompress_point_cloud return, and pcgc_net.Network's bpp and gradient.  Reads only tests/golden/."""
import numpy as np
import pytest
import torch

from gauspcc_amd import runtime
from gauspcc_amd.pcgc_net import Network
from gauspcc_amd.synth import CONV_KEYS

from . import gpu_helpers as gh
from . import wiring

pytestmark = pytest.mark.gpu


def _ideal_bits(c, sd):
    _, st = gh.encode(runtime.Model(sd, 32, c.k), c.points, 11, posq=c.posQ, ideal_bits=True)
    return st


@pytest.mark.parametrize("name", wiring.CASES)
def test_codec_ideal_bits_and_levels(name):
    c = wiring.case(name)
    st = _ideal_bits(c, c.sd)
    rel = abs(st.ideal_bits - c.bits_f64) / c.bits_f64
    print(f"{name}: device ideal bits {st.ideal_bits:.6f} vs reference float64 {c.bits_f64:.6f}: relative difference {rel:.2e}")
    assert rel <= 1e-5
    base = int(np.frombuffer(c.z["bin"].tobytes()[2:6], np.int32)[0])
    assert st.num_levels == c.levels + 1 and st.num_points == len(c.points)
    assert [int(st.level_nodes[d]) for d in range(st.num_levels)] == [base] + [len(c.xyz(d)) for d in range(c.levels)]


@pytest.mark.parametrize("name", wiring.CASES)
@pytest.mark.parametrize("pre_quantized", [True, False])
def test_plugin_api_returns_the_reference_points(tmp_path, name, pre_quantized):
    from gauspcc_amd.pcc_utils import compress_point_cloud, decompress_point_cloud

    c = wiring.case(name)
    ckpt = str(tmp_path / "ckpt_ue_4stage_conv.pt")
    torch.save({k: torch.tensor(v) for k, v in c.sd.items()}, ckpt)
    res = compress_point_cloud(c.points, ckpt, str(tmp_path / "a.bin"), channels=32, kernel_size=c.k, posQ=c.posQ)
    assert res["num_points"] == int(c.z["compress_num_points"])
    dec = decompress_point_cloud(str(tmp_path / "a.bin"), ckpt, None, channels=32, kernel_size=c.k, is_data_pre_quantized=pre_quantized)
    tag = "preq" if pre_quantized else "raw"
    pc = dec["point_cloud"]
    assert str(pc.dtype) == str(c.z[f"dec_{tag}_dtype"]) and dec["num_points"] == int(c.z[f"dec_{tag}_num_points"])
    assert np.array_equal(wiring.sorted_rows(pc.cpu().numpy()), wiring.sorted_rows(c.z[f"dec_{tag}"]))


def _bpp(c, sd):
    net = Network(32, c.k).cuda()
    net.load_state_dict(sd)
    pts = torch.tensor(c.points)
    x = torch.cat((pts[:, 0:1] * 0, pts), dim=-1).int()      # (N, 4) [batch, x, y, z], the reference's input (pcc_utils.py:73)
    return net, net(x)


@pytest.mark.parametrize("name", wiring.CASES)
def test_training_bpp(name):
    c = wiring.case(name)
    _, bpp = _bpp(c, c.sd)
    want = float(c.z["bpp_f64"])
    got = float(bpp.detach())
    rel = abs(got - want) / want
    print(f"{name}: device bpp {got:.7f} vs reference float64 {want:.9f}: relative difference {rel:.2e}")
    assert rel <= 1e-5


def test_training_gradient():
    """Every full tensor, the sampled entries of every convolution kernel, and the kernels' gradient sums and norms: relative error at most
    1e-4 per tensor (test_gpu_pcgc_train.py's criterion).  A sum may cancel to far below its terms, so its error is taken relative to
    the larger of |sum| and the tensor's norm.  The gradient is that of bpp = bits / N: no factor N on either side."""
    c = wiring.case(wiring.GRAD_CASE)
    g = c.grad()
    net, bpp = _bpp(c, c.sd)
    bpp.backward()
    worst, seen = 0.0, 0
    for key, prm in net.named_parameters():
        got = prm.grad.cpu().double().numpy()
        if key in CONV_KEYS:
            want = g[f"val/{key}"]
            norm = float(g[f"norm/{key}"])
            e = float(np.linalg.norm(got.reshape(-1)[g[f"pos/{key}"].astype(np.int64)] - want) / np.linalg.norm(want))
            e = max(e, abs(float(got.sum()) - float(g[f"sum/{key}"])) / max(abs(float(g[f"sum/{key}"])), norm),
                    abs(float(np.sqrt((got * got).sum())) - norm) / norm)
        else:
            want = g[f"full/{key}"]
            e = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        worst, seen = max(worst, e), seen + 1
        assert e <= 1e-4, (key, e)
    assert seen == 39 == sum(k.startswith(("full/", "pos/")) for k in g)
    print(f"{c.name}: device gradient vs reference float64, worst relative error over {seen} tensors {worst:.2e}")


def test_a_mutation_breaks_the_ideal_bits_bound():
    """swap_target_embedding_rows_1_2 (the x and y bits of the TargetEmbedding index exchanged) on the device: outside the bound the unmutated codec
    meets.  (With the mutation removed the difference is the 9e-9 of test_codec_ideal_bits_and_levels and this test fails.)"""
    c = wiring.case(wiring.GRAD_CASE)
    st = _ideal_bits(c, wiring.gen.mutate(c.sd, "swap_target_embedding_rows_1_2"))
    rel = abs(st.ideal_bits - c.bits_f64) / c.bits_f64
    print(f"{c.name}: mutated device ideal bits {st.ideal_bits:.6f} vs reference float64 {c.bits_f64:.6f}: relative difference {rel:.2e}")
    assert rel > 100 * 1e-5
