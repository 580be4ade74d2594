"""The device's attribute coders and generate_neural_gaussians against what the reference's own Python computed and wrote
(tests/golden/attr_b_*.npz, ng_*.npz; tests/golden/make_attr_pins.py; the CPU half is tests/test_attr_pins_cpu.py).

`.b` files, per case: the device's CDF table within 2e-7 (two erfc libraries, tests/test_gpu_attributes.py) of the table the reference's
Python handed to its coder; the device coder on THAT table gives the reference's chunk counts and payload exactly and decodes them to the
reference's symbols; the wrappers write the reference's file names with the reference's min / max / chunk-table length, return the bit
count of the bytes they wrote, and their decoders return the reference's decoded tensor (torch.equal, dtype, shape) from their own files;
Bernoulli files equal the reference's byte for byte (the row is exact); the `_slices` coders with the case's chunk bounds likewise.

NOT asserted: whole-file byte equality of the fused Gaussian and mixture encoders with the reference-written files, and the fused decoders
on the reference-written files.  The coder integerises rint(cdf * (65536 - Lp + 1)): a one-ulp erfc difference between ocml and glibc moves
an integer in a fraction of a percent of the entries -- an arithmetic difference of two libraries, not wiring.  The coder itself is compared
on identical tables (test_device_coder_on_the_reference_table).  The factorized table is torch's own sigmoid and cumsum on either side and
is not compared here either.

Neural Gaussians, per case: the same number of Gaussians in the same order -- every row's position is nearest to the row of the
expectation with the same index, so the kept candidate indices are the stored ones; no pairing heuristic, no borderline allowance: the
inputs have none (tests/attr_pin_cases.py) -- and every output within max(project tolerance, 4 x the reference's own float32-vs-float64
difference) of the reference's float64 run (the expectation is stored as float32: half an ulp, 1e-7 at most here, against 2e-5).
"""
import numpy as np
import pytest

from . import attr_pin_cases as apc
from . import attr_pins as pins
from . import b_assembly as ba

pytestmark = pytest.mark.gpu

GAUSS_MIX = [i for i in pins.B_IDS if apc.b_case(i[1])["kind"] in ("gauss", "mix")]
WITH_TABLE = [i for i in GAUSS_MIX if apc.b_case(i[1])["n"] <= apc.TABLE_ROWS_MAX]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch


def _args(torch, c, f=None):
    """The case's (or one file's) inputs on the device as the wrappers take them."""
    arrays = c.arrays if f is None else {k: v[f.lo:f.hi] for k, v in c.arrays.items()}
    return apc.b_torch_args(c.spec, arrays, torch, "cuda")


def _q_tensor(torch, Q, like):
    return Q if isinstance(Q, torch.Tensor) else torch.full_like(like, Q)


@pytest.mark.parametrize("variant,name", WITH_TABLE)
def test_device_table_matches_the_table_the_reference_coded_with(torch_cuda, variant, name):
    torch = torch_cuda
    from gauspcc_amd import arithmetic

    c = pins.b_case(variant, name)
    for f in c.files:
        assert f.table is not None
        if c.kind == "gauss":
            _, mean, scale, Q = _args(torch, c, f)
            table = arithmetic.calculate_cdf(mean, scale, _q_tensor(torch, Q, mean), f.min, f.max)
        else:
            _, means, scales, probs, Q = _args(torch, c, f)
            q = _q_tensor(torch, Q, means[0])
            table = arithmetic.calculate_cdf_mixed(means, scales, probs, q, f.min, f.max)
            ref = None                                    # the path of test_mixture_coder_matches_table_path_and_oracle_files: the reference's expression on device tables
            for m, s, p in zip(means, scales, probs):
                t = arithmetic.calculate_cdf(m, s, q, f.min, f.max) * p.unsqueeze(-1)
                ref = t if ref is None else ref + t
            assert torch.equal(table, torch.clamp(ref, min=0.0, max=1.0))
        assert table.dtype == torch.float32 and tuple(table.shape) == f.table.shape
        err = float(np.abs(table.cpu().numpy().astype(np.float64) - f.table.astype(np.float64)).max())
        print(f"{name} {f.name}: device table vs the reference's {err:.3g}")
        assert err <= apc.TABLE_TOL, err


@pytest.mark.parametrize("variant,name", pins.B_IDS)
def test_device_coder_on_the_reference_table(torch_cuda, orc, variant, name):
    """arithmetic_encode / arithmetic_decode on the very table the reference coded with: the reference's cnt and payload, the reference's symbols.
    Where the fixture holds no table (more than 600 symbols) it is the oracle's, which tests/test_attr_pins_cpu.py shows to reproduce the file."""
    torch = torch_cuda
    from gauspcc_amd import arithmetic

    c = pins.b_case(variant, name)
    for f in c.files:
        table = f.table if f.table is not None else c.oracle_table(orc, f)
        cnt, payload = (ba.parse_bernoulli(f.blob)[1:] if c.kind == "bern" else ba.parse_gaussian(f.blob)[2:])
        n, lp = table.shape
        assert n == len(f.sym)
        t = torch.tensor(table).cuda()
        b, k = arithmetic.arithmetic_encode(torch.tensor(f.sym).cuda(), t, apc.CHUNK, n, lp)
        assert np.array_equal(k.cpu().numpy(), cnt) and np.array_equal(b.cpu().numpy(), payload)
        dec = arithmetic.arithmetic_decode(t, torch.tensor(payload.copy()), torch.tensor(cnt.copy()), apc.CHUNK, n, lp)
        assert dec.dtype == torch.int16 and np.array_equal(dec.cpu().numpy(), f.sym)


def _check_written(c, tmp_path, stem, bits):
    """The files `stem`_<c>.b against the reference's: names, min / max / chunk-table length, and the bit count of the bytes written."""
    got = sorted((p.name for p in tmp_path.glob(f"{stem}*.b")), key=lambda s: (len(s), s))
    assert got == [f.name.replace(c.name, stem, 1) for f in c.files]
    total = 0
    for f, fname in zip(c.files, got):
        blob = (tmp_path / fname).read_bytes()
        mn, mx, cnt, payload = ba.parse_gaussian(blob)
        wmn, wmx, wcnt, _ = ba.parse_gaussian(f.blob)
        assert (mn, mx) == (wmn, wmx) == (f.min, f.max) and cnt.size == wcnt.size == -(-len(f.sym) // apc.CHUNK)
        assert int(cnt.sum()) == payload.size
        total += (payload.size + 4 * cnt.size) * 8 + 96
    assert bits == total


def _check_decoded(torch, c, dec):
    want = torch.tensor(c.dec)
    assert dec.is_cuda and str(dec.dtype) == c.dec_dtype and dec.shape == want.shape
    assert torch.equal(dec.cpu(), want)


@pytest.mark.parametrize("variant,name", pins.B_IDS)
def test_wrappers_write_the_reference_s_files_and_decode_its_values(torch_cuda, variant, name, tmp_path):
    torch = torch_cuda
    from gauspcc_amd import encodings_cuda as ec

    c = pins.b_case(variant, name)
    fn = str(tmp_path / f"{name}.b")
    kw = dict(chunk_size=c.spec["chunk_size"]) if c.spec.get("chunk_size") else {}
    if c.kind == "bern":
        x = torch.tensor(c.arrays["x"]).cuda()
        bits = ec.encoder(x, file_name=fn)
        blob = (tmp_path / f"{name}.b").read_bytes()
        assert blob == c.files[0].blob                                       # byte for byte: the row [0, 1 - p, 1] is exact
        assert bits == c.bits == (len(blob) - 8) * 8 + 64
        _check_decoded(torch, c, ec.decoder(x.numel(), file_name=fn))
        return
    if c.kind == "fact":
        x = torch.tensor(c.arrays["x"]).cuda()
        bits = ec.encoder_factorized_chunk(x, apc.lower_func, c.spec["q"], file_name=fn, **kw)
        dec = ec.decoder_factorized_chunk(apc.lower_func, c.spec["q"], x.shape[0], x.shape[1], file_name=fn, **kw)
    elif c.kind == "gauss":
        x, mean, scale, Q = _args(torch, c)
        bits = ec.encoder_gaussian_chunk(x, mean, scale, Q, file_name=fn, **kw)
        dec = ec.decoder_gaussian_chunk(mean, scale, Q, file_name=fn, **kw)
    else:
        x, means, scales, probs, Q = _args(torch, c)
        bits = ec.encoder_gaussian_mixed_chunk(x, means, scales, probs, Q, file_name=fn, **kw)
        dec = ec.decoder_gaussian_mixed_chunk(means, scales, probs, Q, file_name=fn, **kw)
    _check_written(c, tmp_path, name, bits)
    _check_decoded(torch, c, dec)


@pytest.mark.parametrize("variant,name", GAUSS_MIX)
def test_slices_coders_with_the_case_s_chunk_bounds(torch_cuda, variant, name, tmp_path):
    """encoder_gaussian_slices / encoder_gaussian_mixed_slices, a slice per file the reference wrote: the stored headers, and the reference's decoded values."""
    torch = torch_cuda
    from gauspcc_amd import encodings_cuda as ec

    c = pins.b_case(variant, name)
    names = [str(tmp_path / f"s{i}.b") for i in range(len(c.files))]
    if c.kind == "gauss":
        x, mean, scale, Q = _args(torch, c)
        q = _q_tensor(torch, Q, mean)
        bits = ec.encoder_gaussian_slices(x, mean, scale, q, c.bounds, names)
        dec = ec.decoder_gaussian_slices(mean, scale, q, c.bounds, names)
    else:
        x, means, scales, probs, Q = _args(torch, c)
        q = _q_tensor(torch, Q, means[0])
        bits = ec.encoder_gaussian_mixed_slices(x, means, scales, probs, q, c.bounds, names)
        dec = ec.decoder_gaussian_mixed_slices(means, scales, probs, q, c.bounds, names)
    assert len(bits) == len(c.files)
    for i, f in enumerate(c.files):
        blob = (tmp_path / f"s{i}_0.b").read_bytes()
        mn, mx, cnt, payload = ba.parse_gaussian(blob)
        assert (mn, mx) == (f.min, f.max) and cnt.size == -(-len(f.sym) // apc.CHUNK) and int(cnt.sum()) == payload.size
        assert bits[i] == (payload.size + 4 * cnt.size) * 8 + 96
    _check_decoded(torch, c, dec)


# ------------------------------------------------------------------------------------------------------------ neural Gaussians
NG_RUNS = [(v, n, "masked") for v, n in pins.NG_IDS] + [(v, n, "all") for v, n in pins.NG_IDS
                                                        if next(c for c in apc.NG_CASES if c["name"] == n).get("also_without_mask")]


@pytest.mark.parametrize("variant,name,tag", NG_RUNS)
def test_generate_neural_gaussians_matches_the_reference_s_float64_run(torch_cuda, variant, name, tag):
    torch = torch_cuda
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians

    c = pins.ng_case(variant, name)
    run = c.runs[tag]
    pc, cam, vis = apc.ng_model(c.spec, c.arrays, torch, "cuda")
    vis = vis if tag == "masked" else None
    pc.ng_rows = vis
    res = generate_neural_gaussians(cam, pc, vis)
    assert len(res) == 6
    got = dict(zip(apc.NG_OUTPUTS, res[:5]))
    assert (res[5] == 0) if c.spec["decoded"] else (res[5] > 0)
    m = len(run.kept)
    for k, cols in zip(apc.NG_OUTPUTS, (3, 3, 1, 3, 4)):
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == (m, cols), (k, tuple(got[k].shape), m)
    # the kept candidates, from the positions: row i lies nearest to row i of the expectation, whose candidate index is kept[i]
    d = torch.cdist(got["xyz"].double().cpu(), torch.tensor(run.out["xyz"]).double())
    kept = run.kept[d.argmin(dim=1).numpy()]
    assert np.array_equal(kept, run.kept), (kept.tolist(), run.kept.tolist())
    for k in apc.NG_OUTPUTS:
        err = float(np.abs(got[k].cpu().numpy().astype(np.float64) - run.out[k].astype(np.float64)).max())
        print(f"{name} {tag} {k}: {err:.3g} (tolerance {run.tol[k]:.3g}, the reference's float32 vs float64 {run.f32_vs_f64[k]:.3g})")
        assert err <= run.tol[k], (k, err, run.tol[k])


def test_no_visible_anchor_gives_five_empty_tensors(torch_cuda):
    torch = torch_cuda
    from gauspcc_amd.neural_gaussians import generate_neural_gaussians

    c = pins.ng_case("hac", "hac_f32_k5")
    pc, cam, vis = apc.ng_model(c.spec, c.arrays, torch, "cuda")
    res = generate_neural_gaussians(cam, pc, torch.zeros_like(vis))
    assert [tuple(t.shape) for t in res[:5]] == [(0, 3), (0, 3), (0, 1), (0, 3), (0, 4)] and res[5] == 0
    assert all(t.is_cuda and t.dtype == torch.float32 for t in res[:5])
