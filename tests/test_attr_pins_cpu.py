"""The attribute side against what the reference's own Python computed and wrote (tests/golden/attr_b_*.npz, ng_*.npz, made by
tests/golden/make_attr_pins.py from HAC/utils/encodings_cuda.py:38-175, 317-492, HAC-plus/utils/encodings_cuda.py:177-317 and the two
gaussian_renderer/__init__.py running under stand-ins), the part that needs no GPU:

  * the builders of tests/attr_pin_cases.py still give the inputs the fixtures were made from (sha256);
  * the `.b` file the GPU tests assemble as their expectation (tests/b_assembly.py: oracle table -> oracle coder -> header | cnt | payload)
    equals the file the reference wrote, byte for byte, with the reference's bit count -- so round(x / Q), min / max and their float32
    storage, the expansion of a scalar Q, the chunking and `_<c>.b` names, the header, the Bernoulli row and the mixture's component
    order and clamp are the reference's, not this project's reading of them;
  * oracle.gaussian_mixed_cdf equals the mixture table the reference's Python handed to the coder bit for bit;
  * the product's host-side readers (encodings_cuda._read_b, _read_slice_files with `lens`) accept every file and return its fields.
"""
import numpy as np
import pytest

from . import attr_pin_cases as apc
from . import attr_pins as pins
from . import b_assembly as ba


@pytest.mark.parametrize("variant,name", pins.B_IDS)
def test_b_inputs_are_those_of_the_fixture(variant, name):
    c = pins.b_case(variant, name)
    assert apc.sha256_of(c.arrays) == c.sha256, "the builders no longer give the fixture's inputs: regenerate"
    assert c.bounds == ([0, c.arrays["x"].size] if c.kind == "bern" else apc.b_chunk_bounds(c.spec, c.arrays["x"].shape[0]))
    want = [f"{name}.b"] if c.kind == "bern" else [f"{name}_{i}.b" for i in range(len(c.bounds) - 1)]
    assert [f.name for f in c.files] == want


@pytest.mark.parametrize("variant,name", pins.NG_IDS)
def test_ng_inputs_are_those_of_the_fixture(variant, name):
    c = pins.ng_case(variant, name)
    built = apc.ng_inputs(c.spec)
    assert apc.sha256_of(built) == c.sha256, "the builders no longer give the fixture's inputs: regenerate"
    assert set(built) == set(c.arrays) and all(np.array_equal(built[k], c.arrays[k]) for k in built)
    for run in c.runs.values():
        assert all(run.tol[k] == max(apc.NG_TOL[k], 4 * run.f32_vs_f64[k]) for k in apc.NG_OUTPUTS)
        assert len(run.kept) == len(run.out["xyz"]) > 0 and np.all(np.diff(run.kept) > 0)
        assert run.separation >= apc.SEPARATION * run.tol["xyz"]                # a position names its candidate


@pytest.mark.parametrize("variant,name", [i for i in pins.B_IDS if apc.b_case(i[1])["kind"] != "fact"])
def test_assembled_file_equals_the_reference_written_file(orc, variant, name):
    c = pins.b_case(variant, name)
    bits = 0
    for f in c.files:
        a = c.part(f)
        if c.kind == "bern":
            xs = a["x"].reshape(-1)
            p1 = np.float32(xs.sum(dtype=np.float32) / np.float32(xs.size))        # a sum of {0, 1}: exact in float32 in any order
            blob, b = ba.bernoulli_file(orc, xs, p1)
            assert np.array_equal(f.sym, xs.astype(np.int16))
        else:
            xi = np.rint(a["x"] / a["q"])                                           # float32, half to even: torch.round(x / Q)
            mn, mx = float(xi.min()), float(xi.max())
            assert (mn, mx) == (f.min, f.max)
            sym = (xi - mn).astype(np.int16)
            assert np.array_equal(sym, f.sym)
            blob, b = ba.gaussian_file(orc, sym, c.oracle_table(orc, f), mn, mx)
        assert blob == f.blob, f"{f.name}: first difference at byte {next((i for i, (p, q) in enumerate(zip(blob, f.blob)) if p != q), min(len(blob), len(f.blob)))}"
        bits += b
    assert bits == c.bits
    if c.kind == "bern":
        assert c.dec_dtype == "torch.int16" and np.array_equal(c.dec, c.arrays["x"].reshape(-1).astype(np.int16))
    else:
        q = c.arrays["q"] if "q" in c.arrays else np.float32(c.spec["q"])
        assert c.dec_dtype == "torch.float32" and c.dec.dtype == np.float32 and np.array_equal(c.dec, np.rint(c.arrays["x"] / q) * q)


@pytest.mark.parametrize("variant,name", [i for i in pins.B_IDS if apc.b_case(i[1])["kind"] in ("gauss", "mix")])
def test_oracle_table_is_the_table_the_reference_coded_with(orc, variant, name):
    """Bit for bit: for the mixture this pins the order the components are added in and the clamp (HAC-plus/utils/encodings_cuda.py:213-226)."""
    c = pins.b_case(variant, name)
    stored = [f for f in c.files if f.table is not None]
    assert stored or c.spec["n"] > apc.TABLE_ROWS_MAX
    for f in stored:
        t = c.oracle_table(orc, f)
        assert t.dtype == f.table.dtype and np.array_equal(t, f.table)
    assert c.table_vs_f64 <= apc.TABLE_TOL


def test_factorized_files_hold_the_reference_table_s_stream(orc):
    """The factorized table is torch's (sigmoid, cumsum): the file is the oracle coder's on the table the reference built, and its layout the Gaussian one."""
    for variant in pins.VARIANTS:
        c = pins.b_case(variant, "f_chunk23")
        assert len(c.files) == 3 and c.dec.shape == (23, 3)
        bits = 0
        for f in c.files:
            xi = np.rint(c.part(f)["x"] / np.float32(c.spec["q"]))
            assert (float(xi.min()), float(xi.max())) == (f.min, f.max) and np.array_equal((xi - xi.min()).astype(np.int16).reshape(-1), f.sym)
            blob, b = ba.gaussian_file(orc, f.sym, f.table, f.min, f.max)
            assert blob == f.blob
            bits += b
        assert bits == c.bits


@pytest.mark.parametrize("variant,name", pins.B_IDS)
def test_host_readers_accept_the_reference_written_files(variant, name, tmp_path):
    from gauspcc_amd.encodings_cuda import _read_b, _read_slice_files, chunk_size_cuda

    c = pins.b_case(variant, name)
    if c.kind == "bern":
        p, cnt, payload = ba.parse_bernoulli(c.files[0].blob)
        xs = c.arrays["x"].reshape(-1)
        assert p == np.float32(xs.sum() / xs.size) and cnt.size == -(-xs.size // chunk_size_cuda) and int(cnt.sum()) == payload.size
        return
    paths = []
    for f in c.files:
        (tmp_path / f.name).write_bytes(f.blob)
        paths.append(str(tmp_path / f.name))
        mn, mx, data, cnt = _read_b(paths[-1])
        wmn, wmx, wcnt, wpayload = ba.parse_gaussian(f.blob)
        assert (mn, mx) == (f.min, f.max) == (wmn, wmx)
        assert np.array_equal(cnt.numpy(), wcnt) and np.array_equal(data.numpy(), wpayload) and int(wcnt.sum()) == wpayload.size
    lens = [len(f.sym) for f in c.files]
    mins, maxs, cnts, datas = _read_slice_files(paths, lens)
    for f, mn, mx, cnt, data, ln in zip(c.files, mins, maxs, cnts, datas, lens):
        assert (float(mn), float(mx)) == (f.min, f.max) and cnt.size == -(-ln // chunk_size_cuda) and int(cnt.sum()) == data.size
    with pytest.raises(RuntimeError, match="chunk table"):
        _read_slice_files(paths[:1], [lens[0] + chunk_size_cuda])
