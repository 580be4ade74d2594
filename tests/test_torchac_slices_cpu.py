"""gauspcc_amd.torchac_encodings.encoder_gaussian_slices / decoder_gaussian_slices on CPU tensors: the slice form of TC-GS's attribute files
(one raw torchac stream per slice, TC-GS/scene/gaussian_model.py:1197-1271) loops over the per-file functions, so it writes the files that
encoder_gaussian called once per slice writes.  No GPU involved."""
import os

import torch


def _scene(n, seed):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(n, generator=g) * 0.8
    scale = torch.rand(n, generator=g) * 0.9 + 0.05
    Q = torch.rand(n, generator=g) * 0.1 + 0.05
    x = (mean + scale * torch.randn(n, generator=g)).clamp(-3.0, 3.0)
    return x, mean, scale, Q


# lengths 700, 0, 1, 1300, 0: an empty slice inside and at the end, a slice of one element
SLICE_START = [0, 700, 700, 701, 2001, 2001]


def test_slices_write_the_per_slice_files_and_round_trip(tmp_path):
    from gauspcc_amd import torchac_encodings as te

    x, mean, scale, Q = _scene(SLICE_START[-1], 11)
    names = [str(tmp_path / f"feat_{s}.b") for s in range(len(SLICE_START) - 1)]
    bits, mins, maxs = te.encoder_gaussian_slices(x, mean, scale, Q, SLICE_START, names)
    assert len(bits) == len(mins) == len(maxs) == len(names)
    for s, (a, b) in enumerate(zip(SLICE_START, SLICE_START[1:])):
        data = open(names[s], "rb").read()
        assert bits[s] == 8 * len(data)
        assert isinstance(mins[s], torch.Tensor) and mins[s].dim() == 0 and isinstance(maxs[s], torch.Tensor) and maxs[s].dim() == 0
        if b == a:
            assert data == b"" and mins[s] == 0 and maxs[s] == 0          # torchac codes no symbols into no bytes
            continue
        solo = str(tmp_path / f"solo_{s}.b")
        sb, lo, hi = te.encoder_gaussian(x[a:b], mean[a:b], scale[a:b], Q[a:b], file_name=solo)
        assert data == open(solo, "rb").read() and len(data) > 0
        assert bits[s] == sb and mins[s] == lo and maxs[s] == hi
    dec = te.decoder_gaussian_slices(mean, scale, Q, SLICE_START, names, mins, maxs)
    assert dec.dtype == torch.float32 and dec.shape == x.shape
    assert torch.equal(dec, torch.round(x / Q) * Q)
    # the bounds as plain numbers, as a caller that stored them in a file would pass them
    dec2 = te.decoder_gaussian_slices(mean, scale, Q, SLICE_START, names, [m.item() for m in mins], [m.item() for m in maxs])
    assert torch.equal(dec2, dec)


def test_scalar_q_and_a_single_slice(tmp_path):
    from gauspcc_amd import torchac_encodings as te

    x, mean, scale, _ = _scene(500, 12)
    name = str(tmp_path / "scaling_0.b")
    bits, mins, maxs = te.encoder_gaussian_slices(x, mean, scale, 0.125, [0, 500], [name])
    solo = str(tmp_path / "solo.b")
    sb, lo, hi = te.encoder_gaussian(x, mean, scale, 0.125, file_name=solo)
    assert open(name, "rb").read() == open(solo, "rb").read() and bits == [sb] and mins[0] == lo and maxs[0] == hi
    assert torch.equal(te.decoder_gaussian_slices(mean, scale, 0.125, [0, 500], [name], mins, maxs), torch.round(x / 0.125) * 0.125)
    assert sorted(os.listdir(tmp_path)) == ["scaling_0.b", "solo.b"]
