"""The torchac-based attribute coders of TC-GS and CAT-3DGS (src/gs_compress/TC-GS/utils/encodings.py:84-176,
src/gs_compress/CAT-3DGS/utils/encodings.py:39-175 -- the two files agree on these functions), SURVEY.md §8(f) row 4:

    from gauspcc_amd.torchac_encodings import encoder_gaussian, decoder_gaussian, encoder, decoder

Same signatures, same `.b` files (ONE torchac stream per file), same return values.  What differs from the reference is
where things run: the reference builds the float CDF table with `torch.distributions` on the GPU, moves the whole table
to the CPU (4 bytes per entry) and lets torchac integerise and code it there; here the table is integerised on the device
it was built on (2 bytes per entry cross PCIe, `gauspcc_amd.torchac`) and coded by libgauspcc's host-side coder
(csrc/hostcoder.hip) -- a single stream is one dependent chain, which a host core runs faster than a GPU lane.  Tables are
built in slabs of rows so that an attribute of millions of symbols never materialises n x (range + 2) floats at once.
CPU tensors work as well (torchac's own convention); nothing here needs a GPU.
"""
import torch

from . import torchac

_SLAB_ENTRIES = 1 << 26          # table entries built at a time (256 MB of float32)

# encodings.py:14 -- the reference's switch between ONE torchac stream per attribute file and its ten-way fan-out (multiprocess_encoder /
# multiprocess_deoder: `<name>_<m>.b`, m = 0..9, each chunk of ceil(n / 10) rows its own stream).  Upstream says "Always False plz. Not yet
# implemented for True" (its fan-out forks ten processes that pickle the table); here both settings work and give the files the reference's
# functions would write.  A single stream is one dependent chain (36 Msymbols/s on one host thread); the ten chunks are independent chains
# and run on ten native threads (the library calls release the GIL) -- the shape to use for attribute sets of 10^7 symbols and more.
use_multiprocessor = False


def _as_q(Q, like):
    if not isinstance(Q, torch.Tensor):
        Q = torch.tensor([Q], dtype=like.dtype, device=like.device).repeat(like.shape[0])     # encodings.py:86-87
    return Q


def _int_rows(mean, scale, Q, min_value, max_value):
    """int16 rows of the table `Normal(mean, scale).cdf((samples - 0.5) * Q)`, samples = min_value .. max_value + 1
    (encodings.py:92-99), integerised as torchac does (`_convert_to_int_and_normalize`), slab by slab, on mean's device"""
    lo, hi = int(min_value), int(max_value)
    samples = torch.arange(lo, hi + 2, device=mean.device).to(torch.float)
    lp = samples.numel()
    rows_per = max(1, _SLAB_ENTRIES // lp)
    out = []
    for a in range(0, mean.shape[0], rows_per):
        m = mean[a: a + rows_per].unsqueeze(-1)
        s = scale[a: a + rows_per].unsqueeze(-1)
        q = Q[a: a + rows_per].unsqueeze(-1)
        lower = torch.distributions.normal.Normal(m, s).cdf((samples.unsqueeze(0) - 0.5) * q)
        out.append(torchac._to_int_rows(lower))
    return torch.cat(out, dim=0) if out else torch.zeros((0, lp), dtype=torch.int16, device=mean.device)


def _chunk_rows(n, chunk_num):
    chunk_len = -(-int(n) // int(chunk_num)) if n else 0                    # int(math.ceil(encoding_len / chunk_num)) (:45, :66)
    return [(m, m * chunk_len, min(n, (m + 1) * chunk_len)) for m in range(chunk_num)]


def multiprocess_encoder(lower, symbol, file_name, chunk_num=10):
    """encodings.py:36-59: rows [m c, (m + 1) c) of the table and their symbols -> `<name>_<m>.b`, m = 0 .. chunk_num - 1 (an empty chunk
    writes an empty file, as torchac does for no symbols); returns the total bit length.  `lower`: float CDF rows (any device) or int16 rows."""
    from concurrent.futures import ThreadPoolExecutor

    assert file_name.endswith('.b')
    n = lower.shape[0]
    enc = torchac.encode_int16_normalized_cdf if lower.dtype == torch.int16 else (lambda l, s_: torchac.encode_float_cdf(l, s_, check_input_bounds=True))

    def one(job):
        m, a, b = job
        byte_stream = enc(lower[a:b], symbol[a:b]) if b > a else b""
        with open(file_name.replace('.b', f'_{m}.b'), 'wb') as fout:
            fout.write(byte_stream)
        return len(byte_stream) * 8

    with ThreadPoolExecutor(max_workers=chunk_num) as pool:
        return sum(pool.map(one, _chunk_rows(n, chunk_num)))


def multiprocess_deoder(lower, file_name, chunk_num=10):
    """encodings.py:62-82 (the reference's spelling): the inverse -- every chunk file decoded on its own thread, results concatenated on
    lower's device (the reference returns `.cuda()`: the same thing for its callers, whose tables are built on the GPU)."""
    from concurrent.futures import ThreadPoolExecutor

    assert file_name.endswith('.b')
    n = lower.shape[0]
    dec = torchac.decode_int16_normalized_cdf if lower.dtype == torch.int16 else torchac.decode_float_cdf

    def one(job):
        m, a, b = job
        with open(file_name.replace('.b', f'_{m}.b'), 'rb') as fin:
            byte_stream_d = fin.read()
        if b <= a:
            return torch.zeros(0, dtype=torch.float32, device=lower.device)
        return dec(lower[a:b], byte_stream_d).to(torch.float32)

    with ThreadPoolExecutor(max_workers=chunk_num) as pool:
        parts = list(pool.map(one, _chunk_rows(n, chunk_num)))
    return torch.cat(parts, dim=0).to(lower.device)


def encoder_gaussian(x, mean, scale, Q, file_name='tmp.b'):
    """encodings.py:84-120.  Returns (bit_len, min_value, max_value) -- the two bounds as 0-d tensors, as the reference's."""
    assert file_name.endswith('.b')
    Q = _as_q(Q, mean)
    assert x.shape == mean.shape == scale.shape == Q.shape
    x_int_round = torch.round(x / Q)
    max_value = x_int_round.max()
    min_value = x_int_round.min()
    x_int_round_idx = (x_int_round - min_value).to(torch.int16)
    assert (x_int_round_idx.to(torch.int32) == x_int_round - min_value).all()
    rows = _int_rows(mean, scale, Q, min_value.item(), max_value.item())
    if use_multiprocessor:                                                   # (:114)
        return multiprocess_encoder(rows, x_int_round_idx, file_name), min_value, max_value
    byte_stream = torchac.encode_int16_normalized_cdf(rows, x_int_round_idx)
    with open(file_name, 'wb') as fout:
        fout.write(byte_stream)
    return len(byte_stream) * 8, min_value, max_value


def decoder_gaussian(mean, scale, Q, file_name='tmp.b', min_value=-100, max_value=100):
    """encodings.py:123-146.  min_value / max_value: what encoder_gaussian returned (tensors or numbers)."""
    assert file_name.endswith('.b')
    Q = _as_q(Q, mean)
    assert mean.shape == scale.shape == Q.shape
    lo = min_value.item() if isinstance(min_value, torch.Tensor) else min_value
    hi = max_value.item() if isinstance(max_value, torch.Tensor) else max_value
    rows = _int_rows(mean, scale, Q, lo, hi)
    if use_multiprocessor:                                                   # (:136)
        sym_out = multiprocess_deoder(rows, file_name, chunk_num=10).to(mean.device).to(torch.float32)
        return (sym_out + min_value) * Q
    with open(file_name, 'rb') as fin:
        byte_stream_d = fin.read()
    sym_out = torchac.decode_int16_normalized_cdf(rows, byte_stream_d).to(mean.device).to(torch.float32)
    x = sym_out + min_value
    return x * Q


# ---------------------------------------------------------------- all slices of an attribute at once
# limits of one gsac_encode_normal_streams call (include/gauspcc.h): slices per call, and count x (2 longest + 48) bytes below 4 GiB.  The call's
# workspace is sized by count x LONGEST slice (4 bytes of packed words and twice 2 bytes of coder scratch per symbol slot), so many short slices beside
# one long one reserve far more than their symbols: the split below keeps a call's workspace under 4 GiB whatever the mix of lengths
_STREAMS_PER_CALL = 65535
_STREAM_BYTES_PER_CALL = 1 << 30


def _slice_groups(lens):
    """Consecutive runs [a, b) of slices that one device call takes."""
    groups, a, longest = [], 0, 0
    for i, ln in enumerate(lens):
        new_longest = max(longest, int(ln))
        if i > a and ((i + 1 - a) > _STREAMS_PER_CALL or (i + 1 - a) * (2 * new_longest + 48) >= _STREAM_BYTES_PER_CALL):
            groups.append((a, i))
            a, new_longest = i, int(ln)
        longest = new_longest
    groups.append((a, len(lens)))
    return groups


def _slice_lens(slice_start, n):
    ss = [int(v) for v in slice_start]
    assert len(ss) >= 1 and ss[0] == 0 and ss[-1] == n and all(b >= a for a, b in zip(ss, ss[1:])), "slice_start: 0 = s[0] <= s[1] <= ... <= s[-1] = len(x)"
    return ss, [b - a for a, b in zip(ss, ss[1:])]


def host(vals):
    """per-slice bounds as the encoder returned them (0-d tensors, or numbers) -> a float32 numpy array"""
    import numpy as np
    if all(isinstance(v, torch.Tensor) for v in vals):
        return torch.stack([v.detach().reshape(()) for v in vals]).to(torch.float32).cpu().numpy()
    return np.array([float(v) for v in vals], dtype=np.float32)


def encoder_gaussian_slices(x, mean, scale, Q, slice_start, file_names):
    """encoder_gaussian for MANY slices of one attribute: slice s = elements [slice_start[s], slice_start[s + 1]) goes to file_names[s] as ONE raw
    torchac stream with its own min / max, as TC-GS's loop writes it per 1 000-anchor slice (TC-GS/scene/gaussian_model.py:1197-1271).  Returns
    (bit_lens, min_values, max_values): three lists with one entry per slice, the bounds as 0-d tensors (what the reference collects into
    `patched_infos`).  A slice of length 0 writes an empty file and reports min = max = 0.

    CUDA tensors: all slices are coded concurrently on the device (gsac_encode_normal_streams), CDF entries evaluated inside the coder, no table; the
    files are written on native threads (inside `encodings_cuda.deferred_writes()` in the background).  CPU tensors: the per-file encoder_gaussian
    above, slice by slice -- the same files as calling it yourself.

    The pair encoder_gaussian_slices / decoder_gaussian_slices reads only its own files: on the device the table is the library's entry function
    (csrc/attributes.hip: normal_cdf_entry, the float32 steps of `Normal.cdf` spelled out), which may differ from a torch-built table in rare entries
    (tests/test_gpu_normal_streams.py prints the share) -- the reference's own files are tied to one `erf` implementation in the same way."""
    assert len(x.shape) == 1
    Q = _as_q(Q, mean)
    assert x.shape == mean.shape == scale.shape == Q.shape
    ss, lens = _slice_lens(slice_start, x.shape[0])
    assert len(file_names) == len(lens) and all(f.endswith('.b') for f in file_names)
    if not x.is_cuda:
        bits, mins, maxs = [], [], []
        for a, b, fn in zip(ss, ss[1:], file_names):
            if b == a:
                open(fn, 'wb').close()
                bl, mn, mx = 0, torch.zeros((), dtype=x.dtype), torch.zeros((), dtype=x.dtype)
            else:
                bl, mn, mx = encoder_gaussian(x[a:b], mean[a:b], scale[a:b], Q[a:b], file_name=fn)
            bits.append(bl); mins.append(mn); maxs.append(mx)
        return bits, mins, maxs
    import numpy as np

    from . import arithmetic
    from .encodings_cuda import _write_files
    bits, mins, maxs, jobs = [], [], [], []
    cont = lambda t, a, b: t[a:b].detach().contiguous()
    for ga, gb in _slice_groups(lens):
        a, b = ss[ga], ss[gb]
        mn, mx, data, cnt = arithmetic.encode_normal_streams(cont(x, a, b), cont(mean, a, b), cont(scale, a, b), cont(Q, a, b), [v - a for v in ss[ga:gb + 1]])
        off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
        blob = data.tobytes()
        jobs += [(file_names[ga + i], blob[int(off[i]):int(off[i + 1])]) for i in range(gb - ga)]
        bits += [int(c) * 8 for c in cnt]
        mins.append(mn); maxs.append(mx)
    _write_files(jobs)
    as_list = lambda parts: list(torch.from_numpy(np.concatenate(parts)).to(x.device).unbind(0))
    return bits, as_list(mins), as_list(maxs)


def decoder_gaussian_slices(mean, scale, Q, slice_start, file_names, min_values, max_values):
    """Inverse of encoder_gaussian_slices: the values of all slices, concatenated in slice order, on mean's device.  min_values / max_values: the
    lists the encoder returned (tensors or numbers).  CUDA tensors: every stream is decoded by a wave of its own in one device call
    (gsac_decode_normal_streams); CPU tensors: decoder_gaussian per file.  Reads only files of encoder_gaussian_slices (see there)."""
    Q = _as_q(Q, mean)
    assert len(mean.shape) == 1 and mean.shape == scale.shape == Q.shape
    ss, lens = _slice_lens(slice_start, mean.shape[0])
    assert len(file_names) == len(lens) == len(min_values) == len(max_values) and all(f.endswith('.b') for f in file_names)
    if not mean.is_cuda:
        parts = [decoder_gaussian(mean[a:b], scale[a:b], Q[a:b], file_name=fn, min_value=mn, max_value=mx)
                 for a, b, fn, mn, mx in zip(ss, ss[1:], file_names, min_values, max_values) if b > a]
        return torch.cat(parts, dim=0) if parts else torch.zeros(0, dtype=torch.float32)
    import numpy as np

    from . import arithmetic
    from .encodings_cuda import _read_files

    mins, maxs = host(min_values), host(max_values)
    blob, offs = _read_files(file_names)         # one blob, valid until this thread's next call: decoded at once
    cnt = np.diff(offs)
    cont = lambda t, a, b: t[a:b].detach().contiguous()
    out = []
    for ga, gb in _slice_groups(lens):
        a, b = ss[ga], ss[gb]
        if int(offs[gb] - offs[ga]) >= 1 << 32:
            raise ValueError("decoder_gaussian_slices: the files of one device call exceed 4 GiB (not written by encoder_gaussian_slices)")
        out.append(arithmetic.decode_normal_streams(cont(mean, a, b), cont(scale, a, b), cont(Q, a, b), [v - a for v in ss[ga:gb + 1]], mins[ga:gb], maxs[ga:gb],
                                                    blob[int(offs[ga]):int(offs[gb])], cnt[ga:gb].astype(np.int32)))
    return out[0] if len(out) == 1 else torch.cat(out, dim=0)


def _binary_cdf(p):
    p_u = 1 - p.unsqueeze(-1)
    return torch.cat([torch.zeros_like(p_u), p_u, torch.ones_like(p_u)], dim=-1)      # encodings.py:153-157


def encoder(x, p, file_name):
    """encodings.py:149-165: x in {-1, +1} with P(x = +1) = p, one torchac stream"""
    assert file_name[-2:] == '.b'
    x = x.detach()
    p = p.detach()
    sym = torch.floor((x + 1) / 2).to(torch.int16)
    byte_stream = torchac.encode_float_cdf(_binary_cdf(p), sym, check_input_bounds=True)
    with open(file_name, 'wb') as fout:
        fout.write(byte_stream)
    return len(byte_stream) * 8


def decoder(p, file_name):
    """encodings.py:167-183"""
    dvc = p.device
    assert file_name[-2:] == '.b'
    with open(file_name, 'rb') as fin:
        byte_stream = fin.read()
    sym_out = torchac.decode_float_cdf(_binary_cdf(p.detach()), byte_stream)
    return (sym_out * 2 - 1).to(torch.float32).to(dvc)
