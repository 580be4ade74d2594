"""bench.py end to end on the GPU box, at a reduced point count: the ONE JSON line the driver parses carries the contract keys and
the `roofline` object; with --full also the `cpu_baseline` object, and every untimed pass behind the timed region ran (sizes, batched,
reference_layout, low_rate, chunk_sweep, scenes_in_flight, side_paths) -- a pass that raises takes the whole line with it, and nothing
else in the suite runs the script as the driver does.  (Round 6: a function-local `import tempfile` in tools/bench_side_paths.py
shadowed the module's and broke exactly this path; no test saw it.)  A plain run (no --full) runs none of those passes."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_bench_prints_one_complete_json_line(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--points", "100000", "--steps", "3", "--warmup", "1", "--cpu-sample", "20000",
                        "--side-anchors", "20000", "--dump-outputs", str(tmp_path / "out"), "--full"], capture_output=True, text=True, timeout=1500, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]               # stdout carries the one JSON line only
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in d, key
    assert d["unit"] == "Mpoints/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["value"] - 100000 * 3 / (d["ms_per_step"] * 3e-3) / 1e6) < 0.02 * d["value"]
    assert d["roundtrip_bit_identical"] is True
    rf = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in rf, key
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == "Mpoints/s" and "sample" in cb
    assert [s["points"] for s in d["sizes"]] == [10_000, 100_000, 1_000_000]
    assert all(b["bytes_identical_to_solo"] and b["decode_identical_to_solo"] and b["one_tree"] for b in d["batched"])
    ref = d["reference_layout"]
    assert ref["roundtrip_bit_identical"] and ref["bytes"] == d["bytes_v0"] and ref["dec_ms"] > ref["enc_ms"] > 0
    assert len(d["low_rate"]) == 2 and all(c["roundtrip_bit_identical"] and c["bytes_v0"] <= c["container_bytes"] for c in d["low_rate"])
    assert d["low_rate"][0]["bpp"] < 0.8 * d["bpp"] and d["low_rate"][1]["bits_per_coded_node"] < 6.0
    sw = d["chunk_sweep"]
    assert [c["chunk_log2"] for c in sw] == [9, 10, 11, 12, 13] and all(c["roundtrip_bit_identical"] for c in sw)
    assert all(a["bytes"] >= b["bytes"] for a, b in zip(sw, sw[1:]))              # smaller chunks cost bytes
    assert d["scenes_in_flight"]["scenes"] == 2 and d["scenes_in_flight"]["value"] > 0
    sp = d["side_paths"]
    assert sp["torchac_shim"]["roundtrip"] and sp["torchac_shim"]["fan_out_roundtrip"] and sp["gaussian_coder"]["fused_bytes_equal_table_bytes"]
    assert sp["rd_loop"]["psnr_decoded_vs_encoder_side_dB"] > 40
    # --dump-outputs: the last timed step's container and decoded points, exact (100 k points are far below the size limit)
    import numpy as np

    from gauspcc_amd import runtime
    from gauspcc_amd.dist import scene_seed
    from gauspcc_amd.synth import synthetic_cloud, synthetic_state_dict
    from tests import gpu_helpers as gh

    assert sorted(os.listdir(tmp_path / "out")) == ["scene0_container_bytes.npy", "scene0_decoded_points.npy"]
    blob = np.load(tmp_path / "out" / "scene0_container_bytes.npy")
    pts = np.load(tmp_path / "out" / "scene0_decoded_points.npy")
    assert blob.dtype == np.float32 and len(blob) == d["container_bytes"]
    assert pts.dtype == np.float64
    # the dumped container is scene 0's: byte for byte an owned encode of the same cloud with the same weights
    cloud = synthetic_cloud(100000, seed=scene_seed(1234, 0))
    model = runtime.Model(synthetic_state_dict(32, 5), 32, 5, 0)
    data = bytes(blob.astype(np.uint8))
    assert np.array_equal(blob, np.frombuffer(data, np.uint8)) and data == gh.encode(model, cloud, 11)[0]
    # ... and the dumped points are what decoding it returns, in the decoder's order; as a set they are the cloud
    assert np.array_equal(gh.decode(model, data)[0].astype(np.float64), pts)
    ref = cloud.astype(np.float64)
    assert np.array_equal(pts[np.lexsort(pts.T[::-1])], ref[np.lexsort(ref.T[::-1])])


def test_plain_bench_runs_only_the_timed_steps(tmp_path):
    """Without --full: the same contract keys and the timed steps' own roofline, none of the untimed passes, and --dump-outputs still
    writes the last timed step's containers and points."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--points", "100000", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in d, key
    assert d["unit"] == "Mpoints/s" and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and abs(d["value"] - 100000 * 3 / (d["ms_per_step"] * 3e-3) / 1e6) < 0.02 * d["value"]
    assert d["roundtrip_bit_identical"] is True
    rf = d["roofline"]
    assert rf["launches"] > 0 and 0 < rf["frac"] < 1 and rf["stages"] == []
    for key in ("bytes_v0", "scenes_in_flight", "sizes", "batched", "reference_layout", "low_rate", "chunk_sweep"):
        assert d[key] is None, key
    assert "side_paths" not in d and "cpu_baseline" not in d
    assert "Start encoding" not in r.stderr                 # the side-path callers never ran
    assert sorted(os.listdir(tmp_path / "out")) == ["scene0_container_bytes.npy", "scene0_decoded_points.npy"]
    import numpy as np

    assert len(np.load(tmp_path / "out" / "scene0_container_bytes.npy")) == d["container_bytes"]
    assert np.load(tmp_path / "out" / "scene0_decoded_points.npy").shape == (100000, 3)
