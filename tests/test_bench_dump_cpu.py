"""bench.py --dump-outputs without a GPU: the arrays a step returned land as exact float32 / float64 .npy files, and outputs above
the size limit are cut to a seeded sample of rows that is the same from run to run.  The GPU side (what the timed step wrote) is
covered by tests/test_gpu_bench_line.py."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _outputs(rng):
    return [(s, bytes(rng.integers(0, 256, 5000 + 7 * s, dtype=np.uint8)), rng.integers(-(1 << 30), 1 << 30, (3000, 3), dtype=np.int32))
            for s in (1, 0)]


def test_dump_is_exact_below_the_limit(tmp_path):
    outs = _outputs(np.random.default_rng(1))
    _bench().dump_outputs(str(tmp_path), outs)
    for s, blob, pts in outs:
        b = np.load(tmp_path / f"scene{s}_container_bytes.npy")
        p = np.load(tmp_path / f"scene{s}_decoded_points.npy")
        assert b.dtype == np.float32 and np.array_equal(b, np.frombuffer(blob, np.uint8))
        assert p.dtype == np.float64 and np.array_equal(p, pts)
    assert sorted(os.listdir(tmp_path)) == ["scene0_container_bytes.npy", "scene0_decoded_points.npy",
                                            "scene1_container_bytes.npy", "scene1_decoded_points.npy"]


def test_dump_above_the_limit_is_a_fixed_sample_within_it(tmp_path):
    outs = _outputs(np.random.default_rng(2))
    limit = 60_000
    bench = _bench()
    bench.dump_outputs(str(tmp_path / "a"), outs, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), outs, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert len(a) > 0 and np.array_equal(a, b)
    for s, _, pts in outs:                                   # sampled rows are whole rows of the output
        p = np.load(tmp_path / "a" / f"scene{s}_decoded_points.npy")
        assert len(p) < len(pts) and {tuple(r) for r in p.astype(np.int64)} <= {tuple(r) for r in pts.astype(np.int64)}


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
