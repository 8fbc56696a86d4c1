"""bench.py's command line without a GPU: the --full / --dump-outputs options and the output dump itself."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("rpg_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stderr[-2000:]


def test_dump_outputs_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    bench = _bench()
    rel = torch.randn(1792, 6)
    ei = torch.arange(2 * 1792, dtype=torch.int64).view(2, 1792)
    bench.dump_outputs(str(tmp_path / "a"), {"rel_poses": rel, "edge_index": ei})
    got = np.load(tmp_path / "a" / "rel_poses.npy")
    assert got.dtype == np.float32 and np.array_equal(got, rel.numpy())          # float32 kept bit for bit
    got = np.load(tmp_path / "a" / "edge_index.npy")
    assert got.dtype == np.float64 and np.array_equal(got, ei.numpy().astype(np.float64))
    # past the cap: a fixed sample of rows, the same on every call, within the budget
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 2 * 24 * 100)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"rel_poses": rel, "abs_poses": rel[:10]})
    b, c = np.load(tmp_path / "b" / "rel_poses.npy"), np.load(tmp_path / "c" / "rel_poses.npy")
    assert b.shape == (100, 6) and np.array_equal(b, c)
    assert all(any(np.array_equal(row, r) for r in rel.numpy()) for row in b[:5])
    assert np.array_equal(np.load(tmp_path / "b" / "abs_poses.npy"), rel[:10].numpy())
