"""CPU: bench.py's --dump-outputs writer.  A frame within the size limit is
written whole; a larger one (the 4K workloads) as the same seeded sample every
time, so the files of two runs line up value for value."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import torch

from conftest import REPO


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    st = SimpleNamespace(rays_primary=35, rays_shadow=2 ** 40 + 1, rays_reflect=7)
    rng = np.random.default_rng(1)
    small = rng.integers(0, 256, (10, 11, 3), dtype=np.uint8)
    large = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)

    bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(small), st)
    got = np.load(tmp_path / "a" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.astype(np.float32))
    rays = np.load(tmp_path / "a" / "ray_counts.npy")
    assert rays.dtype == np.float64 and [int(x) for x in rays] == [35, 2 ** 40 + 1, 7]

    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), torch.from_numpy(large), st)
    b, c = np.load(tmp_path / "b" / "frame.npy"), np.load(tmp_path / "c" / "frame.npy")
    assert b.dtype == np.float32 and b.shape == (1000,) and np.array_equal(b, c)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(large.size, 1000, replace=False))
    assert np.array_equal(b, large.reshape(-1)[idx].astype(np.float32))


def test_dump_limit_is_within_64_mb():
    bench = _bench()
    assert bench.DUMP_MAX_ELEMS * 4 + 3 * 8 + 2 * 128 <= 64 * 10 ** 6  # frame.npy + ray_counts.npy with headers
