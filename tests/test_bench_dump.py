"""bench.py --dump-outputs on the host: whole maps under the size budget, a fixed seeded pixel sample above it."""
import numpy as np

import bench


def _maps(h, w):
    rng = np.random.default_rng(3)
    m = {n: rng.random((h, w), dtype=np.float32) for n in ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled")}
    m["meanl"] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    m["meanr"] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return m


def test_whole_maps_as_float32(tmp_path):
    maps = _maps(30, 40)
    bench.dump_outputs(str(tmp_path), maps)
    assert sorted(f.name for f in tmp_path.iterdir()) == sorted(n + ".npy" for n in maps)
    for n, a in maps.items():
        got = np.load(tmp_path / (n + ".npy"))
        assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, a.astype(np.float32)), n


def test_sample_above_the_budget_is_fixed_and_within_it(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 4096)
    maps = _maps(120, 160)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), maps)
    bench.dump_outputs(str(b), maps)
    assert sum(f.stat().st_size for f in a.iterdir()) <= 200_000
    idx = np.load(a / "sample_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (4096,) and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(b / "sample_index.npy"))
    flat = idx.astype(np.int64)
    for n, m in maps.items():
        got = np.load(a / (n + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, m.reshape(-1)[flat].astype(np.float32)), n
