"""bench.py --dump-outputs, without a GPU: the writer keeps whole images while they fit the 64 MB budget, and above it the same fixed,
seeded sample of pixels in every array, named by pixel_index.npy, within the budget and identical from run to run."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def images(h, w):
    rng = np.random.default_rng(7)
    return {"radiance": rng.random((h, w, 4), dtype=np.float32), "postprocessed": rng.integers(0, 256, (h, w, 4), dtype=np.uint8)}


def test_whole_images_while_they_fit(bench, tmp_path):
    src = images(54, 96)
    bench.write_outputs(str(tmp_path), src)
    assert sorted(os.listdir(tmp_path)) == ["postprocessed.npy", "radiance.npy"]
    for k, a in src.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    assert bench.DUMP_BYTES == 64 * 10 ** 6
    assert 1080 * 1920 * 4 * 4 <= bench.DUMP_BYTES   # the headline's radiance image goes out whole


def test_a_seeded_sample_of_pixels_above_the_budget(bench, tmp_path):
    src = images(108, 192)
    budget = 200000
    for run in ("a", "b"):
        bench.write_outputs(str(tmp_path / run), src, budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["pixel_index.npy", "postprocessed.npy", "radiance.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and len(idx) > 1000 and np.all(np.diff(idx) > 0) and idx[-1] < 108 * 192
    for k, a in src.items():
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, a.reshape(-1, 4)[idx.astype(np.int64)].astype(np.float32))
    for f in files:   # the same arguments give the same files
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
