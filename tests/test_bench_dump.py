"""bench.py --dump-outputs on the host side: the files dump_outputs writes, their dtypes, and the fixed pixel sample that keeps a
large frame within the 64 MB budget.  The GPU run through bench.py itself is in tests/test_gpu_bench.py."""
import os

import numpy as np

import bench


def _frame(h, w):
    rng = np.random.default_rng(3)
    acc = rng.random((h, w, 4), dtype=np.float32) * 16
    pixels = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
    return acc, pixels


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_frame_is_written_whole(tmp_path):
    acc, pixels = _frame(144, 256)
    bench.dump_outputs(str(tmp_path), acc, pixels)
    got = _load(tmp_path)
    assert sorted(got) == ["accumulator", "pixels_rgb"]
    assert got["accumulator"].dtype == np.float32 and np.array_equal(got["accumulator"], acc)
    rgb = got["pixels_rgb"]
    assert rgb.dtype == np.float32 and rgb.shape == (144, 256, 3)
    for c in range(3):
        assert np.array_equal(rgb[..., c], ((pixels >> (8 * c)) & 0xFF).astype(np.float32))
    bench.dump_outputs(str(tmp_path / "acc_only"), acc, None)
    assert sorted(_load(tmp_path / "acc_only")) == ["accumulator"]


def test_large_frame_is_a_fixed_sample_within_the_budget(tmp_path):
    acc, pixels = _frame(2160, 3840)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), acc, pixels)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["accumulator", "pixel_index", "pixels_rgb"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 1000 * 1000
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["pixel_index"]
    assert idx.dtype == np.float64 and idx.size > 1000000 and np.all(np.diff(idx) > 0)
    i = idx.astype(np.int64)
    assert a["accumulator"].dtype == np.float32 and np.array_equal(a["accumulator"], acc.reshape(-1, 4)[i])
    assert np.array_equal(a["pixels_rgb"][:, 1], ((pixels.reshape(-1)[i] >> 8) & 0xFF).astype(np.float32))
