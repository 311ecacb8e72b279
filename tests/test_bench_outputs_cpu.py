"""bench.py --dump-outputs on the CPU: the files it writes, and the seeded row sample of a frame larger than the limit."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_small_frame_is_written_whole(tmp_path):
    img = np.arange(8 * 8 * 3, dtype=np.float32).reshape(8, 8, 3)
    bench.dump_outputs(str(tmp_path / "d"), img, 1234)
    got = np.load(tmp_path / "d" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)
    rays = np.load(tmp_path / "d" / "rays.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [1234.0]
    assert not (tmp_path / "d" / "image_rows.npy").exists()


def test_large_frame_is_a_fixed_sample_of_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_IMAGE_LIMIT", 10 * 16 * 3 * 4)          # room for 10 rows of 16 pixels
    img = np.arange(100 * 16 * 3, dtype=np.float32).reshape(100, 16, 3)
    samples = []
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), img, 7)
        rows = np.load(tmp_path / str(k) / "image_rows.npy")
        got = np.load(tmp_path / str(k) / "image.npy")
        assert rows.dtype == np.float64 and len(rows) == 10 and np.all(np.diff(rows) > 0)
        assert np.array_equal(got, img[rows.astype(np.int64)])
        samples.append(rows)
    assert np.array_equal(samples[0], samples[1])                          # the same rows from run to run
    bench.dump_outputs(str(tmp_path / "0"), img[:5], 7)                    # a small frame into the same folder: no stale row list
    assert not (tmp_path / "0" / "image_rows.npy").exists()
