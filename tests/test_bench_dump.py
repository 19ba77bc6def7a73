"""bench.py --dump-outputs on CPU: what dump_outputs writes for a pool of records (no GPU; the pool here is made up)."""
import glob
import os

import numpy as np

import bench
from mvskit_amd import synth


def fake_pool(n, list_cap):
    rng = np.random.default_rng(5)
    pool = np.zeros(n, synth.patch_dtype(64 if list_cap == 64 else 32))
    pool["coord"] = rng.normal(size=(n, 4))
    pool["ncc"] = rng.uniform(-1, 1, n)
    pool["nimages"] = rng.integers(0, list_cap + 1, n)
    pool["nvimages"] = rng.integers(0, list_cap + 1, n)
    pool["images"] = rng.integers(0, 255, pool["images"].shape)
    pool["vimages"] = rng.integers(0, 255, pool["vimages"].shape)
    pool["id"] = np.arange(n) * 3
    return pool


def read_dir(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}


def test_dump_of_a_small_pool_is_the_whole_pool(tmp_path):
    pool = fake_pool(1000, 16)
    counters = dict(zip(bench.COUNTER_NAMES, range(10, 20)))
    bench.dump_outputs(str(tmp_path), pool, counters, (0.65, 0.35, 2), 16)
    out = read_dir(str(tmp_path))
    assert {a.dtype for a in out.values()} <= {np.dtype(np.float32), np.dtype(np.float64)}
    np.testing.assert_array_equal(out["counters"], np.arange(10, 20))
    np.testing.assert_array_equal(out["thresholds"], np.array([0.65, 0.35, 2.0]))
    assert out["pool_size"][0] == 1000
    np.testing.assert_array_equal(out["pool_rows"], np.arange(1000))
    np.testing.assert_array_equal(out["pool_coord"], pool["coord"])
    np.testing.assert_array_equal(out["pool_ncc"], pool["ncc"])
    np.testing.assert_array_equal(out["pool_id"], pool["id"])
    assert out["pool_images"].shape == (1000, 16)
    for i in range(1000):
        k = pool["nimages"][i]
        np.testing.assert_array_equal(out["pool_images"][i, :k], pool["images"][i, :k])
        assert (out["pool_images"][i, k:] == -1).all()
        k = pool["nvimages"][i]
        np.testing.assert_array_equal(out["pool_vimages"][i, :k], pool["vimages"][i, :k])
        assert (out["pool_vimages"][i, k:] == -1).all()


def test_dump_of_a_large_pool_is_a_fixed_sample_within_64_mb(tmp_path):
    pool = fake_pool(1_500_000, 64)
    counters = dict(zip(bench.COUNTER_NAMES, range(10)), filter_removed={"outside": 1, "exact": 2, "neighbor": 3, "groups": 4})
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), pool, counters, (0.6, 0.3, 3), 64)
    a, b = read_dir(str(tmp_path / "a")), read_dir(str(tmp_path / "b"))
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 64 << 20
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    np.testing.assert_array_equal(a["filter_removed"], [1, 2, 3, 4])
    rows = a["pool_rows"].astype(np.int64)
    assert 0 < rows.shape[0] < pool.shape[0] and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(a["pool_coord"], pool["coord"][rows])
    np.testing.assert_array_equal(a["pool_id"], pool["id"][rows])
