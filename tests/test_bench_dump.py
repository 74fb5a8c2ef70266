"""bench.py --dump-outputs without a GPU: the writer on stand-in contexts.  Files are float32 / float64, all of them stay
within the byte budget, an array that fits is written whole, a longer one as the same seeded sample of its rows in
every run."""
import os

import numpy as np

import bench
from reconstruction_amd.api import PairResult


class _Ctx:
    """What dump_outputs asks of a context: download_pair() with the arrays a caller receives."""

    def __init__(self, h, w, n, seed):
        rng = np.random.default_rng(seed)
        self.res = PairResult(disparity=[rng.standard_normal((h, w)) for _ in range(2)],
                              margin=[(1, 2, 3, 4, w, h), (5, 6, 7, 8, w, h)], n_points=n,
                              xyz=rng.standard_normal((n, 3)), bgr=rng.integers(0, 256, (n, 3), dtype=np.uint8), v_top=n // 2)

    def download_pair(self):
        return self.res


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_samples_long_arrays_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 52 * 1000)      # 500 rows per array for two pairs
    pairs = [(0, _Ctx(60, 80, 3000, 1)), (1, _Ctx(60, 80, 300, 2))]
    bench.dump_outputs(str(tmp_path / "a"), pairs, 2)
    bench.dump_outputs(str(tmp_path / "b"), pairs, 2)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted("pair%d_%s" % (p, n) for p in (0, 1) for n in ("disparity0", "disparity1", "xyz", "bgr", "info"))
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    payload = sum(v.nbytes for k, v in a.items() if not k.endswith("_info"))
    assert payload <= bench.DUMP_BYTES
    r0, r1 = pairs[0][1].res, pairs[1][1].res
    assert a["pair0_disparity0"].shape == (500,) and a["pair0_xyz"].shape == (500, 3)
    assert np.isin(a["pair0_disparity0"], r0.disparity[0]).all()
    assert np.array_equal(a["pair1_xyz"], r1.xyz) and np.array_equal(a["pair1_bgr"], r1.bgr.astype(np.float32))
    assert list(a["pair1_info"]) == [300, 150, 1, 2, 3, 4, 80, 60, 5, 6, 7, 8, 80, 60]


def test_dump_of_the_default_workload_stays_under_64_mb():
    """C2 (4096 x 3072), three pairs in flight: the rows kept per array times their bytes, plus the .npy headers."""
    h, w, n, pairs = 3072, 4096, 4096 * 3072, 3
    k = bench.DUMP_BYTES // pairs // (2 * 8 + 24 + 12)
    per_pair = 2 * 8 * min(k, h * w) + 24 * min(k, n) + 12 * min(k, n) + 14 * 8 + 5 * 128
    assert pairs * per_pair <= 64 * 1000 * 1000
