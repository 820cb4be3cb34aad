"""CPU: bench.py --dump-outputs writes a fixed, seeded sample of the state in float64, within 64 MB."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_the_same_sample_every_time(tmp_path):
    import bench
    n = 1000000
    rng = np.random.default_rng(3)
    uv, eta = rng.normal(size=(n, 3, 2)), rng.normal(size=(n, 3))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path/d), uv, eta)
    files = sorted(os.listdir(tmp_path/'a'))
    assert files == ['cells.npy', 'eta.npy', 'uv.npy'] == sorted(os.listdir(tmp_path/'b'))
    assert sum(os.path.getsize(tmp_path/'a'/f) for f in files) <= 64 << 20
    a = {f: np.load(tmp_path/'a'/f) for f in files}
    b = {f: np.load(tmp_path/'b'/f) for f in files}
    assert all(a[f].dtype == np.float64 and np.array_equal(a[f], b[f]) for f in files)
    cells = a['cells.npy'].astype(np.int64)
    assert len(cells) == bench.DUMP_CELLS and np.all(np.diff(cells) > 0) and cells[-1] < n
    assert np.array_equal(a['uv.npy'], uv[cells]) and np.array_equal(a['eta.npy'], eta[cells])
    # a state smaller than the sample is written whole
    bench.dump_outputs(str(tmp_path/'c'), uv[:100], eta[:100])
    assert np.array_equal(np.load(tmp_path/'c'/'eta.npy'), eta[:100])
