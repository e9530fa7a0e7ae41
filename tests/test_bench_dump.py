"""bench.py --dump-outputs without a GPU: the arrays' types, and the fixed sample of the grid planes when the whole would
exceed the budget (run in a child: importing bench.py sets the HIP queue count of the process that imports it)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
bench.DUMP_BUDGET_BYTES = 1 << 20
ev = np.arange(1000 * 1000, dtype=np.float64).reshape(1000, 1000)
occ = (np.arange(1000 * 1000) % 3).astype(np.int8).reshape(1000, 1000)
for d in sys.argv[2:]:
    bench.dump_outputs(d, {"poses_t": np.ones((4, 2)), "icp_iters": np.full(4, 30, np.int32), "grid_evidence": ev,
                           "grid_occupancy": occ}, planes=("grid_evidence", "grid_occupancy"))
    bench.dump_outputs(d + "_small", {"poses_t": np.ones((4, 2)), "grid_occupancy": occ[:10]}, planes=("grid_occupancy",))
"""


def test_dump_outputs_types_budget_and_fixed_sample(tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + dirs, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = []
    for d in dirs:
        a = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
        assert sorted(a) == ["grid_evidence", "grid_occupancy", "grid_sample_cells", "icp_iters", "poses_t"]
        assert sum(v.nbytes for v in a.values()) <= 1 << 20
        assert a["poses_t"].dtype == np.float64 and a["icp_iters"].dtype == np.float64 and (a["icp_iters"] == 30).all()
        assert a["grid_evidence"].dtype == np.float64 and a["grid_occupancy"].dtype == np.float32
        idx = a["grid_sample_cells"].astype(np.int64)
        assert len(idx) > 1000 and (np.diff(idx) > 0).all() and idx[-1] < 1000 * 1000
        assert np.array_equal(a["grid_evidence"], idx.astype(np.float64))        # the planes keep the sampled cells
        assert np.array_equal(a["grid_occupancy"], (idx % 3).astype(np.float32))
        small = {f[:-4]: np.load(os.path.join(d + "_small", f)) for f in os.listdir(d + "_small")}
        assert sorted(small) == ["grid_occupancy", "poses_t"] and small["grid_occupancy"].shape == (10, 1000)
        got.append(a)
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k
