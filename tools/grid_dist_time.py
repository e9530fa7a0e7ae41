"""Time of slam_gdist_compute_dev, the occupancy grid's distance field and costmap (docs/GRID_DIST.md section 5).

  planes   a  the 2000 x 2000 grid at 0.05 m that config 2's raycast of synth.make_batch (256 scans at their initial poses,
              min_cluster_points 20) leaves after finalize
           b  the same at 4000 x 4000 (config 4's grid, 1024 scans)
           c  a 4000 x 4000 empty plane
           d  a 4000 x 4000 plane with 50 % random obstacles
           e  plane a's raycast with min_cluster_points 0: every cell a beam ended in is an obstacle (plane a itself holds none
              at the node's threshold of 20 hits, docs/GRID_DIST.md section 5)
  R        8, 32, 128, 254, each with the inflation table set (the cost plane is written too)

Per plane and R: device milliseconds of one compute_dev (median / min / max of `--reps` (7) regions of `--calls` (10) calls each
after a warm-up region: device events around the region, every region ending in a synchronise; the figures are per call), the
algorithmic GB/s at 4 bytes per cell (1 read, 2 + 1 written) and its share of the 6.29 TB/s copy peak, and beside them the milliseconds of tests/cpp/grid_dist_oracle.cpp (the same
definition as scalar C++, one thread, -O3) on the same plane on this host -- whose dist2 plane the device's must equal ("equal").
For planes a, b and e also slam_grid_finalize on the same grid, the raycast that dirties its rows outside the region.
Asserts nothing about speed.  One JSON line.

One plane per call, each GPU step under a time limit of its own:

    timeout -k 10 600 python tools/grid_dist_time.py --plane a [--reps 7] [--no-cpu]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from map_builder_time import measure  # noqa: E402
from slam_amd import api, synth  # noqa: E402

RADII = (8, 32, 128, 254)
RES = 0.05
COPY_PEAK_GBS = 6290.0


def raycast_grid(size, scans, min_cluster_points=20):
    batch = synth.make_batch(scans, n_loop=scans)
    g = api.Grid(size, size, RES, rolling=0, min_cluster_points=min_cluster_points)
    d = [api.DeviceArray.from_host(a, dt) for a, dt in
         ((batch.pts, np.float64), (batch.scan_off, np.int32), (batch.R, np.float64), (batch.t, np.float64))]

    def cast():
        g.reset_counts()
        g.raycast_scans_dev(d[0], d[1], batch.n_scans, batch.n_points, d[2], d[3])
    cast()
    g.finalize()
    api.synchronize()
    return g, cast, d


def oracle_exe(tmp):
    exe = os.path.join(tmp, "grid_dist_oracle")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "grid_dist_oracle.cpp"), "-o", exe])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane", choices="abcde", required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10, help="compute_dev calls per timed region (the figures are per call)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--radii", type=int, nargs="*", default=list(RADII))
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps, "calls": a.calls, "plane": a.plane}
    grid = None
    if a.plane in "abe":
        size, scans = (4000, 1024) if a.plane == "b" else (2000, 256)
        grid, cast, keep = raycast_grid(size, scans, 0 if a.plane == "e" else 20)
        occ = grid.read_occupancy()
        out["finalize_ms"] = measure(lambda: grid.finalize(), a.reps, before=cast)["device"]
    else:
        size = 4000
        occ = np.zeros(size * size, np.int8)
        if a.plane == "d":
            occ[np.random.RandomState(1).rand(size * size) < 0.5] = 100
    cells = size * size
    out.update(size=size, obstacles=int((occ == 100).sum()), unknown=int((occ == -1).sum()))
    d_occ = api.DeviceArray.from_host(occ, np.int8)
    with tempfile.TemporaryDirectory() as tmp:
        exe = None
        if not a.no_cpu:
            exe = oracle_exe(tmp)
            occ.tofile(os.path.join(tmp, "occ.i8"))
        rows = {}
        for R in a.radii:
            df = api.DistanceField(size, size, max_cells=R)
            df.set_inflation(RES, min(0.3, R * RES / 2), min(1.2, R * RES), 3.0)
            t = measure(lambda: [df.compute_dev(d_occ) for _ in range(a.calls)], a.reps)["device"]
            t = {k: v / a.calls for k, v in t.items()}
            gbs = 4.0 * cells / (t["median"] * 1e-3) / 1e9
            row = {"device_ms": t, "algorithmic_gbs": gbs, "share_of_copy_peak": gbs / COPY_PEAK_GBS}
            dist2 = df.read()[0]
            row["far_cells"] = int((dist2 == api.GDIST_FAR).sum())
            if exe:
                o = os.path.join(tmp, "dist2.u16")
                ms = subprocess.check_output([exe, os.path.join(tmp, "occ.i8"), str(size), str(size), str(R), "0", o], text=True, timeout=900)
                row["cpu_scalar_ms"] = [float(v) for v in ms.split()]
                row["equal"] = bool(np.array_equal(np.fromfile(o, np.uint16), dist2))
            rows[str(R)] = row
            df.close()
        out["compute_dev"] = rows
    if grid is not None:
        grid.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
