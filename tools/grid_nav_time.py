"""Time of the occupancy grid's navigation field and path, slam_gnav_* (docs/GRID_NAV.md section 6).

  planes   e  plane (e) of docs/GRID_DIST.md section 5: the 2000 x 2000 grid at 0.05 m that config 2's raycast leaves at
              min_cluster_points 0, inflated at R = 32 by the distance field on the device (unknown cells stay closed)
           f  a 4000 x 4000 plane of random cost bytes 0 .. 252 with a tenth of the cells lethal
           o  a 4000 x 4000 open plane, cost 0 everywhere
           m  the serpentine maze of tests/grid_nav_cases.py scaled to 2000 x 2000
  goals    corner: the open cell nearest to (0, 0); middle: the open cell nearest to the plane's centre (the maze: corner only)

Per plane and goal, after the tools/grid_dist_time.py protocol (device events around regions, every region ending in a
synchronise; median / min / max of `--reps` (7) regions after a warm-up region):
  compute      the rounds and tiles processed the host form needed to converge, the device milliseconds of the same number of
               rounds enqueued at once by compute_dev on a plane that lies on the device, the wall milliseconds of the host form
               (which uploads the plane and waits once per batch of rounds), and the share of that wall time that is not device
               work: 1 - device / wall
  path         from the open cell furthest from the goal: its length and the device milliseconds of path_dev
  cpu          tests/cpp/grid_nav_oracle.cpp (scalar binary-heap Dijkstra, one thread, -O3) on this host, whose field the device's
               must equal ("equal"), and the wall milliseconds of the cost plane's read-back that it would need first
Asserts nothing about speed.  One JSON line.

One plane per call, each GPU step under a time limit of its own:

    timeout -k 10 600 python tools/grid_nav_time.py --plane e [--reps 7] [--no-cpu]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_nav_cases as N  # noqa: E402
from grid_dist_time import RES, raycast_grid  # noqa: E402
from map_builder_time import measure, stats  # noqa: E402
from slam_amd import api  # noqa: E402


def plane_e():
    grid, _, keep = raycast_grid(2000, 256, 0)
    df = api.DistanceField(2000, 2000, max_cells=32)
    df.set_inflation(RES, 0.3, 1.2, 3.0)
    grid.distance_field(df)
    cost = df.read()[1]
    df.close()
    grid.close()
    return 2000, cost


def nearest_open(cost, S, size, x, y):
    opn = np.flatnonzero(S[cost] != 0)
    i = opn[np.argmin((opn % size - x) ** 2 + (opn // size - y) ** 2)]
    return int(i % size), int(i // size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane", choices="efom", required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps, "plane": a.plane}
    if a.plane == "e":
        size, cost = plane_e()
    elif a.plane == "f":
        size, cost = 4000, N.random_plane(4000, 4000, 0.1, 0, 1)
    elif a.plane == "o":
        size, cost = 4000, N.plane(4000, 4000)
    else:
        size, cost = 2000, N.maze(2000, 2000)
    cells = size * size
    S = N.step_table()
    out.update(size=size, open_cells=int((S[cost] != 0).sum()))
    d_cost = api.DeviceArray.from_host(cost, np.uint8)
    back = np.empty(cells, np.uint8)
    walls = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        api.check(api.lib().slam_memcpy_d2h(back.ctypes.data, d_cost.ptr, cells, None))
        walls.append((time.perf_counter() - t0) * 1e3)
    out["cost_plane_readback_wall_ms"] = stats(walls[1:])
    goals = {"corner": nearest_open(cost, S, size, 0, 0)}
    if a.plane != "m":
        goals["middle"] = nearest_open(cost, S, size, size // 2, size // 2)
    nf = api.NavField(size, size)
    d_ls = api.DeviceArray((2,), np.int32)
    d_path = api.DeviceArray((cells, 2), np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        exe = None
        if not a.no_cpu:
            exe = os.path.join(tmp, "grid_nav_oracle")
            subprocess.check_call(["g++", "-std=c++17", "-O3", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "grid_nav_oracle.cpp"), "-o", exe])
            cost.tofile(os.path.join(tmp, "cost.u8"))
            S.tofile(os.path.join(tmp, "table.u32"))
        rows = {}
        for name, goal in goals.items():
            g = np.array([goal], np.int32)
            d_goals = api.DeviceArray.from_host(g)
            row = {"goal": goal}
            row["host_form_wall_ms"] = measure(lambda: nf.compute(cost, g), a.reps)["wall"]
            st = nf.state()
            assert st.converged == 1
            row.update(rounds=st.rounds, tiles_processed=st.tiles_processed, tiles=((size + N.TILE - 1) // N.TILE) ** 2)
            pot = nf.potential()
            row["compute_dev_ms"] = measure(lambda: nf.compute_dev(d_cost, d_goals, st.rounds), a.reps)["device"]
            assert nf.state().converged == 1 and np.array_equal(nf.potential(), pot)
            row["host_form_share_not_device"] = 1.0 - row["compute_dev_ms"]["median"] / row["host_form_wall_ms"]["median"]
            finite = np.flatnonzero(pot != N.FAR)
            start = finite[np.argmax(pot[finite])]
            start = (int(start % size), int(start // size))
            row["path_dev_ms"] = measure(lambda: nf.path_dev(start, cells, d_path, d_ls), a.reps)["device"]
            n, status = d_ls.download().tolist()
            row.update(path_start=start, path_length=n, path_status=status, reached_cells=int(len(finite)))
            if exe:
                g.tofile(os.path.join(tmp, "goals.i32"))
                o = os.path.join(tmp, "pot.u32")
                ms = subprocess.check_output([exe, os.path.join(tmp, "cost.u8"), str(size), str(size), os.path.join(tmp, "table.u32"), str(N.ORTH_W),
                                              str(N.DIAG_W), os.path.join(tmp, "goals.i32"), o, "3"], text=True, timeout=900)
                row["cpu_dijkstra_ms"] = [float(v) for v in ms.split()]
                row["equal"] = bool(np.array_equal(np.fromfile(o, np.uint32), pot))
            rows[name] = row
            d_goals.free()
        out["goals"] = rows
    nf.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
