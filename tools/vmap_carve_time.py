"""Time of one free-space carve on the device (slam_vmap_carve_dev, docs/VOXEL_MAP.md section 8) at 8 192 and 131 072 points
per cloud (make_cloud3d with 16 rings x 512 azimuths and 64 x 2 048, the clouds of docs/VOXEL_MAP.md section 7): a map that
holds six clouds at the truth transforms, the sixth carved; beside it the scalar restatement
(tests/cpp/vmap_carve_oracle.cpp) on one CPU thread.

Every figure is the median / min / max of `--reps` (7) regions after a warm-up region: device events around the call and
the host clock around it (the call waits once for its counters, so the host clock is what a caller sees and the events
bracket the same work).  A carve changes seen and miss only, and by the same amounts every time, so the regions do the same
work without the map being restored.  One JSON line.

    python tools/vmap_carve_time.py [--reps 7] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vmap_carve_oracle as VC  # noqa: E402
import vmap_oracle as V  # noqa: E402
from slam_amd import api, synth  # noqa: E402

SIZES = {8192: dict(rings=16, n_az=512), 131072: dict(rings=64, n_az=2048)}


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def region(fn):
    e0, e1 = api.Event(), api.Event()
    api.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1), (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps}
    for n, shape in SIZES.items():
        clouds = [synth.make_cloud3d(k, n_loop=50, **shape) for k in range(6)]
        assert all(len(c) == n for c, _ in clouds)
        T = [V.truth_in_first_frame(clouds[0][1], p) for _, p in clouds]
        d_last = api.DeviceArray.from_host(clouds[5][0])
        vm = api.VoxelMap()
        for (c, _), Tk in zip(clouds, T):
            vm.integrate(c, Tk[:3, :3], Tk[:3, 3])
        rows = [region(lambda: vm.carve_dev(d_last, n, 3, T[5][:3, :3], T[5][:3, 3])) for _ in range(a.reps + 1)]
        assert all(r[2] == rows[0][2] for r in rows)
        info = vm.info()
        row = {"carve_ms": {"device": stats([r[0] for r in rows[1:]]), "wall": stats([r[1] for r in rows[1:]])}, "counters": rows[0][2],
               "map": {k: info[k] for k in ("n_voxels", "capacity", "n_points", "device_bytes")}}
        vm.close()
        if not a.no_cpu:
            om = VC.CarveOracleMap(0.30)
            for (c, _), Tk in zip(clouds, T):
                om.integrate(c, Tk[:3, :3], Tk[:3, 3])
            cpu = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                r = om.carve(clouds[5][0], T[5][:3, :3], T[5][:3, 3])
                cpu.append((time.perf_counter() - t0) * 1e3)
            assert r == rows[0][2], (r, rows[0][2])
            row["cpu_one_thread_ms"] = {"carve": stats(cpu[1:])}
        out[str(n)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
