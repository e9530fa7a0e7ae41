"""Time of the voxel map and the map builder on the device (slam_vmap_*, slam_amd.api.GlobalMapBuilder, docs/VOXEL_MAP.md)
at 8 192 and 131 072 points per cloud (make_cloud3d with 16 rings x 512 azimuths and 64 x 2 048): integrating one resident
cloud into a map that holds five, extracting that map (whole, into resident arrays), and one add_cloud of the sixth
cloud; beside them the scalar restatement (tests/cpp/vmap_oracle.cpp) on one CPU thread for the integrate and the extract.

Every figure is the median / min / max of `--reps` (7) regions after a warm-up region.  integrate and extract: device
events around the region and the host clock around it; both calls wait once for their counters, so the host clock is the
figure a caller sees and the events bracket the same work.  A region integrates into a map restored beforehand outside
the region (clear + five clouds), so that every region does the same work.  add_cloud: the host clock only (it uploads,
filters, registers and waits several times); the builder's state is put back outside every region.  One JSON line.

    python tools/map_builder_time.py [--reps 7] [--no-cpu]
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
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1), (time.perf_counter() - t0) * 1e3


def measure(fn, reps, before=None):
    """reps regions of fn after one warm-up region; before() runs outside every region"""
    rows = []
    for _ in range(reps + 1):
        if before:
            before()
        rows.append(region(fn))
    ev, wall = zip(*rows[1:])
    return {"device": stats(ev), "wall": stats(wall)}


def truth_transforms(clouds):
    return [V.truth_in_first_frame(clouds[0][1], p) for _, p in clouds]


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
        T = truth_transforms(clouds)
        d_clouds = [api.DeviceArray.from_host(c) for c, _ in clouds]
        vm = api.VoxelMap()

        def restore():
            vm.clear()
            for k in range(5):
                vm.integrate_dev(d_clouds[k], n, 3, T[k][:3, :3], T[k][:3, 3])

        row = {}
        row["integrate_ms"] = measure(lambda: vm.integrate_dev(d_clouds[5], n, 3, T[5][:3, :3], T[5][:3, 3]), a.reps, before=restore)
        restore()
        info = vm.info()
        cap = info["n_voxels"]
        d_xyz4, d_count, d_key = api.DeviceArray((cap, 4), np.float32), api.DeviceArray((cap,), np.uint32), api.DeviceArray((cap,), np.uint64)
        row["extract_ms"] = measure(lambda: vm.extract_dev(d_xyz4, cap, d_count=d_count, d_key=d_key), a.reps)
        row["map"] = {k: info[k] for k in ("n_voxels", "capacity", "n_points", "device_bytes")}
        vm.close()

        # one add_cloud of the sixth cloud on a builder that holds five.  Built once; before every region the builder's
        # state (the map and trans_full) is put back from the recorded poses, which costs five integrations and no registration
        b = api.GlobalMapBuilder()
        poses = []
        for k in range(5):
            ok, _r = b.add_cloud(clouds[k][0])
            assert ok
            poses.append(b.pose().astype(np.float64))
        walls, last = [], None
        for _ in range(a.reps + 1):
            b.vmap.clear()
            for k in range(5):
                b.vmap.integrate_dev(d_clouds[k], n, 3, poses[k][:3, :3], poses[k][:3, 3])
            b.trans_full = poses[4].astype(np.float32)
            api.synchronize()
            t0 = time.perf_counter()
            ok, last = b.add_cloud(clouds[5][0])
            walls.append((time.perf_counter() - t0) * 1e3)
            assert ok
        b.close()
        row["add_cloud_ms"] = {"wall": stats(walls[1:])}
        row["add_cloud"] = {"iterations": last["iterations"], "state": last["state"], "fitness": last["fitness"]}

        if not a.no_cpu:
            om = V.OracleMap(0.30)
            cpu_int, cpu_ext = [], []
            for _ in range(a.reps + 1):
                om.clear()
                for k in range(5):
                    om.integrate(clouds[k][0], T[k][:3, :3], T[k][:3, 3])
                t0 = time.perf_counter()
                om.integrate(clouds[5][0], T[5][:3, :3], T[5][:3, 3])
                cpu_int.append((time.perf_counter() - t0) * 1e3)
            om.clear()
            for k in range(5):
                om.integrate(clouds[k][0], T[k][:3, :3], T[k][:3, 3])
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                om.extract()
                cpu_ext.append((time.perf_counter() - t0) * 1e3)
            row["cpu_one_thread_ms"] = {"integrate": stats(cpu_int[1:]), "extract": stats(cpu_ext[1:])}
        out[str(n)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
