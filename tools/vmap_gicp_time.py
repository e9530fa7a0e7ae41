"""Time of the voxel map's distributions and of the registration against them (slam_vmap_enable_distributions ..
slam_vmap_register_gicp, docs/VOXEL_MAP.md section 9) at the cloud sizes of tools/map_builder_time.py: 8 192 and 131 072
points per cloud (make_cloud3d with 16 rings x 512 azimuths and 64 x 2 048).

  integrate_ms           one resident cloud into a 1 m map that holds five, with the moments and without (two maps, same run)
  distributions_ms       slam_vmap_compute_distributions on the map of six (made stale outside the region by a clear + refill)
  register_ms            one slam_vmap_register_gicp of the sixth cloud's keyframe from the fifth pose (covariances computed
                         outside the region)
  add_cloud_ms           one add_cloud of the sixth cloud on a builder that holds five, `direct` on and off in the same run

Every figure is the median / min / max of `--reps` (7) regions after a warm-up region: device events around the region and
the host clock around it for the first three (each call waits for its counters or results, so the host clock is what a
caller sees), the host clock only for add_cloud.  State is put back outside every region.  Asserts nothing about speed.
One JSON line.

    python tools/vmap_gicp_time.py [--reps 7]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import vmap_oracle as V  # noqa: E402
from map_builder_time import SIZES, measure, stats, truth_transforms  # noqa: E402
from slam_amd import api, synth  # noqa: E402


def add_cloud_times(clouds, d_clouds, n, reps, direct):
    """as tools/map_builder_time.py: built once, the state put back from the recorded poses before every region"""
    b = api.GlobalMapBuilder(direct=direct)
    poses = []
    for k in range(5):
        ok, _r = b.add_cloud(clouds[k][0])
        assert ok
        poses.append(b.pose().astype(np.float64))
    walls, last = [], None
    for _ in range(reps + 1):
        for m in b._maps():
            m.clear()
            for k in range(5):
                m.integrate_dev(d_clouds[k], n, 3, poses[k][:3, :3], poses[k][:3, 3])
        if direct:
            b.dmap.compute_distributions()      # a builder in use has them from the last registration's call
        b.trans_full = poses[4].astype(np.float32)
        api.synchronize()
        t0 = time.perf_counter()
        ok, last = b.add_cloud(clouds[5][0])
        walls.append((time.perf_counter() - t0) * 1e3)
        assert ok
    b.close()
    return {"wall": stats(walls[1:]), "iterations": last["iterations"], "state": last["state"], "fitness": last["fitness"],
            "pairs": last["pairs"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps}
    for n, shape in SIZES.items():
        clouds = [synth.make_cloud3d(k, n_loop=50, **shape) for k in range(6)]
        assert all(len(c) == n for c, _ in clouds)
        T = truth_transforms(clouds)
        d_clouds = [api.DeviceArray.from_host(c) for c, _ in clouds]
        row = {}
        maps = {"plain": api.VoxelMap(leaf=1.0), "moments": api.VoxelMap(leaf=1.0)}
        maps["moments"].enable_distributions()
        for name, vm in maps.items():
            def restore(vm=vm, upto=5):
                vm.clear()
                for k in range(upto):
                    vm.integrate_dev(d_clouds[k], n, 3, T[k][:3, :3], T[k][:3, 3])
            row.setdefault("integrate_ms", {})[name] = measure(
                lambda vm=vm: vm.integrate_dev(d_clouds[5], n, 3, T[5][:3, :3], T[5][:3, 3]), a.reps, before=restore)
        vm = maps["moments"]

        def stale():
            vm.clear()
            for k in range(6):
                vm.integrate_dev(d_clouds[k], n, 3, T[k][:3, :3], T[k][:3, 3])
        row["distributions_ms"] = measure(lambda: vm.compute_distributions(), a.reps, before=stale)
        info = vm.info()
        row["map"] = {k: info[k] for k in ("n_voxels", "capacity", "n_points", "device_bytes")}
        row["map"]["plane_voxels"] = int(vm.read_distributions()["flag"].sum())

        store = api.KeyframeStore(leaf_size=0.30, gate=2.0, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
        kid = store.add_keyframe_dev(d_clouds[5], n, 3)
        store.compute_covariances(kid)
        vm.clear()
        for k in range(5):
            vm.integrate_dev(d_clouds[k], n, 3, T[k][:3, :3], T[k][:3, 3])
        vm.compute_distributions()
        init = T[4].astype(np.float32)
        res = []
        row["register_ms"] = measure(lambda: res.append(vm.register_gicp(store, kid, init, gate=2.0, max_iterations=100,
                                                                         transformation_epsilon=1e-6)), a.reps)
        r = res[-1]
        row["register"] = {"source_points": store.info(kid)["n_points"], "iterations": r["iterations"], "state": r["state"], "pairs": r["pairs"],
                           "fitness": r["fitness"], "error_mm_mrad": [1e3 * e for e in V.pose_error(r["transform"], T[5])]}
        store.close()
        for m in maps.values():
            m.close()
        row["add_cloud_ms"] = {"direct": add_cloud_times(clouds, d_clouds, n, a.reps, True),
                               "keyframe": add_cloud_times(clouds, d_clouds, n, a.reps, False)}
        out[str(n)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
