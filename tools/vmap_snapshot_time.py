"""Time of the voxel map's absorb, merge, save and load (slam_vmap_absorb_dev .. slam_vmap_load, docs/VOXEL_MAP.md section 10)
on the two maps of tools/vmap_gicp_time.py: 1 m maps with moments that hold five clouds of 8 192 and of 131 072 points
(make_cloud3d with 16 rings x 512 azimuths and 64 x 2 048) at the truth transforms.

  absorb_dev_ms    the map's records (resident device arrays: keys, counts, sums, E, M) into an empty map of the same table
  merge_ms         the map into an empty map of the same table, straight from its slots
  save_ms          slam_vmap_save to a file in --dir (the three readers, then the write)
  load_ms          slam_vmap_load of that file (read, parse, create, enable, absorb) and the handle's destroy
  reintegrate_ms   the same five resident clouds integrated into an empty map of the same table: what stands in for a load or a
                   merge without this section

Every figure is the median / min / max of `--reps` (7) regions after a warm-up region: device events around the region and the
host clock around it (every call waits for its counters, so the host clock is what a caller sees; save and load are host work
for the most part).  The destination is cleared outside every region.  Asserts nothing about speed.  One JSON line.

    python tools/vmap_snapshot_time.py [--reps 7] [--dir DIR]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from map_builder_time import SIZES, measure, truth_transforms  # noqa: E402
from slam_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps}
    tmp = a.dir or tempfile.mkdtemp(prefix="vmap_snapshot_time_")
    for n, shape in SIZES.items():
        clouds = [synth.make_cloud3d(k, n_loop=50, **shape) for k in range(5)]
        assert all(len(c) == n for c, _ in clouds)
        T = truth_transforms(clouds)
        d_clouds = [api.DeviceArray.from_host(c) for c, _ in clouds]

        def integrate_all(vm):
            for k in range(5):
                vm.integrate_dev(d_clouds[k], n, 3, T[k][:3, :3], T[k][:3, 3])
        src = api.VoxelMap(leaf=1.0)
        src.enable_distributions()
        integrate_all(src)
        info = src.info()
        dst = api.VoxelMap(leaf=1.0, initial_capacity=info["capacity"])
        dst.enable_distributions()
        sums, count, key = src.read_sums()
        E, M, _ = src.read_moments()
        d = [api.DeviceArray.from_host(np.ascontiguousarray(x)) for x in (key, count, sums, E, M)]
        nv = len(key)
        row = {"map": {k: info[k] for k in ("n_voxels", "capacity", "n_points", "device_bytes")}}
        row["absorb_dev_ms"] = measure(lambda: dst.absorb_dev(d[0], d[1], d[2], nv, d_E3=d[3], d_M6=d[4]), a.reps, before=dst.clear)
        row["merge_ms"] = measure(lambda: dst.merge(src), a.reps, before=dst.clear)
        row["reintegrate_ms"] = measure(lambda: integrate_all(dst), a.reps, before=dst.clear)
        assert dst.info()["capacity"] == info["capacity"]          # nothing above grew the destination
        assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read_moments(), src.read_moments()))
        path = os.path.join(tmp, "map_%d.vmap" % n)
        row["save_ms"] = measure(lambda: src.save(path), a.reps)
        row["file_bytes"] = os.path.getsize(path)
        row["load_ms"] = measure(lambda: api.VoxelMap.load(path).close(), a.reps)
        os.remove(path)
        for m in (src, dst):
            m.close()
        out[str(n)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
