"""Time of slam_vmap_search_dev and of slam_amd.api.MapLocalizer.relocalize (docs/VOXEL_MAP.md section 13).

  search_ms[leaf][window][n]  one search with plane voxels and 64 yaws of a resident source of n points (3 730: cloud 5 of the
                              scene through the store's filter at 0.30; 16 384: the first 16 384 points of a 131 072-point cloud
                              of the same trajectory) against the scene's map at leaf 1, 2 and 4, windows of 24 and 125 cells
                              around the map's centre; the hits are fetched, the volume stays on the device
  relocalize_ms               MapLocalizer.relocalize on the scene from no prior (two levels, the window over the whole map),
                              next to localize_ms: case A of tests/map_localizer_cases.py, as tools/map_localizer_time.py has it

Every figure is the median / min / max of `--reps` (7) regions after a warm-up region: device events around the region and the
host clock around it (every call waits for its results, so the host clock is what a caller sees).  Asserts nothing about
speed.  One JSON line.

The three kernels separately: `--one LEAF WINDOW N` runs that one shape `--reps` times and nothing else, for a kernel trace
of its own (rocprofv3 --kernel-trace --stats -- python tools/vmap_search_time.py --one 1 24 3730).

    python tools/vmap_search_time.py [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import map_localizer_cases as ML  # noqa: E402
import vmap_oracle as V  # noqa: E402
from map_builder_time import measure  # noqa: E402
from slam_amd import api, synth  # noqa: E402

LEAVES, WINDOWS, SOURCES = (1.0, 2.0, 4.0), (24, 125), (3730, 16384)


def centre(m):
    x, y, _ = V.cells_of(m.read_sums()[2])
    leaf = m.params.leaf
    return float(np.float32((x.min() + x.max() + 1) * leaf / 2)), float(np.float32((y.min() + y.max() + 1) * leaf / 2)), \
        int(max(x.max() - x.min(), y.max() - y.min()) + 2) // 2 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--one", nargs=3, metavar=("LEAF", "WINDOW", "N"))
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps}
    parts, cloud, truth = ML.scene()
    fine = api.VoxelMap(leaf=ML.LEAF)
    fine.enable_distributions()
    for c, T in parts:
        fine.integrate(c, T[:3, :3], T[:3, 3])
    loc = api.MapLocalizer(levels=3)
    loc.set_map(fine)
    store = api.KeyframeStore(leaf_size=ML.STORE_LEAF, gate=2.0)
    kid = store.add_keyframe(cloud)
    big = synth.make_cloud3d(5, n_loop=50, rings=64, n_az=2048)[0][:16384]
    src = {3730: np.ascontiguousarray(store.read_keyframe(kid)[:, :3]), 16384: np.ascontiguousarray(big[:, :3], np.float32)}
    d_src = {n: api.DeviceArray.from_host(s) for n, s in src.items()}
    out["sources"] = {str(n): len(s) for n, s in src.items()}

    def one(level, w, n, reps):
        m = loc.level(level)
        cx, cy, _ = centre(m)
        p = api.vmap_default_search_params(cx=cx, cy=cy, wx=w, wy=w)
        hits = []
        t = measure(lambda: hits.append(m.search(d_xyz=d_src[n].ptr, n=len(src[n]), stride=3, params=p)[0]), reps)
        h = hits[-1][0]
        t.update(poses=64 * (2 * w + 1) ** 2, score=h["score"], n_with_cell=h["n_with_cell"], offset=list(V.pose_error(h["init"], truth)))
        return t

    if a.one:
        leaf, w, n = float(a.one[0]), int(a.one[1]), int(a.one[2])
        out["one"] = one(LEAVES.index(leaf), w, n, a.reps)
        print(json.dumps(out))
        return
    out["search_ms"] = {str(leaf): {str(w): {str(n): one(k, w, n, a.reps) for n in SOURCES} for w in WINDOWS} for k, leaf in enumerate(LEAVES)}

    two = api.MapLocalizer(levels=2)
    two.set_map(fine)
    cx, cy, w = centre(two.level(1))
    ans = []
    res = {"relocalize_ms": measure(lambda: ans.append(two.relocalize(cloud, cx, cy, 0.0, 2.0 * w)), a.reps)}
    r = ans[-1]
    e = V.pose_error(r["transform"], truth) if r["found"] else (float("nan"), float("nan"))
    res["relocalize"] = dict(found=r["found"], index=r["index"], n_source=r["n_source"], window_cells=w, error_mm=e[0] * 1e3, error_mrad=e[1] * 1e3,
                             hit_scores=[h["score"] for h in r["hits"]])
    four = api.MapLocalizer(levels=ML.CASE_A["levels"])
    four.set_map(fine)
    starts = ML.starts_of(ML.CASE_A, truth)
    res["localize_ms"] = measure(lambda: four.localize(cloud, starts), a.reps)
    out["scene"] = res
    for x in (two, four, loc):
        x.close()
    store.close()
    fine.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
