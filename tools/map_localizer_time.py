"""Time of slam_vmap_coarsen and of slam_amd.api.MapLocalizer (docs/VOXEL_MAP.md section 11).

  coarsen_ms[k]     level k - 1 into an empty level k (k = 1, 2, 3: leaves 2, 4 and 8 from a 1 m map with moments), on the two
                    maps of tools/vmap_snapshot_time.py: five clouds of 8 192 and of 131 072 points at the truth transforms
  reintegrate_ms[k] the same five resident clouds integrated into an empty map of level k's leaf: what stands in for a
                    coarsen without this section
  localize_ms       case A of tests/map_localizer_cases.py (the 8 192-point scene, a fan of eight from 9.7 m and 2.78 rad
                    off, four levels): one MapLocalizer.localize, the derived levels standing
  set_map_ms        MapLocalizer.set_map of the fine map: three creates, three enables, three coarsens
  global_match_ms   for context only: GlobalMatcher.match of the same scan from the same wrong pose on
                    VoxelMap.read() -> set_map, the path docs/VOXEL_MAP.md section 10.5 gives (20 random starts through the
                    keyframe store); GlobalMatcher is untouched by section 11, so this is the parent commit's figure

Every figure is the median / min / max of `--reps` (7) regions after a warm-up region: device events around the region and the
host clock around it (every call waits for its results, so the host clock is what a caller sees).  Asserts nothing about
speed.  One JSON line.

    python tools/map_localizer_time.py [--reps 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import map_localizer_cases as ML  # noqa: E402
import vmap_oracle as V  # noqa: E402
from map_builder_time import SIZES, measure, truth_transforms  # noqa: E402
from slam_amd import api, synth  # noqa: E402


def dist_map(leaf, **kw):
    m = api.VoxelMap(leaf=leaf, **kw)
    m.enable_distributions()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps}
    for n, shape in SIZES.items():
        clouds = [synth.make_cloud3d(k, n_loop=50, **shape) for k in range(5)]
        assert all(len(c) == n for c, _ in clouds)
        T = truth_transforms(clouds)
        d_clouds = [api.DeviceArray.from_host(c) for c, _ in clouds]

        def integrate_all(vm):
            for k in range(5):
                vm.integrate_dev(d_clouds[k], n, 3, T[k][:3, :3], T[k][:3, 3])
        levels = [dist_map(1.0)]
        integrate_all(levels[0])
        row = {"levels": [], "coarsen_ms": [], "reintegrate_ms": []}
        for k in range(1, 4):
            dst = dist_map(2.0 ** k)
            row["coarsen_ms"].append(measure(lambda: dst.coarsen(levels[k - 1]), a.reps, before=dst.clear))
            direct = dist_map(2.0 ** k)
            row["reintegrate_ms"].append(measure(lambda: integrate_all(direct), a.reps, before=direct.clear))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read_moments(), direct.read_moments()))
            direct.close()
            levels.append(dst)
        row["levels"] = [{f: m.info()[f] for f in ("n_voxels", "capacity", "n_points")} for m in levels]
        for m in levels:
            m.close()
        out[str(n)] = row

    parts, cloud, truth = ML.scene()
    fine = dist_map(ML.LEAF)
    for c, Tk in parts:
        fine.integrate(c, Tk[:3, :3], Tk[:3, 3])
    loc = api.MapLocalizer(levels=ML.CASE_A["levels"])
    starts = ML.starts_of(ML.CASE_A, truth)
    res = {"set_map_ms": measure(lambda: loc.set_map(fine), a.reps)}
    ans = []
    res["localize_ms"] = measure(lambda: ans.append(loc.localize(cloud, starts)), a.reps)
    r = ans[-1]
    e = V.pose_error(r["transform"], truth) if r["found"] else (float("nan"), float("nan"))
    res["localize"] = dict(found=r["found"], index=r["index"], n_source=r["n_source"], error_mm=e[0] * 1e3, error_mrad=e[1] * 1e3,
                           iterations=[[None if x is None else x["iterations"] for x in lv] for lv in r["last"]],
                           fitness=[None if x is None else x["fitness"] for x in r["last"][0]],
                           fitness_pairs=[None if x is None else x["fitness_pairs"] for x in r["last"][0]])
    x, y, yaw = (float(v) for v in ML.start_pose(ML.CASE_A, truth))
    matcher = api.GlobalMatcher()
    matcher.set_map(fine.read()[0])
    edges = []
    res["global_match_ms"] = measure(lambda: edges.append(matcher.match(cloud, x, y, yaw)), a.reps)
    g = edges[-1]
    res["global_match"] = dict(matched=bool(g and g["matched"]), matches=sum(1 for q in edges if q and q["matched"]), calls=len(edges))
    if g and g["matched"]:
        ge = V.pose_error(g["refined"], truth)
        res["global_match"].update(start=g["start"], error_mm=ge[0] * 1e3, error_mrad=ge[1] * 1e3)
    out["case_A"] = res
    matcher.close()
    loc.close()
    fine.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
