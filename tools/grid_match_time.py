"""Times of the grid matcher (slam_amd.api.GridMatcher, docs/GRID_MATCH.md section 6) on the synth room.

  update   slam_grid_distance_field + slam_csm_set_plane_dev on one stream, 500 x 500 at 0.1 m (sigma 0.2 m, R 6) and
           2000 x 2000 at 0.05 m (sigma 0.2 m, R 12); the grid holds make_map()'s points as obstacles
  match    one scan at the matcher's default window (+-4 m, +-1.2 rad at 0.01 rad) against the plane-built handle of the
           500 x 500 grid, beside a model-built handle on the same room (two-level form, resident inputs,
           slam_csm_match_batch_dev); both start csm_oracle.BASIN_OFFSET off the truth.  With the bytes of their tables and the
           blocks each evaluates at full resolution: the plane's table is the whole window, the model's two the boxes of its classes
  scores   slam_csm_score_poses_dev at 4 096 poses x 1 081 points against the same plane

Measured as docs/GRID_DIST.md section 5 measures: device events around regions of `--calls` (10) calls, median / min / max of
`--reps` (7) regions after a warm-up region, every region ending in a synchronise; the figures are per call.  Asserts nothing
about speed.  One JSON line; run it twice for the spread between runs.

    timeout -k 10 300 python tools/grid_match_time.py [--reps 7] [--calls 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import csm_oracle as CO  # noqa: E402
from map_builder_time import measure  # noqa: E402
from slam_amd import api  # noqa: E402


def mapped_grid(size, res):
    m_ga, m_nga = CO.synth_map()
    g = api.Grid(size, size, res, min_cluster_points=0)
    g.add_endpoints(np.concatenate([m_ga, m_nga]).astype(np.float32), np.zeros((0, 2), np.float32))
    g.finalize()
    api.synchronize()
    return g


def per_call(t, calls):
    return {k: v / calls for k, v in t.items()}


def resident_scan(cm, k=96):          # a scan that keeps all 1 081 beams
    ga, nga, pose, R0, t0 = CO.basin_case(k)
    pts = np.ascontiguousarray(np.concatenate([ga, nga]))
    d = [api.DeviceArray.from_host(x) for x in (pts, np.array([0, len(pts)], np.int32), np.array([len(ga)], np.int32), R0.reshape(1, 4),
                                                t0.reshape(1, 2), cm.angles(R0)[None])]
    d += [api.DeviceArray((1, 4), np.float64), api.DeviceArray((1, 2), np.float64), api.DeviceArray((1,), api.CSM_RESULT_DTYPE)]
    return pose, pts, len(ga), d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps, "calls": a.calls}

    for size, res in ((500, 0.1), (2000, 0.05)):
        g = mapped_grid(size, res)
        gm = api.GridMatcher(g, 0.2)
        t = measure(lambda: [gm.update() for _ in range(a.calls)], a.reps)["device"]      # (the events' stream)
        out["update_%d_ms" % size] = dict(per_call(t, a.calls), max_cells=gm.max_cells, obstacles=int((g.read_occupancy() == 100).sum()))
        if size != 500:
            gm.close()
            g.close()
            continue
        # the match: plane-built beside model-built, the same scan, the default window
        m_ga, m_nga = CO.synth_map()
        model = api.CorrelativeMatcher(m_ga, m_nga)
        rows = {}
        for name, cm in (("plane_built", gm.matcher), ("model_built", model)):
            pose, pts, n_ga, d = resident_scan(cm)
            t = measure(lambda: [cm.match_batch_dev(d[0], d[1], d[2], 1, d[3], d[4], d[5], d[6], d[7], d[8]) for _ in range(a.calls)], a.reps)
            res_ = d[8].download()[0]
            info = cm.info()
            err = CO.pose_error(d[6].download()[0], d[7].download()[0], pose)
            rows[name] = dict(per_call(t["device"], a.calls), table_bytes=info["table_bytes"], blocks_evaluated=int(res_["blocks_evaluated"]),
                              blocks=info["n_theta"] * info["blocks_x"] * info["blocks_y"], score=int(res_["score"]),
                              max_score=int(res_["max_score"]), error_m=err[0], error_rad=err[1])
        out["match_ms"] = rows
        # the scorer: 4 096 poses about the truth
        rs = np.random.RandomState(7)
        n_poses = 4096
        poses = api.CorrelativeMatcher.poses(pose[2] + rs.uniform(-0.5, 0.5, n_poses), pose[0] + rs.uniform(-2, 2, n_poses),
                                             pose[1] + rs.uniform(-2, 2, n_poses))
        d_pts, d_poses = api.DeviceArray.from_host(pts), api.DeviceArray.from_host(poses)
        d_s, d_n = api.DeviceArray((n_poses,), np.int32), api.DeviceArray((n_poses,), np.int32)
        t = measure(lambda: [gm.matcher.score_poses_dev(d_pts, len(pts), n_ga, d_poses, n_poses, d_s, d_n) for _ in range(a.calls)], a.reps)
        s = d_s.download()
        out["score_poses_ms"] = dict(per_call(t["device"], a.calls), poses=n_poses, points=len(pts), best_share=float(s.max()) / (255.0 * len(pts)),
                                     pose_points_per_us=n_poses * len(pts) / (t["device"]["median"] / a.calls * 1e3))
        model.close()
        gm.close()
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
