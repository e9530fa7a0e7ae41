"""Times of the particle filter (slam_amd.api.ParticleFilter, docs/PARTICLE_FILTER.md section 7) on the synth room.

  step     slam_pf_predict_dev + slam_pf_update_dev on the null stream, 4 096, 65 536 and 262 144 particles x the 1 081 points of
           scan 96 against the likelihood plane of the 500 x 500 grid at 0.1 m (sigma 0.2 m, R 6); the particles start around the
           true pose and the motion is its noise alone (the scan stays), so the filter does what it does in use (`resamples` of `steps`)
  scorer   slam_csm_score_poses_dev alone over the same number of poses and the same scan: the scorer's share of the step
  predict  slam_pf_predict_dev alone

Measured as tools/grid_match_time.py measures: device events around regions of `--calls` (10) calls, median / min / max of
`--reps` (7) regions after a warm-up region, every region ending in a synchronise; the figures are per call.  Asserts nothing
about speed.  One JSON line; run it twice for the spread between runs.

    timeout -k 10 300 python tools/pf_time.py [--reps 7] [--calls 10]
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

from grid_match_time import mapped_grid, per_call  # noqa: E402
from map_builder_time import measure  # noqa: E402
from slam_amd import api, synth  # noqa: E402

SCAN, N_LOOP = 96, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--particles", type=int, nargs="*", default=[4096, 65536, 262144])
    a = ap.parse_args()
    api.set_device(0)
    out = {"device": api.device_info()[0], "reps": a.reps, "calls": a.calls}
    g = mapped_grid(500, 0.1)
    gm = api.GridMatcher(g, 0.2)
    gm.update()
    api.synchronize()
    ga, nga, pose = synth.make_scan(SCAN, N_LOOP)
    pts = np.ascontiguousarray(np.concatenate([ga, nga]))
    d_pts = api.DeviceArray.from_host(pts)
    motion = np.array([(0.0, 0.0, 0.03, 0.03, 3.0, 0)], api.PF_MOTION_DTYPE)       # noise alone: the scan stays the same from step to step
    d_m = api.DeviceArray.from_host(motion)
    for n in a.particles:
        pf = gm.particle_filter(n)
        A = pf.params.n_angles
        pf.init_gaussian(pose[0], pose[1], int(round(pose[2] / (2.0 * np.pi / A))) % A, 0.1, 0.1, 8.0)
        before = pf.state().n_resamples
        t_step = measure(lambda: [(pf.predict_dev(d_m), pf.update_dev(d_pts, len(pts), len(ga))) for _ in range(a.calls)], a.reps)
        s = pf.state()
        t_pred = measure(lambda: [pf.predict_dev(d_m) for _ in range(a.calls)], a.reps)
        x, y, k = pf.particles()
        cs = pf.tables()[0]
        d_poses = api.DeviceArray.from_host(np.stack([cs[2 * k], cs[2 * k + 1], x, y], axis=1))
        d_s, d_n = api.DeviceArray((n,), np.int32), api.DeviceArray((n,), np.int32)
        t_score = measure(lambda: [gm.matcher.score_poses_dev(d_pts, len(pts), len(ga), d_poses, n, d_s, d_n) for _ in range(a.calls)], a.reps)
        step_ms, score_ms = t_step["device"]["median"] / a.calls, t_score["device"]["median"] / a.calls
        out["particles_%d" % n] = dict(step_ms=per_call(t_step["device"], a.calls), predict_ms=per_call(t_pred["device"], a.calls),
                                       scorer_ms=per_call(t_score["device"], a.calls), scorer_share=score_ms / step_ms, points=len(pts),
                                       resamples=int(s.n_resamples - before), steps=(a.reps + 1) * a.calls,
                                       pose_points_per_us=n * len(pts) / (score_ms * 1e3))
        pf.close()
    gm.close()
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
