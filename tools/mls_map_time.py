"""Wall time of the height-cluster MLS map (slam_mls_*, docs/MLS_MAP.md) on graph_slam's 1000^2 map at 0.5 m:
one addToMap of a synth.make_cloud3d keyframe (map frame), the replay of K = 10 and K = 50 keyframes enqueued
on one stream (regenerateGlobalMap, graph_slam.cpp:260-280), the heaviest cell's point count, and the scalar
restatement's (tests/cpp/mls_map_oracle.cpp) single-thread CPU time on the same inputs.

    python tools/mls_map_time.py [--reps 5]
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

import mls_map_oracle as MO  # noqa: E402
from slam_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    api.set_device(0)
    kfs = [MO.keyframe_cloud(k) for k in range(50)]
    dev_clouds = [api.DeviceArray.from_host(c, np.float32) for c, _ in kfs]
    out = {"device": api.device_info()[0], "points_per_keyframe": int(len(kfs[0][0]))}
    # heaviest cell of keyframes 0 and 7 (the binning of mls.cpp:371-388 on the host, range gate included)
    heavy = []
    for k in (0, 7):
        c, (x, y, _) = kfs[k]
        cx = np.trunc(c[:, 0].astype(np.float64) / 0.5 + 500).astype(np.int64)
        cy = np.trunc(c[:, 1].astype(np.float64) / 0.5 + 500).astype(np.int64)
        ok = np.hypot(x - c[:, 0].astype(np.float64), y - c[:, 1].astype(np.float64)) <= 75
        _, n = np.unique(cx[ok] * 1000 + cy[ok], return_counts=True)
        heavy.append({"keyframe": k, "cells": int(len(n)), "mean_points": float(n.mean()), "heaviest": int(n.max())})
    out["binning"] = heavy
    st = api.Stream()
    m = api.MlsMap(1000, 1000, 0.5)
    # one addToMap, map as after the first keyframe
    t_one = []
    for r in range(a.reps):
        m.clear(st)
        for k in (0, 7):
            x, y, _ = kfs[k][1]
            m.set_pose(x, y)
            st.synchronize()
            t0 = time.perf_counter()
            m.add_cloud_dev(dev_clouds[k], len(kfs[k][0]), 3, st)
            st.synchronize()
            t_one.append((time.perf_counter() - t0) * 1e3)
    out["add_ms"] = {"median": float(np.median(t_one)), "min": float(np.min(t_one))}
    for K in (10, 50):
        ts = []
        for r in range(a.reps):
            st.synchronize()
            t0 = time.perf_counter()
            m.clear(st)
            for k in range(K):
                x, y, _ = kfs[k][1]
                m.set_pose(x, y)
                m.add_cloud_dev(dev_clouds[k], len(kfs[k][0]), 3, st)
            st.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["replay_%d_ms" % K] = {"median": float(np.median(ts)), "min": float(np.min(ts))}
    m.close()
    # the restatement, one thread
    ora = MO.OracleMls(1000, 1000, 0.5, api.mls_default_params())
    t_ora = []
    for k in range(50):
        c, (x, y, _) = kfs[k]
        ora.add_cloud(c, (x, y))
        t_ora.append(ora.last_seconds * 1e3)
    out["oracle_add_ms"] = {"median": float(np.median(t_ora)), "replay_10": float(np.sum(t_ora[:10])), "replay_50": float(np.sum(t_ora))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
