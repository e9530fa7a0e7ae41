"""Time of graph_slam's keyframe edges on the device (slam_kf_*, docs/KF_EDGE.md) on synth.make_cloud3d keyframes
(131 072 points each): adding a keyframe (voxel filter + search lattice), one edge, and four edges that share a source
in one call -- graph_slam's shape, KNN = 3 plus the previous keyframe -- with setup_gicp's settings, against the scalar
restatement (tests/cpp/kf_edge_oracle.cpp) on one CPU thread for the same edges.  The restatement stands in for PCL's
kd-tree ICP, which cannot be built here: its search is a hash lattice, not FLANN, so the CPU figure is a stand-in, not PCL's.

Device events around each call and the host clock around it (the call waits for its results), after a warm-up, median of
`--reps` regions of `--inner` calls each.

    python tools/kf_edge_time.py [--reps 7] [--inner 5]
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

import kf_edge_oracle as K  # noqa: E402
from slam_amd import api  # noqa: E402

KS = (0, 1, 2, 4, 8)       # the new keyframe is the last one; its edges go to the other four
SOURCE = 4


def region(fn, inner, stream=None):
    e0, e1 = api.Event(), api.Event()
    api.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    for _ in range(inner):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_ms(e1) / inner, (time.perf_counter() - t0) * 1e3 / inner


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    api.set_device(0)
    clouds = [K.cloud(k) for k in KS]
    out = {"device": api.device_info()[0], "points_per_keyframe": int(len(clouds[0][0]))}
    store = api.KeyframeStore()
    for c, _ in clouds:
        store.add_keyframe(c)
    out["keyframes"] = [store.info(i) for i in range(len(KS))]
    # add-keyframe: host cloud (upload included) and device-resident cloud, into a scratch store
    d_cloud = api.DeviceArray.from_host(clouds[SOURCE][0], np.float32)
    n = len(clouds[SOURCE][0])
    for name, fn in (("add_keyframe_ms", lambda s: s.add_keyframe(clouds[SOURCE][0])),
                     ("add_keyframe_dev_ms", lambda s: s.add_keyframe_dev(d_cloud, n, 3))):
        scratch = api.KeyframeStore()
        fn(scratch)
        fn(scratch)
        ev, wall = zip(*[region(lambda: fn(scratch), a.inner) for _ in range(a.reps)])
        out[name] = {"device": stats(ev), "wall": stats(wall)}
        scratch.close()
    poses = [p for _, p in clouds]
    edges = [(frm, SOURCE, K.relative_init(poses[frm], poses[SOURCE])) for frm in (0, 1, 2, 3)]
    res = store.register_edges(edges)           # warm-up
    store.register_edges(edges[:1])
    out["edges"] = [{"from": KS[e[0]], "to": KS[SOURCE], "iterations": r["iterations"], "state": r["state"], "pairs": r["pairs"]}
                    for e, r in zip(edges, res)]
    for name, batch in (("one_edge_ms", edges[:1]), ("four_edges_ms", edges)):
        ev, wall = zip(*[region(lambda: store.register_edges(batch), a.inner) for _ in range(a.reps)])
        out[name] = {"device": stats(ev), "wall": stats(wall)}
    # the same with the target's points read through L2 instead of staged in LDS (slam_kf_params.target_in_lds)
    store.set_params(target_in_lds=0)
    store.register_edges(edges)
    for name, batch in (("one_edge_l2_ms", edges[:1]), ("four_edges_l2_ms", edges)):
        ev, wall = zip(*[region(lambda: store.register_edges(batch), a.inner) for _ in range(a.reps)])
        out[name] = {"device": stats(ev), "wall": stats(wall)}
    store.set_params(target_in_lds=1)
    # the restatement on one CPU thread, same filtered clouds, same edges (index construction not counted)
    filtered = [store.read_keyframe(i)[:, :3] for i in range(len(KS))]
    ora = [K.OracleKeyframe(f, store.params) for f in filtered]
    per_edge = []
    for frm, to, init in edges:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            o = K.register_edge(ora[frm], filtered[to], init, params=store.params)
            ts.append((time.perf_counter() - t0) * 1e3)
        per_edge.append(float(np.median(ts)))
        assert o["iterations"] == res[frm]["iterations"], (frm, o["iterations"], res[frm]["iterations"])
    out["restatement_cpu_ms"] = {"per_edge": per_edge, "one_edge": per_edge[0], "four_edges": float(np.sum(per_edge))}
    out["speedup_four_edges_device_wall"] = out["restatement_cpu_ms"]["four_edges"] / out["four_edges_ms"]["wall"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
