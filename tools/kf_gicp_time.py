"""Time of the keyframe store's Generalized ICP (slam_kf_compute_covariances, slam_kf_register_gicp, docs/KF_GICP.md) on
synth.make_cloud3d keyframes (131 072 points each, filtered at 0.5 m): the covariances of one keyframe, one request, four
requests that share a source, 20 starts of one source against one target in one call -- global_match.cpp's shape -- and
the same 20 as 20 single calls, against the scalar restatement (tests/cpp/kf_gicp_oracle.cpp) on one CPU thread for one
request and for the 20.  The restatement stands in for PCL's GICP, which cannot be built here: one Gauss-Newton step per
iteration instead of BFGS, a hash lattice instead of FLANN, so the CPU figure is a stand-in, not PCL's.

Device events around each call and the host clock around it (the call waits for its results), after a warm-up, median of
`--reps` regions of `--inner` calls each.

    python tools/kf_gicp_time.py [--reps 7] [--inner 5]
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
import kf_gicp_oracle as O  # noqa: E402
from slam_amd import api  # noqa: E402

KS = (0, 1, 2, 4, 8)       # the source is the last one; its requests go to the other four
SOURCE = 4
STARTS = 20


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


def timed(fn, reps, inner):
    ev, wall = zip(*[region(fn, inner) for _ in range(reps)])
    return {"device": stats(ev), "wall": stats(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    api.set_device(0)
    clouds = [K.cloud(k) for k in KS]
    poses = [p for _, p in clouds]
    out = {"device": api.device_info()[0], "points_per_keyframe": int(len(clouds[0][0]))}
    store = api.KeyframeStore()
    for c, _ in clouds:
        store.add_keyframe(c)
    out["keyframes"] = [store.info(i) for i in range(len(KS))]

    # covariances of one keyframe: a second call does nothing, so every timed call gets a store of its own
    ev, wall = [], []
    for _ in range(a.reps + 1):
        scratch = api.KeyframeStore()
        scratch.add_keyframe(clouds[SOURCE][0])
        e, w = region(lambda: scratch.compute_covariances(0), 1)
        ev.append(e), wall.append(w)
        scratch.close()
    out["covariances_ms"] = {"device": stats(ev[1:]), "wall": stats(wall[1:])}   # the first loads the code object

    edges = [(frm, SOURCE, K.relative_init(poses[frm], poses[SOURCE])) for frm in (0, 1, 2, 3)]
    rs = np.random.RandomState(4)
    starts = [(0, SOURCE, K.relative_init(poses[0], poses[SOURCE], (rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4), rs.uniform(-0.06, 0.06))))
              for _ in range(STARTS)]
    res = store.register_gicp(edges)            # warm-up; computes the covariances
    res20 = store.register_gicp(starts)
    out["requests"] = [{"from": KS[e[0]], "to": KS[SOURCE], "iterations": r["iterations"], "state": r["state"], "pairs": r["pairs"]}
                       for e, r in zip(edges, res)]
    out["starts_iterations"] = [r["iterations"] for r in res20]
    out["one_request_ms"] = timed(lambda: store.register_gicp(edges[:1]), a.reps, a.inner)
    out["four_requests_ms"] = timed(lambda: store.register_gicp(edges), a.reps, a.inner)
    out["twenty_starts_one_call_ms"] = timed(lambda: store.register_gicp(starts), a.reps, a.inner)
    out["twenty_starts_single_calls_ms"] = timed(lambda: [store.register_gicp([s]) for s in starts], a.reps, max(1, a.inner // 5))

    # the restatement on one CPU thread, same filtered clouds, same requests (covariances and index not counted)
    ora = [O.OracleCloud(store.read_keyframe(i)[:, :3], store.params) for i in range(len(KS))]

    def cpu(reqs):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = [O.register_gicp(ora[frm], ora[to], init) for frm, to, init in reqs]
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), got
    one, got1 = cpu(edges[:1])
    twenty, got20 = cpu(starts)
    assert got1[0]["iterations"] == res[0]["iterations"]
    assert [g["iterations"] for g in got20] == out["starts_iterations"]
    out["restatement_cpu_ms"] = {"one_request": one, "twenty_starts": twenty}
    batch = out["twenty_starts_one_call_ms"]["wall"]["median"]
    out["twenty_starts_single_calls_over_one_call"] = out["twenty_starts_single_calls_ms"]["wall"]["median"] / batch
    out["twenty_starts_cpu_over_one_call"] = twenty / batch
    print(json.dumps(out))


if __name__ == "__main__":
    main()
