"""Time of the scan-context descriptor and search on the device (slam_kf_sc_*, docs/SCAN_CONTEXT.md) against the number of
keyframes, beside the scalar restatement (tests/cpp/sc_oracle.cpp) on one CPU thread.  The keyframes are the 48 clouds of
the synthetic loop (32 rings x 512 azimuths, about 3 900 points behind the 0.5 m filter), repeated; default parameters
but max_range = 40 m.

Every timed call waits for its own work (the entry points synchronise), so the host clock around a call is the call.
After a warm-up call of the same shape, the median of `--reps` calls.  The descriptor of N keyframes is one
slam_kf_sc_compute(-1) on a fresh store each time (descriptors cannot be dropped); the search is slam_kf_sc_match.

    python tools/kf_sc_time.py [--reps 7] [--counts 100,1000] [--no-cpu]
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

import sc_oracle as SO  # noqa: E402
from slam_amd import api, synth  # noqa: E402

MAX_RANGE = 40.0


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def fresh_store(clouds, n):
    store = api.KeyframeStore()
    store.set_sc_params(max_range=MAX_RANGE)
    for k in range(n):
        store.add_keyframe(clouds[k % len(clouds)])
    return store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--counts", default="100,1000")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    api.set_device(0)
    clouds = [synth.make_cloud3d(k, 48, rings=32, n_az=512)[0] for k in range(48)]
    out = {"device": api.device_info()[0], "max_range": MAX_RANGE}
    fresh_store(clouds, 2).sc_compute()                  # code objects loaded
    store = None
    for n in [int(v) for v in a.counts.split(",")]:
        ts = []
        for _ in range(max(3, a.reps if n <= 100 else 3)):
            store = fresh_store(clouds, n)
            ts.append(timed(store.sc_compute))
        r = {"descriptors_ms": stats(ts), "descriptor_us_per_keyframe": float(np.median(ts)) * 1e3 / n,
             "filtered_points": store.info(0)["n_points"]}
        store.sc_match([n - 1])
        r["one_query_ms"] = stats([timed(lambda: store.sc_match([n - 1])) for _ in range(a.reps)])
        everyone = np.arange(n, dtype=np.int32)
        store.sc_match(everyone)
        ts = [timed(lambda: store.sc_match(everyone)) for _ in range(a.reps)]
        r["all_pairs_ms"] = stats(ts)
        r["all_pairs_ns_per_pair"] = float(np.median(ts)) * 1e6 / (n * n)
        out["keyframes_%d" % n] = r
    if not a.no_cpu:
        p = SO.Params(max_range=MAX_RANGE)
        tabs = store.sc_tables()
        filtered = [store.read_keyframe(k)[:, :3] for k in range(4)]
        SO.descriptor(filtered[0], p, tabs)
        d = [SO.descriptor(f, p, tabs) for f in filtered]
        cpu = {"descriptor_us_per_keyframe": 1e3 * float(np.median([timed(lambda f=f: SO.descriptor(f, p, tabs)) for f in filtered * 3])),
               "match_us_per_pair": 1e3 * float(np.median([timed(lambda: SO.match(d[0], d[1 + k % 3])) for k in range(15)]))}
        assert np.array_equal(d[0], store.sc_read(0))
        out["restatement_one_cpu_thread"] = cpu
    print(json.dumps(out))


if __name__ == "__main__":
    main()
