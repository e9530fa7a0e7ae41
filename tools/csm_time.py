"""Time of the correlative scan matcher on the device (slam_csm_*, docs/CSM.md) at its defaults (0.1 m lattice, +-4 m,
+-1.2 rad in 0.01 rad steps: 241 x 81 x 81 candidates) on the synth room: the table build, one scan and a batch of
`--batch` scans, two-level and exhaustive, against the scalar restatement (tests/cpp/csm_oracle.cpp) on one CPU thread
for the same scans.  Every scan starts 3 m, -3 m, 1 rad off its true pose, where ICP alone is lost.

Device events around each region and the host clock around it, after a warm-up, median of `--reps` regions of `--inner`
calls each.  The inputs of a batch call are resident; the call is the asynchronous slam_csm_match_batch_dev.

    python tools/csm_time.py [--reps 7] [--inner 3] [--batch 256] [--no-cpu]

--post measures the posterior instead (docs/CSM.md section 6): slam_csm_match_batch_dev alone against
slam_csm_match_post_batch_dev on the same resident scans at the default post parameters, two-level, with the blocks each
evaluates at full resolution.  The difference of the two is the posterior's four kernels; for the split by kernel run it
once under `rocprofv3 --kernel-trace --stats -- python tools/csm_time.py --post --no-cpu`.
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

import csm_oracle as CO  # noqa: E402
from slam_amd import api  # noqa: E402


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


def resident_batch(cm, n_scans):
    """n_scans scans of the 256-pose loop on the device, each started BASIN_OFFSET off its truth"""
    cases = [CO.basin_case((k * 256) // n_scans if n_scans <= 256 else k % 256) for k in range(n_scans)]
    pts = np.ascontiguousarray(np.concatenate([np.concatenate([c[0], c[1]]) for c in cases]))
    off = np.cumsum([0] + [len(c[0]) + len(c[1]) for c in cases]).astype(np.int32)
    nga = np.array([len(c[0]) for c in cases], np.int32)
    R0, t0 = np.array([c[3].reshape(4) for c in cases]), np.array([c[4] for c in cases])
    cs = np.stack([cm.angles(r) for r in R0])
    d = [api.DeviceArray.from_host(x) for x in (pts, off, nga, R0, t0, cs)]
    d += [api.DeviceArray((n_scans, 4), np.float64), api.DeviceArray((n_scans, 2), np.float64),
          api.DeviceArray((n_scans,), api.CSM_RESULT_DTYPE)]
    return cases, d


def time_posterior(a, m_ga, m_nga, out):
    """match alone against match + posterior on the basin scans at the defaults"""
    cm = api.CorrelativeMatcher(m_ga, m_nga)
    cm.reserve(a.batch)
    cm.set_post_params()
    info = cm.info()
    n_blocks = info["n_theta"] * info["blocks_x"] * info["blocks_y"]
    out["info"] = {k: v for k, v in info.items() if k != "params"}
    for n_scans, name in ((1, "one_scan"), (a.batch, "batch_%d" % a.batch)):
        cases, d = resident_batch(cm, n_scans)
        d_post = api.DeviceArray((n_scans,), api.CSM_POST_DTYPE)

        def match():
            cm.match_batch_dev(d[0], d[1], d[2], n_scans, d[3], d[4], d[5], d[6], d[7], d[8])

        def match_post():
            cm.match_post_batch_dev(d[0], d[1], d[2], n_scans, d[3], d[4], d[5], d[6], d[7], d[8], d_post)

        row = {}
        for key, fn in (("match", match), ("match_post", match_post), ("match_again", match)):
            fn()
            ev, wall = zip(*[region(fn, a.inner) for _ in range(a.reps)])
            row[key + "_ms"] = {"device": stats(ev), "wall": stats(wall), "per_scan_device": float(np.median(ev)) / n_scans}
        res, post = d[8].download(), d_post.download()
        base = row["match_ms"]["device"]["median"]
        row["posterior_over_match"] = (row["match_post_ms"]["device"]["median"] - base) / base
        row["blocks_evaluated"] = {"match_median": float(np.median(res["blocks_evaluated"])), "match_max": int(res["blocks_evaluated"].max()),
                                   "posterior_median": float(np.median(post["blocks_evaluated"])),
                                   "posterior_max": int(post["blocks_evaluated"].max()), "of": n_blocks}
        row["n_within"] = {"median": float(np.median(post["n_within"])), "max": int(post["n_within"].max())}
        row["second_modes"] = int(np.count_nonzero(post["second_score"] >= 0))
        out["post_" + name] = row
    cm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--post", action="store_true")
    a = ap.parse_args()
    api.set_device(0)
    m_ga, m_nga = CO.synth_map()
    out = {"device": api.device_info()[0], "model_points": [len(m_ga), len(m_nga)]}

    if a.post:
        time_posterior(a, m_ga, m_nga, out)
        print(json.dumps(out))
        return

    def create():
        api.CorrelativeMatcher(m_ga, m_nga).close()

    create()
    ev, wall = zip(*[region(create, a.inner) for _ in range(a.reps)])
    out["create_ms"] = {"device": stats(ev), "wall": stats(wall)}      # upload, both tables at both levels, scratch, destroy
    cm = api.CorrelativeMatcher(m_ga, m_nga)
    cm.reserve(a.batch)
    info = cm.info()
    out["info"] = {k: v for k, v in info.items() if k != "params"}
    n_blocks = info["n_theta"] * info["blocks_x"] * info["blocks_y"]
    for n_scans, name in ((1, "one_scan"), (a.batch, "batch_%d" % a.batch)):
        cases, d = resident_batch(cm, n_scans)
        for ex, form in ((0, "two_level"), (1, "exhaustive")):
            cm.set_exhaustive(ex)
            inner = 1 if (ex and n_scans > 1) else a.inner
            reps = 3 if (ex and n_scans > 1) else a.reps

            def call():
                cm.match_batch_dev(d[0], d[1], d[2], n_scans, d[3], d[4], d[5], d[6], d[7], d[8])

            call()
            ev, wall = zip(*[region(call, inner) for _ in range(reps)])
            res = d[8].download()
            out["%s_%s_ms" % (name, form)] = {"device": stats(ev), "wall": stats(wall), "per_scan_device": float(np.median(ev)) / n_scans}
            if not ex:
                out["%s_blocks_evaluated" % name] = {"median": float(np.median(res["blocks_evaluated"])), "max": int(res["blocks_evaluated"].max()),
                                                     "of": n_blocks, "share_median": float(np.median(res["blocks_evaluated"])) / n_blocks}
                errs = [CO.pose_error(R, t, c[2]) for R, t, c in zip(d[6].download(), d[7].download(), cases)]
                out["%s_candidate_error" % name] = {"max_m": max(e[0] for e in errs), "max_rad": max(e[1] for e in errs)}
        cm.set_exhaustive(0)
    if not a.no_cpu:
        # the restatement on one CPU thread: table build, then one scan both ways (the exhaustive form once: seconds)
        t0 = time.perf_counter()
        om = CO.OracleMatcher(m_ga, m_nga)
        out["restatement_cpu_ms"] = {"create": (time.perf_counter() - t0) * 1e3}
        ga, nga, pose, R0, tt0 = CO.basin_case(0)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            om.match(ga, nga, R0, tt0)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["restatement_cpu_ms"]["one_scan_two_level"] = float(np.median(ts))
        t0 = time.perf_counter()
        om.match(ga, nga, R0, tt0, exhaustive=True)
        out["restatement_cpu_ms"]["one_scan_exhaustive"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
