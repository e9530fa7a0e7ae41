"""Times slam_pgo_optimize(10) on the device against the restatement (tests/cpp/pgo_oracle.cpp, banded solve, one CPU thread)
for loop graphs of N = 60, 240 and 1000 vertices: median / min / max of 7 runs after a warm-up.  Nothing is asserted; the
figures go into docs/PGO.md.    python tools/pgo_time.py [N ...]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import pgo_cases as K  # noqa: E402
import pgo_oracle as O  # noqa: E402
from slam_amd import api  # noqa: E402

RUNS = 7


def timed(make, run):
    out = []
    for k in range(RUNS + 1):          # the first is the warm-up
        g = make()
        t0 = time.perf_counter()
        res = run(g)
        out.append(time.perf_counter() - t0)
    return np.array(out[1:]) * 1e3, res, g


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [60, 240, 1000]
    api.set_device(0)
    print("device: %s" % api.device_info()[0])
    for n in sizes:
        laps = 2 if n < 100 else 3
        case = K.loop_graph(n, laps, 1)
        dev, rd, gd = timed(lambda: case.fill(api.PoseGraph()), lambda g: g.optimize(10))
        cpu, rc, gc = timed(lambda: case.fill(O.OracleGraph(banded=True)), lambda g: g.optimize(10))
        dm, dr = K.pose_errors(gd.read_vertices(), gc.read_vertices())
        print("N %4d  E %5d  w %2d  trials %2d  chi2 %.6g -> %.6g | device ms median %.2f min %.2f max %.2f | restatement ms median %.2f "
              "min %.2f max %.2f | apart %.3g m %.3g rad" % (n, len(case.edges), rd.half_bandwidth, rd.n_trials, rd.chi2_initial, rd.chi2_final,
                                                              np.median(dev), dev.min(), dev.max(), np.median(cpu), cpu.min(), cpu.max(),
                                                              dm.max(), dr.max()))
        gd.close()


if __name__ == "__main__":
    main()
