"""slam_amd::CorrelativeMatcher (include/slam_amd/correlative.hpp): tests/cpp/csm_test.cpp makes the call pair
CorrelativeMatcher::match, IcpPointToPoint::fit on one of the scans ICP alone loses (tests/csm_oracle.py: the basin) and
prints both poses; they must be the Python path's bit for bit -- both go through the same C-ABI entry points."""
import os
import subprocess

import numpy as np
import pytest

import csm_oracle as CO
from slam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN, MAX_ITER = 96, 100
RUN_SECONDS = 120


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "csm_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "csm_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_csm_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def hex_doubles(words):
    return np.array([float.fromhex(w) for w in words])


@pytest.mark.gpu
def test_match_then_fit_equals_the_python_path(tmp_path):
    d = str(tmp_path)
    exe = compile_test(d)
    m_ga, m_nga = CO.synth_map()
    ga, nga, pose, R0, t0 = CO.basin_case(SCAN)
    for name, a in (("m_ga", m_ga), ("m_nga", m_nga), ("t_ga", ga), ("t_nga", nga), ("init", np.concatenate([R0.reshape(4), t0]))):
        np.ascontiguousarray(a, np.float64).tofile(os.path.join(d, name + ".f64"))
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(MAX_ITER)], timeout=RUN_SECONDS, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    rows = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}

    cm, icp = api.CorrelativeMatcher(m_ga, m_nga), api.Icp(m_ga, m_nga)
    icp.set_max_iterations(MAX_ITER)
    Rc, tc, res = cm.match(ga, nga, R0, t0)
    Rf, tf, _ = icp.fit(ga, nga, Rc, tc, 5.0)
    assert hex_doubles(rows["candidate"]).tobytes() == np.concatenate([Rc.reshape(4), tc]).tobytes()
    assert [int(v) for v in rows["result"][:6]] == [res.k, res.a, res.b, res.score, res.max_score, res.n_points]
    assert float.fromhex(rows["result"][6]) == res.score / res.max_score
    assert hex_doubles(rows["fit"]).tobytes() == np.concatenate([Rf.reshape(4), tf]).tobytes()
    assert rows["edges"] == ["1", "1", "1"]
    # ... and the pair does what it is for: ICP alone is lost from this start (tests/test_csm_oracle.py), the pair is not
    e = CO.pose_error(Rf, tf, pose)
    assert e[0] < 0.01 and e[1] < 1e-3, e
    cm.close()
    icp.close()
