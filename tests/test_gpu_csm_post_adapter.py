"""slam_amd::CorrelativeMatcher::matchPosterior and slam_amd::Posterior (include/slam_amd/correlative.hpp):
tests/cpp/csm_post_test.cpp runs the room and the corridor of docs/CSM.md section 6 and prints the posterior, the floored
covariance, the information matrix and ambiguous(); all must be the Python path's bit for bit -- the same C-ABI entry
point and the same operations in the two adapters."""
import os
import subprocess

import numpy as np
import pytest

import csm_post_cases as PC
from slam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_SECONDS = 120


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "csm_post_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "csm_post_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_csm_post_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def test_python_helpers_by_hand():
    """Not a GPU test: covariance, information and ambiguous of a posterior written down by hand"""
    p = api.CsmPosterior()
    p.valid, p.second_score, p.score, p.n_points, p.u = 1, 90, 100, 10, (0.1, 0.1, 0.01)
    p.cov[0], p.cov[3], p.cov[5], p.cov[1] = 2.0, 1.0, 0.5, 0.25
    c = p.covariance(floor=False)
    assert c.tolist() == [[2.0, 0.25, 0.0], [0.25, 1.0, 0.0], [0.0, 0.0, 0.5]]
    f = p.covariance()
    assert f[0, 0] == 2.0 + (0.1 * 0.1) / 12.0 and f[2, 2] == 0.5 + (0.01 * 0.01) / 12.0 and f[0, 1] == 0.25
    assert np.allclose(p.information() @ f, np.eye(3), atol=1e-12)
    assert p.ambiguous(1) and not p.ambiguous(0)
    p.second_score = -1
    assert not p.ambiguous(255)
    z = api.CsmPosterior()
    z.u = (0.0, 0.0, 0.0)
    assert z.information() is None                                 # an all-zero covariance has no inverse


def hex_doubles(words):
    return np.array([float.fromhex(w) for w in words])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["room", "corridor"])
def test_match_posterior_equals_the_python_path(tmp_path, scene):
    d = str(tmp_path)
    exe = compile_test(d)
    m_ga, m_nga, ga, nga, R0, t0 = PC.room_scene() if scene == "room" else PC.corridor_scene()
    for name, a in (("m_ga", m_ga), ("m_nga", m_nga), ("t_ga", ga), ("t_nga", nga), ("init", np.concatenate([R0.reshape(4), t0]))):
        np.ascontiguousarray(a, np.float64).tofile(os.path.join(d, name + ".f64"))
    hx, hy, ht, step = PC.SCENE_WINDOW
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(hx), str(hy), str(ht), float(step).hex()], timeout=RUN_SECONDS, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    rows = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}

    cm = api.CorrelativeMatcher(m_ga, m_nga)
    cm.set_window(hx, hy, ht, step)
    cm.set_post_params()
    Rc, tc, res, post = cm.match_post(ga, nga, R0, t0)
    assert hex_doubles(rows["candidate"]).tobytes() == np.concatenate([Rc.reshape(4), tc]).tobytes()
    assert [int(v) for v in rows["result"][:6]] == [res.k, res.a, res.b, res.score, res.max_score, res.n_points]
    assert [int(v) for v in rows["ints"]] == [post.valid, post.n_within, post.margin, post.blocks_evaluated, post.second_score,
                                              post.second_k, post.second_a, post.second_b]
    assert [int(v) for v in rows["sums"]] == [post.m0] + list(post.m1) + list(post.m2)
    assert hex_doubles(rows["mean"]).tobytes() == np.array(list(post.mean)).tobytes()
    assert hex_doubles(rows["cov"]).tobytes() == np.array(list(post.cov)).tobytes()
    assert hex_doubles(rows["covariance"]).tobytes() == post.covariance().tobytes()
    assert hex_doubles(rows["unfloored"]).tobytes() == post.covariance(floor=False).tobytes()
    info = post.information()
    assert info is not None and hex_doubles(rows["information"]).tobytes() == info.tobytes()
    assert np.allclose(info @ post.covariance(), np.eye(3), atol=1e-9)
    ambiguous = scene == "corridor"
    assert post.ambiguous(1) == ambiguous
    assert rows["flags"] == ["1", "1", "1", str(int(ambiguous)), str(int(post.ambiguous(0)))]
    cm.close()
