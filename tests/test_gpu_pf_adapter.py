"""slam_amd::ParticleFilter (include/slam_amd/correlative.hpp): tests/cpp/pf_test.cpp fills an MLS grid with the synthetic room,
updates a GridMatcher, starts a filter and runs predict + update over three scans, hands particles in, runs the resampling rule
alone and walks the failure paths; every number must be the Python path's (slam_amd.api.ParticleFilter) bit for bit -- both go through
the same C-ABI entry points -- on a fixed grid and on one whose window has rolled."""
import os
import subprocess

import numpy as np
import pytest

import csm_oracle as CO
import pf_cases as F
from slam_amd import api, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, STEPS, N, SEED = 96, 3, 1024, 20260
SIZE, RES, SIGMA = 128, 0.5, 0.5
RUN_SECONDS = 120


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "pf_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pf_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pf_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter headers are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def digest(a):
    """FNV-1a over the array's bytes, as pf_test.cpp prints it"""
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def python_step(pf, ok=True):
    x, y, k = pf.particles()
    acc, w = pf.weights()
    s = pf.state()
    return ([int(ok), s.t, s.n, s.resampled, s.degenerate, s.best, s.refused, s.n_resamples, s.A_max, s.W, s.S2, s.MX, s.MY, s.MC, s.MS],
            [float(v).hex() for v in (s.x, s.y, s.theta)], [digest(x), digest(y), digest(k), digest(acc), digest(w)])


def row_step(words):
    return [int(v) for v in words[:15]], [float.fromhex(v).hex() for v in words[15:18]], words[18:23]        # (hex: NaN before an update compares)


@pytest.mark.gpu
@pytest.mark.parametrize("centre", ((0.0, 0.0), (7 * RES + 0.2, -5 * RES - 0.1)))
def test_the_cpp_twin_equals_the_python_path(tmp_path, centre):
    d = str(tmp_path)
    exe = compile_test(d)
    g = api.Grid(SIZE, SIZE, RES)
    g.set_min_cluster_points(0)
    g.set_pose(*centre)
    c = np.asarray(g.get_pose(), np.float64)
    m_ga, m_nga = CO.synth_map()
    obs = (np.concatenate([m_ga, m_nga]) - c).astype(np.float32)
    g.add_scan_inorder(obs, np.zeros((0, 2), np.float32))
    gm = api.GridMatcher(g, SIGMA)
    gm.update()
    pf = gm.particle_filter(N, seed=SEED)
    A = pf.params.n_angles
    scans = [synth.make_scan(FIRST + i, 256) for i in range(STEPS + 1)]
    x0, y0, th0 = scans[0][2]
    start = np.array([x0, y0, F.heading_index(th0, A), 0.3, 0.3, 10.0])
    motions = np.array([[0.12 + 0.01 * i, -0.01, 0.05, 0.04, 3.0, 16 + i] for i in range(STEPS)])
    weights = np.random.RandomState(3).randint(0, 65537, 777).astype(np.uint32)
    for name, a, dt in (("obstacles.f32", obs, np.float32), ("start.f64", start, np.float64), ("motions.f64", motions, np.float64),
                        ("weights.u32", weights, np.uint32)):
        np.ascontiguousarray(a, dt).tofile(os.path.join(d, name))
    for i in range(STEPS):
        np.ascontiguousarray(scans[i + 1][0]).tofile(os.path.join(d, "t_ga_%d.f64" % i))
        np.ascontiguousarray(scans[i + 1][1]).tofile(os.path.join(d, "t_nga_%d.f64" % i))

    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(SIZE), repr(RES), repr(SIGMA), repr(centre[0]), repr(centre[1]), str(N), str(SEED), str(STEPS)],
                       timeout=RUN_SECONDS, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    rows = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}

    assert int(rows["setup"][0]) == gm.max_cells and int(rows["setup"][3]) == N
    assert (float.fromhex(rows["setup"][1]), float.fromhex(rows["setup"][2])) == gm.centre == tuple(c)
    cs, G, wtab = pf.tables()
    assert rows["tables"] == ["1", digest(cs), digest(G), digest(wtab)]
    pf.init_gaussian(*start)
    assert row_step(rows["init"]) == python_step(pf)
    for i in range(STEPS):
        pf.predict(tuple(motions[i]))
        s = pf.update(scans[i + 1][0], scans[i + 1][1])
        assert row_step(rows["step%d" % i]) == python_step(pf), i
        assert s.W > 0 and abs(s.x - scans[i + 1][2][0]) <= 2 * RES and abs(s.y - scans[i + 1][2][1]) <= 2 * RES    # map frame, rolled or not
    assert pf.state().n_resamples >= 1
    x, y, k = pf.particles()
    pf.set_particles(x + 0.5, y, (k + 7) % A)
    assert row_step(rows["set"]) == python_step(pf)
    src = pf.resample_indices(weights, 12345)
    assert rows["resample"] == ["1", str(len(weights)), digest(src)] and np.array_equal(src, F.resample_search(weights, 12345))
    assert rows["edges"] == ["1"] * 9
    for word in ("the grid matcher is not usable", "n_particles", "n_angles", "a negative sigma", "3 particles given", "heading",
                 "wtab[0] must be 65536"):
        assert word in r.stderr, word                                                # every failure is logged
    pf.close(), gm.close()
