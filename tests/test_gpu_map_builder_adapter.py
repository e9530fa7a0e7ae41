"""slam_amd::GlobalMapBuilder (include/slam_amd/map_builder.hpp): tests/cpp/map_builder_test.cpp runs the six clouds of
docs/VOXEL_MAP.md, a cloud that is refused for its score, one a kilometre away and a good one again, and prints every
step; slam_amd.api.GlobalMapBuilder on the same clouds must give the same bits -- both go through the same C-ABI calls."""
import os
import signal
import subprocess

import numpy as np
import pytest

import vmap_oracle as V
from slam_amd import api, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_SECONDS = 120       # the C++ program
TEST_SECONDS = 300      # a whole test: above RUN_SECONDS, so that a child that hangs ends as a failed test and an in-process hang
                        # ends the session
# between the largest accepted fitness (0.050) and cloud 25's (0.219) of tests/test_vmap_oracle.py: their geometric mean
TIGHT_SCORE = 0.1045


@pytest.fixture(autouse=True)
def time_limit():
    """Every test here ends after TEST_SECONDS, and the session with it: nothing more is started on the GPU."""
    def expired(signum, frame):
        pytest.exit("GPU test exceeded %d s" % TEST_SECONDS, returncode=3)
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "map_builder_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_builder_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_builder_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


@pytest.mark.gpu
def test_cpp_and_python_build_the_same_map(tmp_path):
    d = str(tmp_path)
    exe = compile_test(d)
    clouds = [c for c, _ in V.builder_clouds()]
    clouds.append(synth.make_cloud3d(25, n_loop=50, rings=16, n_az=512)[0])
    clouds.append(clouds[3] + np.float32([1000, 0, 0]))
    clouds.append(synth.make_cloud3d(6, n_loop=50, rings=16, n_az=512)[0])
    for i, c in enumerate(clouds):
        np.ascontiguousarray(c, np.float32).tofile(os.path.join(d, "cloud_%d.f32" % i))
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(len(clouds)), "6", repr(TIGHT_SCORE)], timeout=RUN_SECONDS, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(lines) == len(clouds) + 1 and lines[-1][0] == "store"

    b = api.GlobalMapBuilder()
    accepted = []
    for i, c in enumerate(clouds):
        if i >= 6:
            b.MAX_SCORE = TIGHT_SCORE
        ok, res = b.add_cloud(c)
        accepted.append(ok)
        row = lines[i]
        assert row[0] == "cloud" and int(row[1]) == int(ok) and int(row[2]) == int(res is not None), i
        if res is not None:
            assert [int(v) for v in row[3:6]] == [res["iterations"], res["state"], res["fitness_pairs"]], i
            assert float.fromhex(row[6]) == res["fitness"], i
        pose = np.array([float.fromhex(w) for w in row[7:23]], np.float32)
        assert np.array_equal(pose.view(np.uint32), b.pose().reshape(16).view(np.uint32)), i
    assert accepted == [True] * 6 + [False, False, True]
    xyz4, count, key = b.vmap.read()
    assert np.fromfile(os.path.join(d, "map.xyz4"), np.uint32).tobytes() == xyz4.view(np.uint32).tobytes()
    assert np.fromfile(os.path.join(d, "map.count"), np.uint32).tobytes() == count.tobytes()
    assert np.fromfile(os.path.join(d, "map.key"), np.uint64).tobytes() == key.tobytes()
    i = b.vmap.info()
    live = sum(1 for kid in range(len(b.store)) if _alive(b.store, kid))
    assert [int(v) for v in lines[-1][1:]] == [len(b.store), live, b.map_id, i["n_voxels"], i["n_points"]]
    assert live <= 2 and i["n_points"] == 7 * 8192
    b.close()


def _alive(store, kid):
    try:
        return store.info(kid)["n_points"] > 0
    except api.SlamError:
        return False
