"""GlobalMapBuilder with `direct` on (docs/VOXEL_MAP.md section 9): slam_amd.api.GlobalMapBuilder(direct=True) against its
restatement (tests/vmap_gicp_oracle.py: OracleDirectBuilder) on the six-cloud sequence step by step, the rejections, carve and
direct together, and slam_amd::GlobalMapBuilder (tests/cpp/map_builder_direct_test.cpp) against the Python twin on nine
clouds bit for bit."""
import os
import signal
import subprocess

import numpy as np
import pytest

import vmap_cases as K
import vmap_gicp_oracle as VG
import vmap_oracle as V
from slam_amd import api, build, synth
from test_gpu_vmap_gicp import ANG_TOL, MARGIN_TOL, POS_TOL, RECORDED_MM, RECORDED_MRAD, check_equal, device_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_SECONDS = 120       # the C++ program
TEST_SECONDS = 300
# between the largest accepted fitness of the sequence (0.0283, step 1) and cloud 25's from the last pose (0.0727), both the
# restatement's: their geometric mean
TIGHT_SCORE = 0.0454


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


def small_cloud(k):
    return synth.make_cloud3d(k, n_loop=50, rings=16, n_az=512)


def live_keyframes(store):
    n = 0
    for kid in range(len(store)):
        try:
            n += store.info(kid)["n_points"] > 0
        except api.SlamError:
            pass
    return n


def device_map(vm):
    xyz4, count, key = vm.read()
    return xyz4, count, key, vm.read_sums()[0]


def build_six():
    clouds = V.builder_clouds()
    dev = api.GlobalMapBuilder(direct=True)
    ora = VG.OracleDirectBuilder(filter=device_filter(dev.LEAF_SIZE, dev.gate))
    rows = []
    for k, (c, pose) in enumerate(clouds):
        ok, r = dev.add_cloud(c)
        oko, ro = ora.add_cloud(c, adopt=(ok, dev.pose()))
        rows.append((ok, r, oko, ro, ora.n_source, V.truth_in_first_frame(clouds[0][1], pose)))
        assert live_keyframes(dev.store) == 0 and dev.map_id == -1     # the scan is gone, a map keyframe never was
    return dev, ora, clouds, rows


@pytest.mark.gpu
def test_six_clouds_step_by_step_and_rejections():
    dev, ora, clouds, rows = build_six()
    assert dev.direct and dev.DIST_LEAF == 1.0 and dev.dmap.params.leaf == 1.0 and dev.vmap.params.leaf == 0.30
    assert rows[0][:4] == (True, None, True, None)
    for k, (ok, r, oko, ro, n_source, truth) in enumerate(rows[1:], 1):
        dp, da = V.pose_error(r["transform64"], ro["transform64"])
        et = V.pose_error(r["transform"], truth)
        print("step %d: accepted %d/%d iterations %d/%d state %d/%d pairs %d/%d of %d fitness %.6g/%.6g; device - restatement %.3g m %.3g rad; "
              "from the truth %.2f mm %.3f mrad; margin %.3g" % (k, ok, oko, r["iterations"], ro["iterations"], r["state"], ro["state"], r["pairs"],
                                                                 ro["pairs"], n_source, r["fitness"], ro["fitness"], dp, da, et[0] * 1e3, et[1] * 1e3,
                                                                 ro["margin"]))
        assert oko and ro["pairs_trace"][0] >= n_source // 2          # the inputs' conditions
        if not ro["margin"] < MARGIN_TOL:
            assert (ok, r["iterations"], r["state"], r["pairs"]) == (oko, ro["iterations"], ro["state"], ro["pairs"]), k
        assert ok and r["state"] == api.KF_TRANSFORM
        assert dp <= POS_TOL and da <= ANG_TOL, k
        assert et[0] * 1e3 <= 2 * RECORDED_MM[k - 1] and et[1] * 1e3 <= 2 * RECORDED_MRAD[k - 1], k
    # both maps are, bit for bit, the restatement's maps of the same clouds under the device's f32 transforms
    assert K.same_map(device_map(dev.vmap), ora.vmap.extract())
    check_equal(dev.dmap, ora.dmap)
    assert np.array_equal(dev.map().view(np.uint32), ora.vmap.extract()[0].view(np.uint32))        # map() stays the 0.30 m map
    assert dev.vmap.info()["n_points"] == dev.dmap.info()["n_points"] == 6 * 8192
    assert (dev.n_clouds, dev.n_accepted, len(dev.store)) == (6, 6, 5)

    # rejections leave both maps and the pose untouched
    bad = small_cloud(25)[0]
    worst_good = max(r["fitness"] for _, r, _, _, _, _ in rows[1:])
    before, before_d, pose = device_map(dev.vmap), dev.dmap.read_moments(), dev.pose()
    _, ro = ora.register(bad)
    print("cloud 25 from the last pose: restatement fitness %.4f after %d iterations; largest accepted fitness %.4f" %
          (ro["fitness"], ro["iterations"], worst_good))
    assert ro["fitness"] > 2 * worst_good
    dev.MAX_SCORE = ora.MAX_SCORE = float(np.sqrt(ro["fitness"] * worst_good))
    ok, r = dev.add_cloud(bad)
    assert not ok and r["fitness_pairs"] > 0 and r["fitness"] > dev.MAX_SCORE
    ok2, r2 = dev.add_cloud(clouds[3][0] + np.float32([1000, 0, 0]))
    assert not ok2 and r2["fitness_pairs"] == 0 and r2["state"] == api.KF_NO_CORRESPONDENCES
    assert K.same_map(device_map(dev.vmap), before) and np.array_equal(dev.pose(), pose)
    assert all(VG.same_bits(a, b) for a, b in zip(dev.dmap.read_moments(), before_d))
    c6, p6 = small_cloud(6)
    ok, r = dev.add_cloud(c6)
    oko, ro = ora.add_cloud(c6, adopt=(ok, dev.pose()))
    et = V.pose_error(r["transform"], V.truth_in_first_frame(clouds[0][1], p6))
    print("cloud 6 after the rejections: fitness %.4f, %.2f mm %.3f mrad from the truth" % (r["fitness"], et[0] * 1e3, et[1] * 1e3))
    assert ok and oko and (r["iterations"], r["state"]) == (ro["iterations"], ro["state"])
    check_equal(dev.dmap, ora.dmap)
    assert (dev.n_clouds, dev.n_accepted) == (9, 7) and live_keyframes(dev.store) == 0
    dev.close()


@pytest.mark.gpu
def test_direct_off_touches_nothing_new_and_carve_with_direct():
    plain = api.GlobalMapBuilder()
    assert not plain.direct and plain.dmap is None
    clouds = V.builder_clouds(range(3))
    both = api.GlobalMapBuilder(carve=True, direct=True)
    assert (both.dmap.dist_params.max_miss_num, both.dmap.dist_params.max_miss_den) == (both.CARVE_NUM, both.CARVE_DEN)
    ora = VG.OracleDistMap(1.0, max_miss_num=both.CARVE_NUM, max_miss_den=both.CARVE_DEN)
    T = np.eye(4)
    for c, _ in clouds:
        ok, r = both.add_cloud(c)
        assert ok
        T = both.pose().astype(np.float64)
        ora.integrate(c, T[:3, :3], T[:3, 3])
        plain.add_cloud(c)
    seen, miss, key = both.dmap.read_carve()
    assert seen.sum() > 0 and both.last_carve["n_seen"] > 0
    ora.set_carve(seen, miss, key)
    check_equal(both.dmap, ora)
    plain.close()
    both.close()


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "map_builder_direct_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_builder_direct_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_builder_direct_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


@pytest.mark.gpu
def test_cpp_and_python_build_the_same_maps(tmp_path):
    d = str(tmp_path)
    exe = compile_test(d)
    clouds = [c for c, _ in V.builder_clouds()]
    clouds.append(small_cloud(25)[0])
    clouds.append(clouds[3] + np.float32([1000, 0, 0]))
    clouds.append(small_cloud(6)[0])
    for i, c in enumerate(clouds):
        np.ascontiguousarray(c, np.float32).tofile(os.path.join(d, "cloud_%d.f32" % i))
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(len(clouds)), "6", repr(TIGHT_SCORE)], timeout=RUN_SECONDS, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(lines) == len(clouds) + 1 and lines[-1][0] == "map"

    b = api.GlobalMapBuilder(direct=True)
    accepted = []
    for i, c in enumerate(clouds):
        if i >= 6:
            b.MAX_SCORE = TIGHT_SCORE
        ok, res = b.add_cloud(c)
        accepted.append(ok)
        row = lines[i]
        assert row[0] == "cloud" and int(row[1]) == int(ok) and int(row[2]) == int(res is not None), i
        if res is not None:
            assert [int(v) for v in row[3:7]] == [res["iterations"], res["state"], res["pairs"], res["fitness_pairs"]], i
            assert float.fromhex(row[7]) == res["fitness"], i
        pose = np.array([float.fromhex(w) for w in row[8:24]], np.float32)
        assert np.array_equal(pose.view(np.uint32), b.pose().reshape(16).view(np.uint32)), i
    assert accepted == [True] * 6 + [False, False, True]
    assert np.fromfile(os.path.join(d, "map.xyz4"), np.uint32).tobytes() == b.map().view(np.uint32).tobytes()
    E, M, key = b.dmap.read_moments()
    assert np.fromfile(os.path.join(d, "dist.key"), np.uint64).tobytes() == key.tobytes()
    assert np.fromfile(os.path.join(d, "dist.E"), np.int64).tobytes() == E.tobytes()
    assert np.fromfile(os.path.join(d, "dist.M"), np.int64).tobytes() == M.tobytes()
    assert np.fromfile(os.path.join(d, "dist.flag"), np.uint8).tobytes() == b.dmap.read_distributions()["flag"].tobytes()
    i = b.dmap.info()
    assert [int(v) for v in lines[-1][1:]] == [len(b.map()), i["n_voxels"], i["n_points"], len(b.store)]
    assert i["n_points"] == 7 * 8192
    b.close()
