"""slam_amd.api.GlobalMapBuilder with `carve` on (docs/VOXEL_MAP.md section 8) against its restatement
(tests/vmap_carve_oracle.py: OracleCarveBuilder on the carve and the Generalized ICP restatements) on the mover scene of
tests/vmap_carve_cases.py, step by step; `carve` off against the restatement that has never heard of carving; and
slam_amd::GlobalMapBuilder (tests/cpp/map_builder_carve_test.cpp) against the Python twin bit for bit."""
import os
import signal
import subprocess

import numpy as np
import pytest

import vmap_carve_cases as K
import vmap_carve_oracle as VC
import vmap_cases as KV
import vmap_oracle as V
from slam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS_TOL, ANG_TOL = 1e-4, 1e-5   # BASELINE.json, as tests/test_gpu_map_builder.py
MARGIN_TOL = 1e-9
RUN_SECONDS = 120
TEST_SECONDS = 300


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


def device_filter(leaf, gate):
    """the store's own voxel filter, through a store of its own: [n, >= 3] f32 -> [m, 3] f32"""
    store = api.KeyframeStore(leaf_size=leaf, gate=gate)

    def f(xyz):
        kid = store.add_keyframe(np.ascontiguousarray(xyz, np.float32))
        out = store.read_keyframe(kid)[:, :3].copy()
        store.remove_keyframe(kid)
        return out
    return f


def device_map(vm):
    xyz4, count, key = vm.read()
    return xyz4, count, key, vm.read_sums()[0]


@pytest.mark.gpu
def test_the_scene_step_by_step():
    scene = K.mover_scene()
    dev = api.GlobalMapBuilder(carve=True)
    ora = VC.OracleCarveBuilder(filter=device_filter(dev.LEAF_SIZE, dev.gate), carve=True)
    assert dev.carve and (dev.CARVE_NUM, dev.CARVE_DEN) == (1, 1)
    for k, (c, pose, truth) in enumerate(scene):
        ok, r = dev.add_cloud(c)
        # the restatement makes its own request on its own carved map, then takes the device's f32 transform over: its
        # voxel map and its carve are then the restatement's of the device's transforms
        oko, ro = ora.add_cloud(c, adopt=(ok, dev.pose()))
        assert ok and oko, k
        assert dev.last_carve == ora.last_carve, (k, dev.last_carve, ora.last_carve)
        if k == 0:
            assert r is None and ro is None
            continue
        dp, da = V.pose_error(r["transform64"], ro["transform64"])
        et = V.pose_error(r["transform"], truth)
        print("step %d: iterations %d/%d state %d/%d fitness %.6g/%.6g; device - restatement %.3g m %.3g rad; from the truth %.2f mm "
              "%.3f mrad; margin %.3g; carve %s" % (k, r["iterations"], ro["iterations"], r["state"], ro["state"], r["fitness"], ro["fitness"],
                                                   dp, da, et[0] * 1e3, et[1] * 1e3, ro["margin"], dev.last_carve))
        if not ro["margin"] < MARGIN_TOL:           # nobody is excused unless the restatement's own stop was a coin toss
            assert (ok, r["iterations"], r["state"]) == (oko, ro["iterations"], ro["state"]), k
        assert dp <= POS_TOL and da <= ANG_TOL, k
        # step by step: the map, seen and miss are the restatement's of the device's own transforms
        assert KV.same_map(device_map(dev.vmap), ora.vmap.extract()), k
        assert all(np.array_equal(a, b) for a, b in zip(dev.vmap.read_carve(), ora.vmap.read_carve())), k
    carved, whole = dev.map(), dev.vmap.read()[0]
    assert np.array_equal(carved.view(np.uint32), ora.map().view(np.uint32))
    g_whole, g_carved = int(K.ghost_mask(whole, scene[0][1]).sum()), int(K.ghost_mask(carved, scene[0][1]).sum())
    print("device builder on the mover scene: %d voxels, %d ghosts uncarved; %d voxels, %d ghosts carved" % (len(whole), g_whole, len(carved), g_carved))
    assert len(carved) < len(whole) and g_carved < g_whole
    assert (dev.n_clouds, dev.n_accepted) == (K.N_SCANS, K.N_SCANS)
    dev.close()


@pytest.mark.gpu
def test_carve_off_is_a_builder_that_has_never_heard_of_carving():
    scene = K.mover_scene()[:4]
    dev = api.GlobalMapBuilder(carve=False)
    ora = V.OracleBuilder(filter=device_filter(dev.LEAF_SIZE, dev.gate))       # the restatement from before carving existed
    assert not dev.carve
    for k, (c, pose, truth) in enumerate(scene):
        ok, r = dev.add_cloud(c)
        oko, ro = ora.add_cloud(c, adopt=(ok, dev.pose()))
        assert ok and oko and dev.last_carve is None
        if k and not ro["margin"] < MARGIN_TOL:
            assert (r["iterations"], r["state"]) == (ro["iterations"], ro["state"]), k
    assert KV.same_map(device_map(dev.vmap), ora.vmap.extract())
    assert np.array_equal(dev.map().view(np.uint32), ora.vmap.extract()[0].view(np.uint32))
    seen, miss, key = dev.vmap.read_carve()
    assert not seen.any() and not miss.any()
    dev.close()


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "map_builder_carve_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_builder_carve_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_builder_carve_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


@pytest.mark.gpu
def test_cpp_and_python_build_the_same_carved_map(tmp_path):
    d = str(tmp_path)
    exe = compile_test(d)
    clouds = [c for c, _, _ in K.mover_scene()]
    for i, c in enumerate(clouds):
        np.ascontiguousarray(c, np.float32).tofile(os.path.join(d, "cloud_%d.f32" % i))
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(len(clouds))], timeout=RUN_SECONDS, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(lines) == len(clouds) + 1 and lines[-1][0] == "map"

    b = api.GlobalMapBuilder(carve=True)
    for i, c in enumerate(clouds):
        ok, res = b.add_cloud(c)
        row = lines[i]
        assert ok and row[0] == "cloud" and int(row[1]) == 1 and int(row[2]) == int(res is not None), i
        if res is not None:
            assert [int(v) for v in row[3:6]] == [res["iterations"], res["state"], res["fitness_pairs"]], i
            assert float.fromhex(row[6]) == res["fitness"], i
        pose = np.array([float.fromhex(w) for w in row[7:23]], np.float32)
        assert np.array_equal(pose.view(np.uint32), b.pose().reshape(16).view(np.uint32)), i
        assert [int(v) for v in row[23:29]] == [b.last_carve[f] for f in VC.COUNTERS], i
    seen, miss, key = b.vmap.read_carve()
    carved = b.map()
    assert np.fromfile(os.path.join(d, "map.key"), np.uint64).tobytes() == key.tobytes()
    assert np.fromfile(os.path.join(d, "map.seen"), np.uint32).tobytes() == seen.tobytes()
    assert np.fromfile(os.path.join(d, "map.miss"), np.uint32).tobytes() == miss.tobytes()
    assert np.fromfile(os.path.join(d, "map.carved"), np.uint32).tobytes() == carved.view(np.uint32).tobytes()
    i = b.vmap.info()
    assert [int(v) for v in lines[-1][1:]] == [i["n_voxels"], i["n_points"], len(carved)] and miss.any() and len(carved) < i["n_voxels"]
    b.close()
