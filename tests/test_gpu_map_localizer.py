"""slam_amd.api.MapLocalizer on the device (docs/VOXEL_MAP.md section 11.3) on cases A and B of tests/map_localizer_cases.py,
with the device's own filter as in tests/test_gpu_vmap_gicp.py: per (start, level) the restatement registers from the device's
f32 init; the derived levels against maps integrated directly; the winner; determinism; load against set_map; and
slam_amd::MapLocalizer (tests/cpp/map_localizer_test.cpp) against the Python twin, bit for bit."""
import math
import os
import signal
import subprocess

import numpy as np
import pytest

import map_localizer_cases as ML
import vmap_gicp_oracle as VG
import vmap_oracle as V
from slam_amd import api, build
from test_gpu_vmap_gicp import check_equal, device_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_SECONDS = 120       # the C++ program
TEST_SECONDS = 300
POS_TOL, ANG_TOL = 1e-4, 1e-5   # BASELINE.json, as tests/test_gpu_vmap_gicp.py
MARGIN_TOL = 1e-9
CASES = {"A": ML.CASE_A, "B": ML.CASE_B}
SCALARS = ("iterations", "state", "converged", "pairs", "mse", "cost", "fitness", "fitness_pairs")


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


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def result_bits(r):
    return None if r is None else {k: bits(v) if isinstance(v, np.ndarray) else v for k, v in r.items()}


def answer_bits(out):
    return {k: ([[result_bits(r) for r in lv] for lv in v] if k == "last" else bits(v) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


@pytest.fixture(scope="module")
def world():
    """the scene, the fine device map (leaf 1, distributions, clouds 0 .. 4 at the truth), and per case the device's answer
    with the restatement's registration of every (start, level) from the device's own f32 init -- computed once"""
    parts, cloud, truth = ML.scene()
    fine = api.VoxelMap(leaf=ML.LEAF)
    fine.enable_distributions()
    for c, T in parts:
        assert fine.integrate(c, T[:3, :3], T[:3, 3]) == 0
    runs = {}
    for name, case in CASES.items():
        loc = api.MapLocalizer(levels=case["levels"])
        loc.set_map(fine)
        starts = ML.starts_of(case, truth)
        out = loc.localize(cloud, starts)
        ora = ML.OracleLocalizer(parts, case["levels"], filter=device_filter(ML.STORE_LEAF, 2.0))
        assert ora.set_scan(cloud) == out["n_source"]
        want = [[None] * len(starts) for _ in range(case["levels"])]
        for i in range(len(starts)):
            init = np.array(starts[i], np.float32)
            for k in range(case["levels"] - 1, -1, -1):
                r = out["last"][k][i]
                if r is None:
                    break
                want[k][i] = ora.register(k, init)
                init = r["transform"]
        runs[name] = dict(loc=loc, starts=starts, out=out, ora=ora, want=want)
    yield dict(parts=parts, cloud=cloud, truth=truth, fine=fine, runs=runs)
    for r in runs.values():
        r["loc"].close()
    fine.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_start_and_level_against_the_restatement(world, name):
    run = world["runs"][name]
    out, want, levels = run["out"], run["want"], CASES[name]["levels"]
    for i in range(len(run["starts"])):
        live = True
        for k in range(levels - 1, -1, -1):
            r, ro = out["last"][k][i], want[k][i]
            assert (r is not None) == live, (i, k)                              # one call per level carries exactly the live starts
            if not live:
                continue
            dp, da = V.pose_error(r["transform64"], ro["transform64"])
            n = ro["iterations"] + 1
            print("%s start %d level %d: iterations %d/%d state %d/%d pairs %d/%d fitness %.6g/%.6g (%d/%d pairs); device - restatement "
                  "%.3g m %.3g rad; margin %.3g" % (name, i, k, r["iterations"], ro["iterations"], r["state"], ro["state"], r["pairs"], ro["pairs"],
                                                   r["fitness"], ro["fitness"], r["fitness_pairs"], ro["fitness_pairs"], dp, da, ro["margin"]))
            if not ro["margin"] < MARGIN_TOL:           # nobody is excused unless the restatement's own stop was a coin toss
                assert (r["iterations"], r["state"], r["converged"]) == (ro["iterations"], ro["state"], ro["converged"]), (i, k)
                assert r["pairs"] == ro["pairs"], (i, k)
            assert dp <= POS_TOL and da <= ANG_TOL, (i, k)
            assert (r["state"] in ML.OUT) == (ro["state"] in ML.OUT), (i, k)    # the live / out decisions
            live = r["state"] not in ML.OUT


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_pairs_of_every_iteration(world, name):
    """the traced form of the same requests: the pairs of every iteration against the restatement's"""
    run = world["runs"][name]
    loc, out, want = run["loc"], run["out"], run["want"]
    scan = loc.store.add_keyframe(world["cloud"])
    try:
        for i in range(len(run["starts"])):
            init = np.array(run["starts"][i], np.float32)
            for k in range(CASES[name]["levels"] - 1, -1, -1):
                r, ro = out["last"][k][i], want[k][i]
                if r is None:
                    break
                m = loc.level(k)
                t = m.register_gicp(loc.store, scan, init, trace=ML.MAX_ITERATIONS + 1, gate=ML.GATE_RATIO * m.params.leaf,
                                    max_iterations=ML.MAX_ITERATIONS, transformation_epsilon=ML.TRANSFORMATION_EPSILON)
                for f in ("transform", "transform64", "hessian"):
                    assert VG.same_bits(t[f], r[f]), (i, k, f)                  # the batch's answer is the single traced call's
                assert all(t[f] == r[f] for f in SCALARS), (i, k)
                if not ro["margin"] < MARGIN_TOL:
                    n = ro["iterations"] + 1
                    assert np.array_equal(t["pairs_trace"][:n], ro["pairs_trace"][:n]), (i, k)
                init = r["transform"]
    finally:
        loc.store.remove_keyframe(scan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_winner(world, name):
    run, truth = world["runs"][name], world["truth"]
    out, want = run["out"], run["want"]
    w = ML.pick(want[0], out["n_source"], api.MapLocalizer.MAX_SCORE)
    assert out["found"] and w >= 0
    e = V.pose_error(out["transform"], truth)
    print("%s: winner %d (restatement %d), %.3f mm %.4f mrad from the truth" % (name, out["index"], w, e[0] * 1e3, e[1] * 1e3))
    assert e[0] * 1e3 <= 2 * ML.RECORDED_MM and e[1] * 1e3 <= 2 * ML.RECORDED_MRAD
    dp, da = V.pose_error(out["transform64"], want[0][w]["transform64"])
    assert dp <= POS_TOL and da <= ANG_TOL
    if all((r is None) == (ro is None) and (r is None or VG.same_bits(r["transform"], ro["transform"])) for r, ro in zip(out["last"][0], want[0])):
        assert out["index"] == w
    assert out["index"] == ML.pick(out["last"][0], out["n_source"], api.MapLocalizer.MAX_SCORE)
    T = out["transform"]
    assert VG.same_bits(T, out["last"][0][out["index"]]["transform"])
    assert (out["x"], out["y"], out["theta"]) == (float(T[0, 3]), float(T[1, 3]), math.atan2(float(T[1, 0]), float(T[0, 0])))
    if name == "A":
        lost = [r for r in out["last"][0] if r is not None and r["fitness"] > api.MapLocalizer.MAX_SCORE]
        assert len(lost) >= 1


@pytest.mark.gpu
def test_the_derived_levels_are_maps_integrated_directly(world):
    run = world["runs"]["A"]
    for k in range(CASES["A"]["levels"]):
        check_equal(run["loc"].level(k), run["ora"].levels[k])
    assert run["loc"].level(0) is world["fine"] and [run["loc"].level(k).params.leaf for k in range(4)] == [1.0, 2.0, 4.0, 8.0]


@pytest.mark.gpu
def test_no_keyframe_stays_and_the_same_call_gives_the_same_bits(world):
    run = world["runs"]["A"]
    loc = run["loc"]
    again = loc.localize(world["cloud"], run["starts"])
    assert answer_bits(again) == answer_bits(run["out"])
    assert len(loc.store) >= 2
    for kid in range(len(loc.store)):
        with pytest.raises(api.SlamError) as e:
            loc.store.info(kid)
        assert e.value.code == api.E_INVALID
    # the fan of the call's own making: yaw_fan(x, y, yaw, N_YAW) is the default
    x, y, yaw = ML.start_pose(CASES["A"], world["truth"])
    own = loc.localize(world["cloud"], x=x, y=y, yaw=yaw)
    assert loc.N_YAW == CASES["A"]["fan"] and answer_bits(own) == answer_bits(run["out"])


@pytest.mark.gpu
def test_load_gives_what_set_map_gives_and_rebuild_follows_the_map(world, tmp_path):
    run = world["runs"]["B"]
    p = str(tmp_path / "fine.vmap")
    world["fine"].save(p)
    loc = api.MapLocalizer(levels=CASES["B"]["levels"])
    loc.load(p)
    assert loc.owned and loc.level(0) is not world["fine"]
    assert answer_bits(loc.localize(world["cloud"], run["starts"])) == answer_bits(run["out"])
    # the fine map grows: rebuild() makes the derived levels those of the grown map
    extra = V.builder_clouds([5])[0][0]
    T = world["truth"]
    loc.level(0).integrate(extra, T[:3, :3], T[:3, 3])
    loc.rebuild()
    ora = ML.OracleLocalizer(world["parts"] + [(extra, T)], CASES["B"]["levels"])
    for k in range(CASES["B"]["levels"]):
        check_equal(loc.level(k), ora.levels[k])
    loc.close()


@pytest.mark.gpu
def test_maps_the_localiser_cannot_take(world):
    plain = api.VoxelMap(leaf=1.0)
    big = api.VoxelMap(leaf=2.0)
    big.enable_distributions()
    odd = api.VoxelMap(leaf=0.7)             # moments at a leaf that is no multiple of 2^-16 m: coarsen refuses
    odd.enable_distributions()
    odd.integrate(world["parts"][0][0])
    loc = api.MapLocalizer(levels=4)
    for m in (plain, big, odd):
        with pytest.raises(api.SlamError) as e:
            loc.set_map(m)
        assert e.value.code == api.E_INVALID
    with pytest.raises(api.SlamError):
        loc.localize(world["cloud"], world["runs"]["B"]["starts"])              # no map was taken
    with pytest.raises(api.SlamError):
        loc.rebuild()
    three = api.MapLocalizer(levels=3)
    three.set_map(big)                       # 2 m times 4 is 8 m: the last legal leaf
    assert three.level(2).params.leaf == 8.0
    for x in (three, loc):
        x.close()
    for m in (plain, big, odd):
        m.close()


# ------------------------------------------------------------------ the C++ twin
def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "map_localizer_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_localizer_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_localizer_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def hexes(words):
    return [float.fromhex(w) for w in words]


@pytest.mark.gpu
def test_cpp_twin_returns_the_python_twins_bits(world, tmp_path):
    d = str(tmp_path)
    exe = compile_test(d)
    run, case = world["runs"]["A"], CASES["A"]
    world["fine"].save(os.path.join(d, "map.vmap"))
    np.ascontiguousarray(world["cloud"][:, :3], np.float32).tofile(os.path.join(d, "scan.f32"))
    x, y, yaw = ML.start_pose(case, world["truth"])
    assert all(bits(a) == bits(b) for a, b in zip(api.MapLocalizer.yaw_fan(x, y, yaw, case["fan"]), run["starts"]))
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(case["levels"]), float(x).hex(), float(y).hex(), float(yaw).hex(), str(case["fan"])], timeout=RUN_SECONDS,
                       capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    starts = [ln for ln in lines if ln[0] == "start"]
    assert len(starts) == case["fan"]
    for ln, s in zip(starts, run["starts"]):
        assert bits(np.array(hexes(ln[2:]), np.float32)) == bits(s)
    out = run["out"]
    results = {(int(ln[1]), int(ln[2])): ln for ln in lines if ln[0] == "result"}
    assert set(results) == {(k, i) for k in range(case["levels"]) for i in range(case["fan"]) if out["last"][k][i] is not None}
    for (k, i), ln in results.items():
        p = out["last"][k][i]
        assert [int(v) for v in ln[3:8]] == [p["iterations"], p["state"], p["converged"], p["pairs"], p["fitness_pairs"]], (k, i)
        assert float.fromhex(ln[8]) == p["fitness"], (k, i)
        assert bits(np.array(hexes(ln[9:25]), np.float32)) == bits(p["transform"]) and bits(np.array(hexes(ln[25:41]))) == bits(p["transform64"]), (k, i)
    v = [ln for ln in lines if ln[0] == "verdict"][0]
    assert [int(w) for w in v[1:4]] == [int(out["found"]), out["index"], out["n_source"]]
    assert hexes(v[4:7]) == [out["x"], out["y"], out["theta"]]
    assert bits(np.array(hexes(v[7:23]), np.float32)) == bits(out["transform"]) and bits(np.array(hexes(v[23:39]))) == bits(out["transform64"])
    assert lines[-1][:3] == ["keyframes", "1", "issued,"]
