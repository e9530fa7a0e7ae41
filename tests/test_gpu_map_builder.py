"""slam_amd.api.GlobalMapBuilder (global_generate.cpp's loop over slam_vmap_* and slam_kf_register_gicp) against its
restatement (tests/vmap_oracle.py: OracleBuilder on the voxel map's and the Generalized ICP's scalar restatements): the
six-cloud sequence of docs/VOXEL_MAP.md step by step, the rejections, and the built map as GlobalMatcher's prior map."""
import signal

import numpy as np
import pytest

import kf_gicp_cases as G
import vmap_cases as K
import vmap_oracle as V
from slam_amd import api, synth

pytestmark = pytest.mark.gpu
POS_TOL, ANG_TOL = 1e-4, 1e-5   # BASELINE.json, as tests/test_gpu_kf_gicp.py
MARGIN_TOL = 1e-9
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


def small_cloud(k):
    return synth.make_cloud3d(k, n_loop=50, rings=16, n_az=512)


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


def live_keyframes(store):
    n = 0
    for kid in range(len(store)):
        try:
            n += store.info(kid)["n_points"] > 0
        except api.SlamError:
            pass
    return n


def build_six():
    """The six clouds through the device builder and, step by step on the same map, through the restatement."""
    clouds = V.builder_clouds()
    dev = api.GlobalMapBuilder()
    ora = V.OracleBuilder(filter=device_filter(dev.LEAF_SIZE, dev.gate))
    rows = []
    for k, (c, pose) in enumerate(clouds):
        ok, r = dev.add_cloud(c)
        # the restatement makes its own request on its own map, then takes the device's f32 transform over: its voxel
        # map is then the restatement's map of the device's transforms, and both face the same map at the next cloud
        oko, ro = ora.add_cloud(c, adopt=(ok, dev.pose()))
        rows.append((ok, r, oko, ro, V.truth_in_first_frame(clouds[0][1], pose)))
        assert live_keyframes(dev.store) <= 2
    return dev, ora, clouds, rows


@pytest.fixture(scope="module")
def built():
    """build_six() once for the tests that only read it: none of them changes the builders"""
    return build_six()


def test_six_clouds_step_by_step(built):
    dev, ora, clouds, rows = built
    assert rows[0][:4] == (True, None, True, None)
    for k, (ok, r, oko, ro, truth) in enumerate(rows[1:], 1):
        dp, da = V.pose_error(r["transform64"], ro["transform64"])
        et = V.pose_error(r["transform"], truth)
        print("step %d: accepted %d/%d iterations %d/%d state %d/%d fitness %.6g/%.6g; device - restatement %.3g m %.3g rad; from the "
              "truth %.2f mm %.3f mrad; margin %.3g" % (k, ok, oko, r["iterations"], ro["iterations"], r["state"], ro["state"], r["fitness"],
                                                        ro["fitness"], dp, da, et[0] * 1e3, et[1] * 1e3, ro["margin"]))
        if not ro["margin"] < MARGIN_TOL:           # nobody is excused unless the restatement's own stop was a coin toss
            assert (ok, r["iterations"], r["state"]) == (oko, ro["iterations"], ro["state"]), k
        assert ok and r["state"] == api.KF_TRANSFORM
        assert dp <= POS_TOL and da <= ANG_TOL, k
    # the device map is, bit for bit, the restatement's voxel map of the same clouds under the device's f32 transforms
    assert K.same_map(device_map(dev.vmap), ora.vmap.extract())
    i = dev.vmap.info()
    assert i["n_points"] == 6 * 8192 and i["n_voxels"] == ora.vmap.n_voxels
    assert np.array_equal(dev.map().view(np.uint32), ora.vmap.extract()[0].view(np.uint32))
    assert (dev.n_clouds, dev.n_accepted) == (6, 6)
    # the store: one id for the map and one per later scan were issued, two at most are alive
    assert len(dev.store) == 6 and live_keyframes(dev.store) <= 2 and dev.store.info(dev.map_id)["n_points"] > 0


def test_rejections_leave_map_and_pose_untouched():
    dev, ora, clouds, rows = build_six()       # builders of its own: it changes MAX_SCORE and the map
    bad = small_cloud(25)[0]
    worst_good = max(r["fitness"] for _, r, _, _, _ in rows[1:])
    before, pose = device_map(dev.vmap), dev.pose()
    # measured at the reference's MAX_SCORE (nothing changes the map when the cloud is then refused below): a copy of the
    # builder's state is not needed, the restatement's request at the same state gives the fitness
    _, ro = ora.register(bad)
    print("cloud 25 from the last pose: restatement fitness %.4f after %d iterations; largest accepted fitness %.4f" %
          (ro["fitness"], ro["iterations"], worst_good))
    assert ro["fitness"] > 2 * worst_good
    dev.MAX_SCORE = ora.MAX_SCORE = float(np.sqrt(ro["fitness"] * worst_good))
    ok, r = dev.add_cloud(bad)
    assert not ok and r["fitness_pairs"] > 0 and r["fitness"] > dev.MAX_SCORE
    assert K.same_map(device_map(dev.vmap), before) and np.array_equal(dev.pose(), pose)
    ok, r = dev.add_cloud(clouds[3][0] + np.float32([1000, 0, 0]))
    assert not ok and r["fitness_pairs"] == 0 and r["state"] == api.KF_NO_CORRESPONDENCES
    assert K.same_map(device_map(dev.vmap), before) and np.array_equal(dev.pose(), pose)
    c6, p6 = small_cloud(6)
    ok, r = dev.add_cloud(c6)
    oko, ro = ora.add_cloud(c6, adopt=(ok, dev.pose()))
    et = V.pose_error(r["transform"], V.truth_in_first_frame(clouds[0][1], p6))
    print("cloud 6 after the rejections: fitness %.4f, %.2f mm %.3f mrad from the truth" % (r["fitness"], et[0] * 1e3, et[1] * 1e3))
    assert ok and oko and (r["iterations"], r["state"]) == (ro["iterations"], ro["state"])
    assert K.same_map(device_map(dev.vmap), ora.vmap.extract()) and dev.vmap.info()["n_points"] == 7 * 8192
    assert (dev.n_clouds, dev.n_accepted) == (9, 7) and live_keyframes(dev.store) <= 2
    dev.close()


def test_the_built_map_is_a_prior_map_for_the_global_matcher(built):
    """drive, build a map, relocalise in it: cloud k = 8 from G.POSE_OFFSET off its true pose, as tests/test_gpu_global_match.py
    starts its scan.  Found on the CPU with the restatement: seed 1 passes first at start 5, 19 mm and 1.3 mrad from the truth
    after the coarse match.  Bounds: a match is found, the refinement ends no farther from the truth than the coarse match
    (the existing test's), and within 0.05 m and 0.01 rad of it: three times what docs/KF_GICP.md section 5 records for
    Generalized ICP on voxel centroids (14.7 mm, 2.9 mrad)."""
    dev, ora, clouds, rows = built
    gm = api.GlobalMatcher(seed=1)
    gm.set_map(dev.map())
    scan, pose = small_cloud(8)
    truth = V.truth_in_first_frame(clouds[0][1], pose)
    true_pose = (truth[0, 3], truth[1, 3], float(np.arctan2(truth[1, 0], truth[0, 0])))
    cur = [np.float32(p + o) for p, o in zip(true_pose, G.POSE_OFFSET)]
    e = gm.match(scan, *cur)
    assert e is not None and e["matched"]
    coarse, refined = V.pose_error(e["coarse"], truth), V.pose_error(e["refined"], truth)
    print("global match in the built map: start %d, coarse %.2f mm %.3f mrad, refined %.2f mm %.3f mrad from the truth" %
          (e["start"], coarse[0] * 1e3, coarse[1] * 1e3, refined[0] * 1e3, refined[1] * 1e3))
    assert refined[0] <= coarse[0]
    assert refined[0] <= 0.05 and refined[1] <= 0.01
    gm.close()
