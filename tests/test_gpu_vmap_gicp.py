"""The voxel map's moments, plane distributions and Generalized ICP against them on the device (slam_vmap_enable_distributions
.. slam_vmap_register_gicp; slam_amd/csrc/voxmap.hip, vmap_gicp.hip) against their scalar restatement
(tests/cpp/vmap_gicp_oracle.cpp): moments, sums, counts, keys and distributions bit for bit whatever the table's size and the
order; the registration of the builder's sequence against the growing map step by step; the edges; a batch; the exits the
sequence never takes (a degenerate step, the iteration cap, a trace shorter than the run, a NaN start); handle lifetime.
A map on which distributions were never enabled answers what it answered before."""
import ctypes as C
import signal

import numpy as np
import pytest

import vmap_cases as K
import vmap_gicp_cases as G
import vmap_gicp_oracle as VG
import vmap_oracle as V
from slam_amd import api

pytestmark = pytest.mark.gpu
TEST_SECONDS = 300
POS_TOL, ANG_TOL = 1e-4, 1e-5   # BASELINE.json, as tests/test_gpu_kf_gicp.py
MARGIN_TOL = 1e-9
# the restatement's error against the truth per step of the sequence (docs/VOXEL_MAP.md section 9), mm and mrad; the device
# is bounded at twice that, as section 6 bounds the keyframe path
RECORDED_MM = (1.28, 2.95, 1.68, 1.55, 1.71)
RECORDED_MRAD = (0.064, 0.043, 0.017, 0.031, 0.002)
DIST_FIELDS = ("centroid", "normal", "cov6", "eig", "flag", "key")


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


def dist_map(leaf, **kw):
    dist = {k: kw.pop(k) for k in list(kw) if k in ("min_points", "flat_ratio", "line_ratio", "epsilon", "max_miss_num", "max_miss_den")}
    dm = api.VoxelMap(leaf=leaf, **kw)
    dm.enable_distributions(**dist)
    return dm, VG.OracleDistMap(leaf, **dist)


def check_equal(dm, om):
    """moments, sums, counts, keys and distributions of the device map against the restatement's, bit for bit"""
    want = om.read()
    sums, count, key = dm.read_sums()
    E, M, key2 = dm.read_moments()
    assert VG.same_bits(key, want["key"]) and VG.same_bits(key2, want["key"])
    assert VG.same_bits(count, want["count"]) and VG.same_bits(sums, want["sums"])
    assert VG.same_bits(E, want["E"]) and VG.same_bits(M, want["M"])
    got = dm.read_distributions()
    for f in DIST_FIELDS:
        assert VG.same_bits(got[f], want[f]), f
    assert dm.info()["n_voxels"] == om.n_voxels == len(want["key"])
    return want


@pytest.mark.parametrize("n", G.SIZES)
@pytest.mark.parametrize("moved", (False, True))
def test_sizes_with_and_without_a_transform(n, moved):
    pts = K.cloud(257, 7, spread=3.0)[:n]
    R, t = K.transform(1) if moved else (None, None)
    dm, om = dist_map(0.25)
    assert dm.integrate(pts, R, t) == om.integrate(pts, R, t)
    check_equal(dm, om)
    dm.close()


@pytest.mark.parametrize("leaf", (0.25, 0.30, 1.0))
def test_two_thousand_points_in_one_voxel(leaf):
    pts = ((K.one_voxel(2000).astype(np.float64) - 0.5) * (leaf / 0.25) * 0.999 + 2.0 * leaf + 0.0005 * leaf).astype(np.float32)
    dm, om = dist_map(leaf)
    dm.integrate(pts)
    om.integrate(pts)
    want = check_equal(dm, om)
    assert list(want["count"]) == [2000]
    E, M = G.python_moments(pts, leaf)
    assert [int(x) for x in dm.read_moments()[0][0]] == E and [int(x) for x in dm.read_moments()[1][0]] == M
    dm.close()


def test_hand_worked_voxels_and_a_negative_d():
    for leaf in G.LEAVES:
        dm, om = dist_map(leaf, min_points=4)
        pts = np.concatenate([G.negative_point(leaf)[0], G.corner_point(leaf)[0], G.square(leaf)[0], G.line(leaf)[0], G.blob(leaf)[0],
                              G.too_few(leaf, 4)[0]])
        dm.integrate(pts)
        om.integrate(pts)
        want = check_equal(dm, om)
        assert want["flag"].sum() == 1
        dm.close()
    leaf, p, key, e = G.negative_d_point()
    dm, om = dist_map(leaf)
    dm.integrate(p)
    om.integrate(p)
    check_equal(dm, om)
    assert tuple(int(x) for x in dm.read_moments()[0][0]) == e
    dm.close()


def four(order, leaf=1.0, **kw):
    dm, om = dist_map(leaf, **kw)
    for i in order:
        pts, (R, t) = K.FOUR_CLOUDS[i]
        assert dm.integrate(pts, R, t) == om.integrate(pts, R, t)
    return dm, om


@pytest.fixture(scope="module")
def base():
    """the four clouds in their first order in a map created large, at leaf 0.25 (many voxels) and 1.0 (many plane voxels)"""
    out = {}
    for leaf in (0.25, 1.0):
        dm, om = four(K.ORDERS[0], leaf, initial_capacity=1 << 16)
        out[leaf] = (dm, om, check_equal(dm, om))
        assert dm.info()["capacity"] == 1 << 16
    assert out[1.0][2]["flag"].sum() >= 10      # a guard of the inputs: plane and other voxels are both there
    return out


def same_read(a, b):
    return all(VG.same_bits(a[f], b[f]) for f in a)


@pytest.mark.parametrize("carve", (False, True))
def test_growth_through_rehashes_gives_the_same_bits(base, carve):
    """initial_capacity 64, one cloud at a time in pieces of 100 points: a rehash whenever the load rule asks for one; with
    `carve`, a carve call between the pieces, so that the carved rehash and the moments' move run together"""
    dm, om = dist_map(0.25, initial_capacity=64)
    caps = set()
    for pts, (R, t) in K.FOUR_CLOUDS:
        for o in range(0, len(pts), 100):
            dm.integrate(pts[o:o + 100], R, t)
            om.integrate(pts[o:o + 100], R, t)
            caps.add(dm.info()["capacity"])
            if carve and o % 300 == 0:
                dm.carve(pts[o:o + 100], R, t)
    assert len(caps) >= 4
    want = check_equal(dm, om)
    assert same_read(want, base[0.25][2])
    if carve:      # the carve planes came through the same rehashes: a carved map's counters are alive and the moments untouched
        seen, miss, key = dm.read_carve()
        assert VG.same_bits(key, want["key"]) and seen.sum() > 0
    dm.close()


def test_orders_and_runs_give_the_same_bits(base):
    for order in K.ORDERS[1:] + (K.ORDERS[2],):
        dm, om = four(order, 1.0)
        assert same_read(check_equal(dm, om), base[1.0][2])
        dm.close()


def test_clear_and_enable_refusals():
    dm, om = dist_map(1.0, initial_capacity=64)
    pts, (R, t) = K.FOUR_CLOUDS[0]
    dm.integrate(pts, R, t)
    with pytest.raises(api.SlamError) as e:
        dm.enable_distributions()
    assert e.value.code == api.E_INVALID
    dm.clear()
    om.clear()
    assert len(dm.read_moments()[2]) == 0 and len(dm.read_distributions()["key"]) == 0
    dm.enable_distributions(min_points=6)          # legal again on the empty map
    pts, (R, t) = K.FOUR_CLOUDS[1]
    dm.integrate(pts, R, t)
    om.integrate(pts, R, t)
    check_equal(dm, om)                            # nothing of the first cloud is left in the moments
    dm.close()
    big = api.VoxelMap(leaf=8.5)
    with pytest.raises(api.SlamError) as e:
        big.enable_distributions()
    assert e.value.code == api.E_INVALID
    big.close()
    plain = api.VoxelMap(leaf=1.0)
    L, n = api.lib(), C.c_int()
    assert L.slam_vmap_read_moments(plain.h, None, None, None, 0, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_compute_distributions(plain.h, None) == api.E_INVALID
    plain.close()


@pytest.mark.parametrize("stride", (3, 4, 5))
def test_host_and_device_forms_with_strides(stride):
    pts = np.full((300, stride), np.nan, np.float32)       # what lies between the points is not read
    pts[:, :3] = K.cloud(300, 9, spread=3.0)
    R, t = K.transform(2)
    d = api.DeviceArray.from_host(pts)
    stream = api.Stream()
    dm, om = dist_map(1.0)
    assert dm.integrate_dev(d, 300, stride=stride, R=R, t=t, stream=stream) == om.integrate(pts[:, :3].copy(), R, t) == 0
    assert dm.integrate(pts, R, t) == om.integrate(pts[:, :3].copy(), R, t)
    dm.compute_distributions(stream=stream)
    stream.synchronize()
    check_equal(dm, om)
    dm.close()


def test_carved_rule_in_the_plane_rule():
    """a carved map with max_miss 1 / 1: the restatement gets the device's own seen and miss (the carve is section 8's, held
    elsewhere), the flags must follow the carved rule bit for bit and differ from the uncarved ones"""
    dm, om = dist_map(1.0, max_miss_num=1, max_miss_den=2)
    free, _ = dist_map(1.0)
    for pts, (R, t) in K.FOUR_CLOUDS:
        for m in (dm, om, free):
            m.integrate(pts, R, t)
    for pts, (R, t) in K.FOUR_CLOUDS:
        dm.carve(pts, R, t, origin=(0.0, 0.0, 2.0))
    seen, miss, key = dm.read_carve()
    om.set_carve(seen, miss, key)
    want = check_equal(dm, om)
    plain = free.read_distributions()["flag"]
    print("plane voxels: %d without the carved rule, %d with it" % (plain.sum(), want["flag"].sum()))
    assert want["flag"].sum() < plain.sum()
    dm.close()
    free.close()


def test_a_map_never_enabled_answers_as_before(base):
    """every existing entry point on a map without distributions against the restatement of section 1, and device_bytes what
    it was: the table and the counters at creation (36 bytes a slot and four u32), and after the same calls exactly the
    planes' 72 + 112 bytes a slot below a map that has them"""
    cap = 1 << 16
    dm, om = api.VoxelMap(leaf=0.25, initial_capacity=cap), V.OracleMap(0.25)
    twin = api.VoxelMap(leaf=0.25, initial_capacity=cap)
    assert dm.info()["device_bytes"] == cap * 36 + 16
    twin.enable_distributions()
    assert twin.info()["device_bytes"] == cap * 36 + 16 + cap * (72 + 112)
    for pts, (R, t) in K.FOUR_CLOUDS:
        assert dm.integrate(pts, R, t) == om.integrate(pts, R, t) == twin.integrate(pts, R, t)
    xyz4, count, key = dm.read()
    sums = dm.read_sums()[0]
    twin.read(), twin.read_sums()
    assert K.same_map((xyz4, count, key, sums), om.extract())
    assert len(dm.read_carve()[2]) == len(key) and not dm.read_carve()[0].any()
    want = base[0.25][2]
    assert VG.same_bits(key, want["key"]) and VG.same_bits(sums, want["sums"]) and VG.same_bits(count, want["count"])
    twin.read_carve()
    assert twin.info()["device_bytes"] - dm.info()["device_bytes"] == cap * (72 + 112)
    dm.close()
    twin.close()


# ------------------------------------------------------------------ the registration
def device_filter(leaf, gate):
    """the store's own voxel filter, through a store of its own: [n, >= 3] f32 -> [m, 3] f32"""
    store = api.KeyframeStore(leaf_size=leaf, gate=gate)

    def f(xyz):
        kid = store.add_keyframe(np.ascontiguousarray(xyz, np.float32))
        out = store.read_keyframe(kid)[:, :3].copy()
        store.remove_keyframe(kid)
        return out
    return f


@pytest.fixture(scope="module")
def sequence():
    """Clouds k = 1 .. 5 of the builder's sequence against the growing 1 m map: the device registers, the restatement makes
    the same request on its own map and then takes the device's f32 transform over, so both face the same map at the next
    cloud (as tests/test_gpu_map_builder.py holds the keyframe path)."""
    clouds = V.builder_clouds()
    dm = api.VoxelMap(leaf=1.0)
    dm.enable_distributions()
    store = api.KeyframeStore(leaf_size=0.30, gate=2.0, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
    store.set_gicp_params(max_iterations=100, transformation_epsilon=1e-6)
    ora = VG.OracleDirectBuilder(filter=device_filter(0.30, 2.0))
    dm.integrate(clouds[0][0])
    ora.add_cloud(clouds[0][0])
    T = np.eye(4, dtype=np.float32)
    rows = []
    for k in range(1, 6):
        c = clouds[k][0]
        kid = store.add_keyframe(c)
        r = dm.register_gicp(store, kid, T, trace=101, gate=2.0, max_iterations=100, transformation_epsilon=1e-6)
        single = dm.register_gicp(store, kid, T, gate=2.0, max_iterations=100, transformation_epsilon=1e-6)
        ok = r["fitness_pairs"] > 0 and bool(r["converged"]) and not r["fitness"] > 1.0
        oko, ro = ora.add_cloud(c, adopt=(ok, r["transform"]))
        rows.append((k, kid, T.copy(), ok, r, single, oko, ro, ora.n_source, V.truth_in_first_frame(clouds[0][1], clouds[k][1])))
        if ok:
            T = np.array(r["transform"], np.float32).reshape(4, 4)
            T64 = T.astype(np.float64)
            dm.integrate(c, T64[:3, :3], T64[:3, 3])
    return dm, store, ora, rows


def test_sequence_step_by_step(sequence):
    dm, store, ora, rows = sequence
    for k, kid, T0, ok, r, single, oko, ro, n_source, truth in rows:
        dp, da = V.pose_error(r["transform64"], ro["transform64"])
        et, eo = V.pose_error(r["transform"], truth), V.pose_error(ro["transform"], truth)
        n = ro["iterations"] + 1
        print("step %d: accepted %d/%d iterations %d/%d state %d/%d pairs %s / %s of %d fitness %.6g/%.6g; device - restatement %.3g m %.3g "
              "rad; from the truth %.2f mm %.3f mrad (restatement %.2f mm %.3f mrad); margin %.3g" %
              (k, ok, oko, r["iterations"], ro["iterations"], r["state"], ro["state"], list(r["pairs_trace"][:n]), list(ro["pairs_trace"][:n]),
               n_source, r["fitness"], ro["fitness"], dp, da, et[0] * 1e3, et[1] * 1e3, eo[0] * 1e3, eo[1] * 1e3, ro["margin"]))
        # conditions on the inputs: they guard the inputs, not the device
        assert oko and ro["pairs_trace"][0] >= n_source // 2
        if not ro["margin"] < MARGIN_TOL:           # nobody is excused unless the restatement's own stop was a coin toss
            assert (ok, r["iterations"], r["state"], r["converged"]) == (oko, ro["iterations"], ro["state"], ro["converged"]), k
            assert np.array_equal(r["pairs_trace"][:n], ro["pairs_trace"][:n]) and r["pairs"] == ro["pairs"], k
        assert dp <= POS_TOL and da <= ANG_TOL, k
        # the fitness runs on the f32 transform: with the same f32 bits the two differ by the order of an f64 sum (n eps, n < 4000);
        # one ulp of a rotation entry moves a point 50 m out by 3e-6 m and a term (n . r)^2 with |r| of 0.1 m by 6e-7 of 1e-2
        if VG.same_bits(r["transform"], ro["transform"]):
            assert r["fitness_pairs"] == ro["fitness_pairs"] and abs(r["fitness"] - ro["fitness"]) <= 1e-11 * ro["fitness"], k
        else:
            assert abs(r["fitness"] - ro["fitness"]) <= 1e-3 * ro["fitness"], k
        assert et[0] * 1e3 <= 2 * RECORDED_MM[k - 1] and et[1] * 1e3 <= 2 * RECORDED_MRAD[k - 1], k
        # the plain form is the traced form
        for f in ("transform", "transform64", "hessian"):
            assert VG.same_bits(r[f], single[f]), f
        assert all(r[f] == single[f] for f in ("iterations", "state", "converged", "pairs", "mse", "cost", "fitness", "fitness_pairs"))
    # the device's 1 m map is, bit for bit, the restatement's map of the same clouds under the device's f32 transforms
    check_equal(dm, ora.dmap)


def test_a_batch_of_four_equals_four_single_calls(sequence):
    dm, store, ora, rows = sequence
    reqs = [(kid, T0) for k, kid, T0, *_ in rows[:4]]
    kw = dict(gate=2.0, max_iterations=100, transformation_epsilon=1e-6)
    batch = dm.register_gicp(store, reqs, trace=16, **kw)
    for (kid, T0), b in zip(reqs, batch):
        s = dm.register_gicp(store, kid, T0, trace=16, **kw)
        for f in ("transform", "transform64", "hessian", "pairs_trace"):
            assert VG.same_bits(b[f], s[f]), f
        assert all(b[f] == s[f] for f in ("iterations", "state", "converged", "pairs", "mse", "cost", "fitness", "fitness_pairs"))
    assert len({b["transform64"].tobytes() for b in batch}) == 4


def test_edges_too_few_pairs_and_no_plane_voxel(sequence):
    dm, store, ora, rows = sequence
    # a source far from everything: no pair at all
    far = store.add_keyframe(V.builder_clouds([1])[0][0] + np.float32([1000, 0, 0]))
    r = dm.register_gicp(store, far, np.eye(4), trace=4)
    assert (r["state"], r["converged"], r["iterations"], r["pairs"], r["fitness_pairs"], r["fitness"]) == (api.KF_NO_CORRESPONDENCES, 0, 0, 0, 0, 0.0)
    assert np.array_equal(r["transform"], np.eye(4, dtype=np.float32)) and list(r["pairs_trace"]) == [0, -1, -1, -1]
    # a map whose voxels are lines: no plane voxel
    lines, _ = dist_map(1.0)
    lines.integrate(np.concatenate([G.line(1.0, cell=(c, 0, 0))[0] for c in range(-3, 4)]))
    assert lines.read_distributions()["flag"].sum() == 0
    kid = rows[0][1]
    r = lines.register_gicp(store, kid, np.eye(4))
    assert (r["state"], r["pairs"], r["fitness_pairs"]) == (api.KF_NO_CORRESPONDENCES, 0, 0)
    # two pairable points among many: fewer than 3 pairs.  The store refuses a keyframe of fewer than k points, so the source
    # is a full cloud moved away except for what lands near the two patches of tests/test_vmap_gicp_oracle.py
    patches, po = dist_map(1.0)
    pp = np.concatenate([G.plane_patch((0, 0, 0), 0, n=4), G.plane_patch((1, 0, 0), 2, n=4)])
    patches.integrate(pp)
    po.integrate(pp)
    src = np.concatenate([np.float32([(0.5, 0.5, 0.5), (1.5, 0.5, 0.5)]), V.builder_clouds([1])[0][0] + np.float32([500, 500, 0])])
    small = api.KeyframeStore(leaf_size=0.30, gate=2.0)
    kid = small.add_keyframe(src)
    xyz, cov = small.read_keyframe(kid)[:, :3].copy(), None
    small.compute_covariances(kid)
    cov = small.covariances(kid)
    r = patches.register_gicp(small, kid, np.eye(4), gate=0.4, trace=4)
    ro = po.register(xyz, cov, np.eye(4), gate=0.4, trace=4)
    assert (r["state"], r["pairs"], r["iterations"]) == (ro["state"], ro["pairs"], ro["iterations"]) == (api.KF_NO_CORRESPONDENCES, 2, 0)
    assert r["fitness_pairs"] == ro["fitness_pairs"] == 2
    with pytest.raises(api.SlamError) as e:           # a dead keyframe id
        small.remove_keyframe(kid)
        patches.register_gicp(small, kid, np.eye(4))
    assert e.value.code == api.E_INVALID
    plain = api.VoxelMap(leaf=1.0)
    with pytest.raises(api.SlamError) as e:           # a map without distributions
        plain.register_gicp(store, rows[0][1], np.eye(4))
    assert e.value.code == api.E_INVALID
    for m in (lines, patches, plain):
        m.close()
    small.close()


# ------------------------------------------------------------------ the exits the sequence never takes
@pytest.fixture(scope="module")
def exits():
    """Eight plane voxels in a row (normal z, centroids at (c + 1/2, 1/2, 1/2)) on the device and in the restatement, and two
    small sources, each in a store whose filter keeps every point: a line along x with y = z = 0 exactly, 32 points each in the
    middle of a 0.25 m filter voxel, and 64 points of a fixed seed in the box x 0 .. 8, y 0 .. 1, z 0.3 .. 0.7.  A source is
    (store, keyframe id, the store's own filtered cloud, its covariances)."""
    dm, om = dist_map(1.0)
    patches = np.concatenate([G.plane_patch((c, 0, 0), 2, n=4) for c in range(8)])
    dm.integrate(patches)
    om.integrate(patches)
    assert check_equal(dm, om)["flag"].sum() == 8
    rng = np.random.default_rng(20261020)
    clouds = {"line": (0.25, np.float32([(0.25 * i + 0.125, 0, 0) for i in range(32)])),
              "box": (0.05, (rng.random((64, 3)) * [8, 1, 0.4] + [0, 0, 0.3]).astype(np.float32))}
    src = {}
    for name, (leaf, xyz) in clouds.items():
        store = api.KeyframeStore(leaf_size=leaf, gate=2.0)
        kid = store.add_keyframe(xyz)
        store.compute_covariances(kid)
        src[name] = (store, kid, store.read_keyframe(kid)[:, :3].copy(), store.covariances(kid))
        assert len(src[name][2]) == len(xyz) >= 20
    yield dm, om, src
    dm.close()
    for store, *_ in src.values():
        store.close()


def test_degenerate_line_returns_the_start(exits):
    """no pair constrains the roll about the line: H(0, 0) is an exact zero and the first pivot fails"""
    dm, om, src = exits
    store, kid, xyz, cov = src["line"]
    assert not xyz[:, 1:].any()
    ro = om.register(xyz, cov, np.eye(4), gate=2.0, trace=4)
    assert (ro["state"], ro["iterations"], ro["converged"]) == (api.KF_DEGENERATE, 0, 0) and ro["pairs"] >= 3      # the input's guard
    r = dm.register_gicp(store, kid, np.eye(4), gate=2.0, trace=4)
    print("degenerate: state %d iterations %d pairs %d trace %s H00 %g" % (r["state"], r["iterations"], r["pairs"], list(r["pairs_trace"]),
                                                                         r["hessian"][0, 0]))
    assert (r["state"], r["iterations"], r["converged"], r["pairs"]) == (api.KF_DEGENERATE, 0, 0, ro["pairs"])
    assert np.array_equal(r["pairs_trace"], ro["pairs_trace"]) and r["pairs_trace"][0] == ro["pairs"]
    assert VG.same_bits(r["transform"], np.eye(4, dtype=np.float32)) and VG.same_bits(r["transform64"], np.eye(4))


@pytest.mark.parametrize("cap", (1, 2))
def test_iteration_cap(exits, cap):
    dm, om, src = exits
    store, kid, xyz, cov = src["box"]
    ro = om.register(xyz, cov, np.eye(4), gate=2.0, max_iterations=cap, trace=4)
    assert (ro["state"], ro["iterations"]) == (api.KF_ITERATIONS, cap) and ro["pairs"] >= 3                        # the input's guard
    r = dm.register_gicp(store, kid, np.eye(4), gate=2.0, max_iterations=cap, trace=4)
    dp, da = V.pose_error(r["transform64"], ro["transform64"])
    print("cap %d: state %d iterations %d pairs %d trace %s; device - restatement %.3g m %.3g rad; margin %.3g" %
          (cap, r["state"], r["iterations"], r["pairs"], list(r["pairs_trace"]), dp, da, ro["margin"]))
    if not ro["margin"] < MARGIN_TOL:
        assert (r["state"], r["iterations"], r["converged"]) == (api.KF_ITERATIONS, cap, 1)
        assert r["pairs"] == ro["pairs"] and np.array_equal(r["pairs_trace"], ro["pairs_trace"])
    assert dp <= POS_TOL and da <= ANG_TOL
    dp, da = V.pose_error(r["transform"], ro["transform"])
    assert dp <= POS_TOL and da <= ANG_TOL


def test_a_trace_shorter_than_the_run(exits):
    """trace_cap 2 of a run of more than two iterations: two entries are written and not a word beyond them, and the result
    is that of the same call with a long trace"""
    dm, om, src = exits
    store, kid, xyz, cov = src["box"]
    ro = om.register(xyz, cov, np.eye(4), gate=2.0, trace=128)
    assert ro["iterations"] > 2                                                                                   # the input's guard
    full = dm.register_gicp(store, kid, np.eye(4), gate=2.0, trace=128)
    assert full["iterations"] > 2 and (full["pairs_trace"][:full["iterations"]] >= 0).all()
    req, res, p = api.VmapGicpReq(), api.VmapGicpResult(), api.vmap_default_gicp_params(gate=2.0)
    req.src = kid
    req.init[:] = np.eye(4, dtype=np.float32).reshape(16).tolist()
    tr = np.full(8, -7, np.int32)
    api.check(api.lib().slam_vmap_register_gicp_traced(dm.h, store.h, C.byref(req), 1, C.byref(p), C.byref(res), tr.ctypes.data_as(C.c_void_p), 2, None))
    r = api.vmap_gicp_result_dict(res)
    print("short trace: %s of %s, iterations %d / %d" % (list(tr), list(full["pairs_trace"][:4]), r["iterations"], full["iterations"]))
    assert np.array_equal(tr[:2], full["pairs_trace"][:2]) and (tr[2:] == -7).all()
    for f in ("transform", "transform64", "hessian"):
        assert VG.same_bits(r[f], full[f]), f
    assert all(r[f] == full[f] for f in ("iterations", "state", "converged", "pairs", "mse", "cost", "fitness", "fitness_pairs"))


def test_nan_start_is_returned_as_it_came(exits):
    dm, om, src = exits
    store, kid, xyz, cov = src["box"]
    init = np.full((4, 4), np.nan, np.float32)
    ro = om.register(xyz, cov, init, gate=2.0, trace=4)
    assert (ro["state"], ro["iterations"], ro["pairs"]) == (api.KF_NO_CORRESPONDENCES, 0, 0)                      # the input's guard
    r = dm.register_gicp(store, kid, init, gate=2.0, trace=4)
    assert (r["state"], r["iterations"], r["converged"], r["pairs"], r["fitness_pairs"]) == (api.KF_NO_CORRESPONDENCES, 0, 0, 0, 0)
    assert list(r["pairs_trace"]) == [0, -1, -1, -1]
    assert VG.same_bits(r["transform"][:3], init[:3]) and VG.same_bits(r["transform64"][:3], init[:3].astype(np.float64))
    assert VG.same_bits(r["transform"][3], np.float32([0, 0, 0, 1])) and VG.same_bits(r["transform64"][3], np.float64([0, 0, 0, 1]))


def test_create_enable_integrate_register_destroy_cycles_keep_device_memory_flat(sequence):
    """As tests/test_gpu_vmap.py sizes it: the table is created with 2^20 slots, so that a cycle's handle moves free device
    memory in pieces it can be read in; 40 cycles may cost at most what one cycle's handle holds while alive."""
    from test_gpu_lifetime import free_bytes, hip_runtime
    rt = hip_runtime()
    dm0, store, ora, rows = sequence
    cloud0 = V.builder_clouds([0])[0][0]
    kid = rows[0][1]

    def cycle(alive=None):
        dm = api.VoxelMap(leaf=1.0, initial_capacity=1 << 20)
        dm.enable_distributions()
        dm.integrate(cloud0)
        r = dm.register_gicp(store, kid, np.eye(4))
        if alive is not None:
            alive.append(free_bytes(rt))
        dm.close()
        return r["transform64"].tobytes(), r["iterations"]

    first = cycle()
    for _ in range(2):
        cycle()
    free_after_warmup = free_bytes(rt)
    alive = []
    assert cycle(alive) == first
    S = free_after_warmup - alive[0]
    for _ in range(40):
        assert cycle() == first
    free_after = free_bytes(rt)
    print("vmap gicp lifetime: S = %d bytes, drift over 40 cycles %d bytes" % (S, free_after_warmup - free_after))
    assert S > 0 and free_after >= free_after_warmup - S
