"""The voxel map on the device (slam_vmap_*, slam_amd/csrc/voxmap.hip) against its scalar restatement
(tests/cpp/vmap_oracle.cpp): keys, counts, sums and centroids bit for bit, whatever the table's size, the order of the
clouds and the run; the extraction's box, min_count and capacity; handle lifetime; argument errors.  Inputs:
tests/vmap_cases.py, the smallest that reach every path (one lane, a wavefront and one more, two workgroups, rehashes)."""
import ctypes as C
import signal

import numpy as np
import pytest

import vmap_cases as K
import vmap_oracle as V
from slam_amd import api

pytestmark = pytest.mark.gpu
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


def device_map(m):
    """(xyz4, count, key, sums) of the whole device map, as OracleMap.extract gives them"""
    xyz4, count, key = m.read()
    sums, count2, key2 = m.read_sums()
    assert np.array_equal(count, count2) and np.array_equal(key, key2)
    return xyz4, count, key, sums


def both(clouds, leaf=K.LEAF, **kw):
    """the device map and the restatement of the same (points, R, t) list; the dropped counts must agree on the way"""
    dm, om = api.VoxelMap(leaf=leaf, **kw), V.OracleMap(leaf)
    for pts, R, t in clouds:
        assert dm.integrate(pts, R, t) == om.integrate(pts, R, t)
    return dm, om


def check_equal(dm, om):
    got, want = device_map(dm), om.extract()
    assert K.same_map(got, want)
    i = dm.info()
    assert i["n_voxels"] == om.n_voxels == len(want[2]) and i["n_points"] == om.n_points
    assert i["n_voxels"] <= i["capacity"] // 2
    return got


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("moved", (False, True))
def test_sizes_with_and_without_a_transform(n, moved):
    pts = K.cloud(257, 7, spread=3.0)[:n]
    R, t = K.transform(1) if moved else (None, None)
    dm, om = both([(pts, R, t)])
    got = check_equal(dm, om)
    assert len(got[2]) <= n and (n == 0) == (len(got[2]) == 0)
    dm.close()


def test_two_thousand_points_in_one_voxel():
    dm, om = both([(K.one_voxel(2000), None, None)])
    got = check_equal(dm, om)
    assert list(got[1]) == [2000]
    dm.close()


# (points, dropped, voxels) of the four edge clouds, and what carving the dropped cloud from (0.1, 0.1, 0.1) counts
EDGE_CLOUDS = ((K.boundary_points()[0], 0, 3), (K.negative_points()[0], 0, 3), (K.rounding_points()[0], 0, 1), (K.dropped_points()[0], 7, 2))
DROPPED_CARVE = dict(n_rays=2, n_dropped=7, n_skipped=1)


def test_boundaries_rounding_and_dropped_points():
    for pts in (K.boundary_points()[0], K.negative_points()[0], K.rounding_points()[0]):
        dm, om = both([(pts, None, None)])
        check_equal(dm, om)
        dm.close()
    pts, want_dropped = K.dropped_points()
    dm, om = api.VoxelMap(leaf=K.LEAF), V.OracleMap(K.LEAF)
    assert dm.integrate(pts) == om.integrate(pts) == want_dropped
    check_equal(dm, om)
    # a transform that throws every point out of range
    assert dm.integrate(pts[:1], np.eye(3), (0, 5e6, 0)) == om.integrate(pts[:1], np.eye(3), (0, 5e6, 0)) == 1
    check_equal(dm, om)
    dm.close()
    # the same four clouds through the other users of the cell rule: the integrate with moments, and carve
    from test_gpu_vmap_carve import Pair
    from test_gpu_vmap_gicp import check_equal as check_dist_equal, dist_map
    for pts, dropped, voxels in EDGE_CLOUDS:
        dm, om = dist_map(K.LEAF)
        assert dm.integrate(pts) == om.integrate(pts) == dropped
        assert len(check_dist_equal(dm, om)["key"]) == voxels
        dm.close()
        p = Pair(leaf=K.LEAF)
        p.integrate(pts)
        r = p.carve(pts, origin=(0.1, 0.1, 0.1))
        assert r["n_dropped"] == dropped and r["n_rays"] == len(pts) - dropped
        if dropped:
            assert {k: r[k] for k in DROPPED_CARVE} == DROPPED_CARVE
        seen, miss, key = p.check()
        assert len(key) == voxels
        p.close()


def four(order, **kw):
    return both([(K.FOUR_CLOUDS[i][0],) + K.FOUR_CLOUDS[i][1] for i in order], **kw)


@pytest.fixture(scope="module")
def base():
    """the four clouds in their first order, in a map created large: the bits everything else must reproduce"""
    dm, om = four(K.ORDERS[0], initial_capacity=1 << 16)
    got = check_equal(dm, om)
    assert dm.info()["capacity"] == 1 << 16
    return dm, om, got


def test_growth_through_rehashes_gives_the_same_bits(base):
    dm, om = four(K.ORDERS[0], initial_capacity=64)
    assert dm.info()["capacity"] >= 2 * len(base[2][2]) > 64
    assert K.same_map(check_equal(dm, om), base[2])
    dm.close()
    # one cloud at a time in pieces of 100 points: a rehash whenever the load rule asks for one
    dm = api.VoxelMap(leaf=K.LEAF, initial_capacity=64)
    caps = set()
    for pts, (R, t) in K.FOUR_CLOUDS:
        for o in range(0, len(pts), 100):
            dm.integrate(pts[o:o + 100], R, t)
            caps.add(dm.info()["capacity"])
    assert len(caps) >= 4
    assert K.same_map(device_map(dm), base[2])
    dm.close()


def test_three_orders_of_four_clouds_give_the_same_bits(base):
    for order in K.ORDERS[1:]:
        dm, om = four(order)
        assert K.same_map(check_equal(dm, om), base[2])
        dm.close()


def test_the_same_call_twice_gives_the_same_bits(base):
    a, _ = four(K.ORDERS[2])
    b, _ = four(K.ORDERS[2])
    assert K.same_map(device_map(a), device_map(b)) and K.same_map(device_map(a), base[2])
    a.close()
    b.close()


def test_extraction(base):
    dm, om, whole = base
    xyz4, count, key, _ = whole
    assert np.all(key[1:] > key[:-1]) and np.all(xyz4[:, 3] == 0)
    # boxes with both ends on a centroid: the ends are centroids of the map itself
    xs, ys = np.sort(xyz4[:, 0]), np.sort(xyz4[:, 1])
    n = len(xs)
    for lo, hi in (((xs[n // 4], ys[n // 4]), (xs[3 * n // 4], ys[3 * n // 4])), ((xs[0], ys[0]), (xs[-1], ys[-1])),
                   ((xs[n // 2], ys[0]), (xs[n // 2], ys[-1])), ((1.0, 1.0), (-1.0, -1.0))):
        want = om.extract(lo, hi)
        got = dm.read(lo, hi)
        assert K.same_map(got, want[:3])
        inside = (xyz4[:, 0] >= lo[0]) & (xyz4[:, 0] <= hi[0]) & (xyz4[:, 1] >= lo[1]) & (xyz4[:, 1] <= hi[1])
        assert np.array_equal(got[2], key[inside])
    assert len(dm.read((xs[n // 2], ys[0]), (xs[n // 2], ys[-1]))[2]) >= 1     # the voxel the ends lie on is kept
    for mc in (1, 2, 5):
        want = om.extract(min_count=mc)
        assert 0 < len(want[2]) and K.same_map(dm.read(min_count=mc), want[:3])
    assert len(om.extract(min_count=2)[2]) < len(key)
    want = om.extract((xs[n // 4], ys[n // 4]), (xs[3 * n // 4], ys[3 * n // 4]), 2)
    assert K.same_map(dm.read((xs[n // 4], ys[n // 4]), (xs[3 * n // 4], ys[3 * n // 4]), 2), want[:3])


def test_device_form_and_a_capacity_too_small(base):
    dm, om, whole = base
    n = len(whole[2])
    d_xyz4, d_count, d_key = api.DeviceArray((n, 4), np.float32), api.DeviceArray((n,), np.uint32), api.DeviceArray((n,), np.uint64)
    for a in (d_xyz4, d_count, d_key):
        a.zero()
    with pytest.raises(api.SlamError) as e:
        dm.extract_dev(d_xyz4, n - 1, d_count=d_count, d_key=d_key)
    assert e.value.code == api.E_NOMEM and e.value.needed == n
    api.synchronize()
    assert not d_xyz4.download().any() and not d_key.download().any()       # nothing was written
    stream = api.Stream()
    assert dm.extract_dev(d_xyz4, n, d_count=d_count, d_key=d_key, stream=stream) == n
    stream.synchronize()
    assert K.same_map((d_xyz4.download(), d_count.download(), d_key.download()), whole[:3])
    # the centroids alone, and a box, through the device form
    d_xyz4.zero()
    lo, hi = (-1.0, -2.0), (2.0, 1.5)
    want = om.extract(lo, hi)
    got_n = dm.extract_dev(d_xyz4, n, lo=lo, hi=hi)
    api.synchronize()
    assert got_n == len(want[2]) and np.array_equal(d_xyz4.download()[:got_n].view(np.uint32), want[0].view(np.uint32))


def test_device_pointer_integration_with_a_stride_and_a_stream():
    pts = np.zeros((300, 5), np.float32)
    pts[:, :3] = K.cloud(300, 9, spread=3.0)
    pts[:, 3:] = np.nan                       # what lies between the points is not read
    R, t = K.transform(2)
    d = api.DeviceArray.from_host(pts)
    stream = api.Stream()
    dm, om = api.VoxelMap(leaf=0.30), V.OracleMap(0.30)
    assert dm.integrate_dev(d, 300, stride=5, R=R, t=t, stream=stream) == om.integrate(pts[:, :3].copy(), R, t) == 0
    assert dm.integrate(pts, R, t) == om.integrate(pts[:, :3].copy(), R, t)     # the host form with the same stride
    check_equal(dm, om)
    dm.close()


def test_an_empty_map_and_clear():
    dm = api.VoxelMap(leaf=K.LEAF, initial_capacity=64)
    assert all(len(a) == 0 for a in dm.read()) and dm.info()["n_voxels"] == 0
    d = api.DeviceArray((4, 4), np.float32)
    assert dm.extract_dev(d, 0) == 0 and dm.extract_dev(d, 4) == 0
    pts, (R, t) = K.FOUR_CLOUDS[0]
    om = V.OracleMap(K.LEAF)
    dm.integrate(pts, R, t)
    cap = dm.info()["capacity"]
    dm.clear()
    i = dm.info()
    assert (i["n_voxels"], i["n_points"], i["capacity"]) == (0, 0, cap) and len(dm.read()[2]) == 0
    pts, (R, t) = K.FOUR_CLOUDS[1]
    assert dm.integrate(pts, R, t) == om.integrate(pts, R, t)
    check_equal(dm, om)                      # nothing of the first cloud is left
    dm.close()


def test_create_destroy_cycles_keep_device_memory_flat():
    """As tests/test_gpu_lifetime.py measures it: after warm-up cycles, 40 cycles may cost at most what one cycle's
    handle holds while alive, so a buffer leaked per cycle of 1 / 40 of that shows.  The table is created with 2^20 slots
    (36 MB, and 5 MB of extraction scratch): free device memory moves in pieces far larger than a table of a few thousand
    slots, which would read as S = 0."""
    from test_gpu_lifetime import free_bytes, hip_runtime
    rt = hip_runtime()
    pts, (R, t) = K.FOUR_CLOUDS[0]

    def cycle(alive=None):
        dm = api.VoxelMap(leaf=K.LEAF, initial_capacity=1 << 20)
        dm.integrate(pts, R, t)
        out = dm.read()
        if alive is not None:
            alive.append(free_bytes(rt))
        dm.close()
        return out

    first = cycle()
    for _ in range(2):
        cycle()
    free_after_warmup = free_bytes(rt)
    alive = []
    assert K.same_map(cycle(alive), first)
    S = free_after_warmup - alive[0]
    for _ in range(40):
        assert K.same_map(cycle(), first)
    free_after = free_bytes(rt)
    print("vmap lifetime: S = %d bytes, drift over 40 cycles %d bytes" % (S, free_after_warmup - free_after))
    assert S > 0 and free_after >= free_after_warmup - S


def test_argument_errors():
    L = api.lib()
    h = C.c_void_p()
    bad = api.vmap_default_params(leaf=0.0)
    assert L.slam_vmap_create(C.byref(bad), C.byref(h)) == api.E_INVALID
    bad = api.vmap_default_params(leaf=float("nan"))
    assert L.slam_vmap_create(C.byref(bad), C.byref(h)) == api.E_INVALID
    bad = api.vmap_default_params(initial_capacity=(1 << 30) + 1)       # would round up to 2^31 slots
    assert L.slam_vmap_create(C.byref(bad), C.byref(h)) == api.E_INVALID
    assert L.slam_vmap_create(None, None) == api.E_INVALID
    dm = api.VoxelMap(leaf=K.LEAF)
    pts = np.zeros((4, 3), np.float32)
    d = api.DeviceArray.from_host(pts)
    R, t = np.eye(3).reshape(9), np.zeros(3)
    n = C.c_int(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.slam_vmap_integrate_dev(None, d.ptr, 4, 3, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_integrate_dev(dm.h, d.ptr, -1, 3, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_integrate_dev(dm.h, d.ptr, 4, 2, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_integrate_dev(dm.h, None, 4, 3, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_integrate_dev(dm.h, d.ptr, 4, 3, p(R), None, None, None) == api.E_INVALID     # R without t
    assert L.slam_vmap_integrate(dm.h, None, 4, 3, None, None, None) == api.E_INVALID
    assert b"slam_vmap_integrate" in L.slam_last_error()
    lo = np.zeros(2, np.float32)
    assert L.slam_vmap_extract_dev(dm.h, p(lo), None, 0, d.ptr, None, None, 1, C.byref(n), None) == api.E_INVALID   # lo without hi
    assert L.slam_vmap_extract_dev(dm.h, None, None, 0, d.ptr, None, None, -1, C.byref(n), None) == api.E_INVALID
    assert L.slam_vmap_extract_dev(dm.h, None, None, -1, d.ptr, None, None, 1, C.byref(n), None) == api.E_INVALID
    assert L.slam_vmap_extract_dev(dm.h, None, None, 0, d.ptr, None, None, 1, None, None) == api.E_INVALID
    assert L.slam_vmap_read(None, None, None, 0, None, None, None, 0, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_read_sums(None, None, None, None, 0, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_clear(None, None) == api.E_INVALID and L.slam_vmap_info(None, None, None, None, None) == api.E_INVALID
    assert n.value == -5 and dm.info()["n_voxels"] == 0
    L.slam_vmap_destroy(None)
    # an empty cloud is no error and touches nothing
    assert L.slam_vmap_integrate_dev(dm.h, None, 0, 3, None, None, C.byref(n), None) == api.SLAM_OK and n.value == 0
    dm.close()
