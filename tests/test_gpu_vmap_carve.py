"""Free-space carving on the device (slam_vmap_carve*, slam_amd/csrc/voxmap.hip) against its scalar restatement
(tests/cpp/vmap_carve_oracle.cpp): seen, miss, the six counters, the keys and the carved extraction bit for bit, whatever the
table's size, the order of the clouds and the run.  Inputs: tests/vmap_carve_cases.py and tests/vmap_cases.py, the smallest
that reach every path (one lane, a wavefront and one more, two workgroups, the edges of the 64-step chunks, rehashes)."""
import ctypes as C
import signal

import numpy as np
import pytest

import vmap_carve_cases as K
import vmap_carve_oracle as VC
import vmap_cases as KV
import vmap_oracle as V
from slam_amd import api

pytestmark = pytest.mark.gpu
TEST_SECONDS = 300
RATIOS = ((1, 1), (0, 1), (1, 2), (2, 1), (3, 7))
ORIGIN = (0.3, -0.2, 0.1)


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


class Pair:
    """a device map and the restatement, driven together: every call's counters must agree on the way"""

    def __init__(self, leaf=K.LEAF, **kw):
        self.dm, self.om = api.VoxelMap(leaf=leaf, **kw), VC.CarveOracleMap(leaf)

    def integrate(self, pts, R=None, t=None):
        assert self.dm.integrate(pts, R, t) == self.om.integrate(pts, R, t)

    def carve(self, pts, R=None, t=None, origin=None, **kw):
        got = self.dm.carve(pts, R, t, origin, **kw)
        want = self.om.carve(pts, R, t, origin, **kw)
        assert got == want, (got, want)
        return got

    def planes(self):
        return self.dm.read_carve()

    def check(self):
        """seen, miss and keys, the map itself, and the carved extraction at several ratios"""
        got, want = self.dm.read_carve(), self.om.read_carve()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        xyz4, count, key = self.dm.read()
        assert KV.same_map((xyz4, count, key, self.dm.read_sums()[0]), self.om.extract())
        i = self.dm.info()
        assert i["n_voxels"] == self.om.n_voxels == len(key) and i["n_points"] == self.om.n_points
        for mm in RATIOS:
            assert KV.same_map(self.dm.read(max_miss=mm), self.om.extract(max_miss=mm)[:3]), mm
        return got

    def close(self):
        self.dm.close()


BLOCK = K.box_points((-12, -12, -2), (12, 12, 2))      # every cell of a slab around the origin: voxels to cross


@pytest.mark.parametrize("n", KV.SIZES)
@pytest.mark.parametrize("moved", (False, True))
@pytest.mark.parametrize("origin", (None, ORIGIN))
def test_sizes_with_and_without_a_transform_and_an_origin(n, moved, origin):
    pts = KV.cloud(257, 7, spread=3.0)
    R, t = KV.transform(1) if moved else (None, None)
    p = Pair()
    p.integrate(BLOCK)
    p.integrate(pts, R, t)
    r = p.carve(pts[:n], R, t, origin)
    seen, miss, key = p.check()
    assert r["n_rays"] == n and (n > 0 or r["n_steps"] == 0) and (n < 63 or miss.sum() > 0)
    assert r["n_seen"] == int(seen.sum()) <= n and r["n_missed"] == int(miss.sum())
    p.close()


@pytest.mark.parametrize("length", K.CHUNK_EDGE_LENGTHS)
def test_single_rays_at_the_chunk_edges(length):
    o, q = K.skew_ray(length + 1)
    p = Pair()
    p.integrate(K.box_points(o, q, pad=0))
    r = p.carve(q[None], origin=o, end_margin=1, tail_num=0)
    assert (r["n_steps"], r["n_missed"], r["n_seen"], r["n_skipped"]) == (length, length, 1, 0)
    p.check()
    want = VC.closed_form_cells((0, 0, 0), np.floor(q.astype(np.float64) / K.LEAF), VC.params(tail_num=0))
    assert np.array_equal(K.crossed_cells(p.dm), K.sorted_rows(want))
    p.close()


@pytest.mark.parametrize("name", sorted(K.RAYS))
def test_hand_worked_ray(name):
    o, q, prm, want = K.RAYS[name]
    kw = dict(end_margin=prm.end_margin, tail_num=prm.tail_num, tail_den=prm.tail_den, max_ray_cells=prm.max_ray_cells)
    p = Pair()
    p.integrate(K.box_points(o, q))
    r = p.carve(q[None], origin=o, **kw)
    p.check()
    got = K.crossed_cells(p.dm)
    if want is None:
        assert (r["n_skipped"], r["n_steps"], r["n_missed"], r["n_seen"]) == (1, 0, 0, 1) and len(got) == 0
    else:
        assert np.array_equal(got, K.sorted_rows(want)) and (r["n_skipped"], r["n_steps"], r["n_missed"]) == (0, len(want), len(want))
    p.close()


def test_two_thousand_rays_through_one_voxel_and_endpoints_in_one_voxel():
    rng = np.random.default_rng(3)
    ends = (K.centre((10, 0, 0)).astype(np.float64) + (rng.random((2000, 3)) - 0.5) * 0.2499).astype(K.F)      # all in cell (10, 0, 0)
    p = Pair()
    p.integrate(K.centre((2, 0, 0))[None])
    r = p.carve(ends, origin=K.centre((0, 0, 0)))
    seen, miss, key = p.check()
    assert list(miss) == [1] and list(seen) == [0] and (r["n_steps"], r["n_missed"], r["n_seen"]) == (2000 * 8, 1, 0)
    p.close()
    pts = KV.one_voxel(2000)
    p = Pair()
    p.integrate(pts)
    r = p.carve(pts)
    seen, miss, key = p.check()
    assert list(seen) == [1] and list(miss) == [0] and (r["n_seen"], r["n_missed"]) == (1, 0)
    p.close()


def test_a_table_of_64_slots_at_the_load_limit():
    """32 voxels in 64 slots: a lookup of an absent key has to run to an empty slot, for some of them past the last slot"""
    pts = KV.cloud(257, 7, spread=3.0)
    cells = np.concatenate([VC.closed_form_cells((0, 0, 0), np.floor(q.astype(np.float64) / K.LEAF)) for q in pts[:40]])
    cells = np.unique(cells, axis=0)
    rng = np.random.default_rng(5)
    cells = cells[rng.permutation(len(cells))[:32]]
    p = Pair(initial_capacity=64)
    p.integrate(K.centre(cells))
    assert p.dm.info() == dict(p.dm.info(), n_voxels=32, capacity=64)
    r = p.carve(pts)
    seen, miss, key = p.check()
    assert r["n_steps"] > 500 and 0 < r["n_missed"] <= 32 and p.dm.info()["capacity"] == 64
    p.close()


def test_planes_travel_through_rehashes_and_clear_zeroes_them():
    p = Pair(initial_capacity=64)
    p.integrate(BLOCK[:20])
    clouds = KV.FOUR_CLOUDS
    p.carve(BLOCK[:60], origin=ORIGIN)
    caps = {p.dm.info()["capacity"]}
    p.integrate(BLOCK[:2000])
    caps.add(p.dm.info()["capacity"])
    p.carve(clouds[0][0], *clouds[0][1])
    p.check()
    p.integrate(BLOCK)
    caps.add(p.dm.info()["capacity"])
    for pts, (R, t) in clouds:
        p.integrate(pts, R, t)
        p.carve(pts, R, t, ORIGIN)
        caps.add(p.dm.info()["capacity"])
    assert len(caps) >= 3                       # at least two rehashes with the planes alive
    seen, miss, key = p.check()
    assert miss.max() >= 2
    # the same cloud again: every voxel it charged is charged once more (the serial went on, the stamps did not stick)
    before = p.planes()
    r = p.carve(clouds[3][0], *clouds[3][1], ORIGIN)
    after = p.check()
    assert int((after[0] - before[0]).sum()) == r["n_seen"] > 0 and int((after[1] - before[1]).sum()) == r["n_missed"] > 0
    # clear
    cap = p.dm.info()["capacity"]
    p.dm.clear(), p.om.clear()
    assert p.dm.info()["capacity"] == cap and len(p.dm.read_carve()[2]) == 0
    p.integrate(BLOCK)
    seen, miss, key = p.check()
    assert not seen.any() and not miss.any()
    p.carve(clouds[1][0], *clouds[1][1])
    assert p.check()[1].max() == 1
    p.close()


def test_a_map_never_carved_answers_as_before():
    pts, (R, t) = KV.FOUR_CLOUDS[0]
    dm, om = api.VoxelMap(leaf=K.LEAF), V.OracleMap(K.LEAF)          # the restatement that has never heard of carving
    assert dm.integrate(pts, R, t) == om.integrate(pts, R, t)
    bytes_before = dm.info()["device_bytes"]
    xyz4, count, key = dm.read()
    want = om.extract()
    assert KV.same_map((xyz4, count, key, dm.read_sums()[0]), want)
    seen, miss, key2 = dm.read_carve()
    assert np.array_equal(key2, want[2]) and not seen.any() and not miss.any() and seen.dtype == miss.dtype == np.uint32
    for mm in RATIOS:
        assert KV.same_map(dm.read(max_miss=mm), want[:3])          # miss = 0 passes every ratio
    assert dm.info()["device_bytes"] >= bytes_before                 # read_carve's staging at most
    held = dm.info()["device_bytes"]
    dm.carve(pts, R, t)
    assert dm.info()["device_bytes"] >= held + 3 * 4 * dm.info()["capacity"]     # the three planes arrive with the first carve
    assert KV.same_map((dm.read() + (dm.read_sums()[0],)), want)    # and the map is what it was
    dm.close()


def carve_four(order, **kw):
    p = Pair(**kw)
    p.integrate(BLOCK)
    for pts, (R, t) in KV.FOUR_CLOUDS:
        p.integrate(pts, R, t)
    for i in order:
        pts, (R, t) = KV.FOUR_CLOUDS[i]
        p.carve(pts, R, t, ORIGIN)
    return p


@pytest.fixture(scope="module")
def base():
    p = carve_four(KV.ORDERS[0], initial_capacity=1 << 16)
    got = p.check()
    assert got[1].max() >= 2 and got[0].max() >= 1
    return got


def test_three_orders_of_four_clouds_and_the_same_call_twice(base):
    for order in KV.ORDERS[1:] + (KV.ORDERS[2],):
        p = carve_four(order)
        assert all(np.array_equal(a, b) for a, b in zip(p.check(), base))
        p.close()


def test_strides_host_and_device_forms_and_a_stream(base):
    stream = api.Stream()
    for stride in (3, 4, 5):
        p = Pair()
        p.integrate(BLOCK)
        for pts, (R, t) in KV.FOUR_CLOUDS:
            p.integrate(pts, R, t)
        for k, (pts, (R, t)) in enumerate(KV.FOUR_CLOUDS):
            wide = np.full((len(pts), stride), np.nan, np.float32)       # what lies between the points is not read
            wide[:, :3] = pts
            want = p.om.carve(pts, R, t, ORIGIN)
            if k % 2:
                got = p.dm.carve(wide, R, t, ORIGIN)
            else:
                d = api.DeviceArray.from_host(wide)
                got = p.dm.carve_dev(d, len(pts), stride, R, t, ORIGIN, stream=stream if k else None)
                d.free()
            assert got == want
        assert all(np.array_equal(a, b) for a, b in zip(p.check(), base))
        # the carved extraction through the device form
        n = p.dm.info()["n_voxels"]
        d_xyz4, d_count, d_key = api.DeviceArray((n, 4), np.float32), api.DeviceArray((n,), np.uint32), api.DeviceArray((n,), np.uint64)
        want = p.om.extract((-1.0, -2.0), (2.0, 1.5), 1, (1, 1))
        got_n = p.dm.extract_dev(d_xyz4, n, lo=(-1.0, -2.0), hi=(2.0, 1.5), min_count=1, d_count=d_count, d_key=d_key, stream=stream, max_miss=(1, 1))
        stream.synchronize()
        assert 0 < got_n == len(want[2]) < n
        assert KV.same_map((d_xyz4.download()[:got_n], d_count.download()[:got_n], d_key.download()[:got_n]), want[:3])
        with pytest.raises(api.SlamError) as e:
            p.dm.extract_dev(d_xyz4, got_n - 1, lo=(-1.0, -2.0), hi=(2.0, 1.5), min_count=1, max_miss=(1, 1))
        assert e.value.code == api.E_NOMEM and e.value.needed == got_n
        p.close()


def test_argument_errors():
    L = api.lib()
    p = Pair()
    p.integrate(BLOCK)
    p.carve(BLOCK[:100], origin=ORIGIN)
    before = p.planes()
    pts = np.ascontiguousarray(BLOCK[:4])
    d = api.DeviceArray.from_host(pts)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    R, t, n = np.eye(3).reshape(9), np.zeros(3), C.c_int(-5)
    h = p.dm.h
    assert L.slam_vmap_carve_dev(None, d.ptr, 4, 3, None, None, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_carve_dev(h, d.ptr, 4, 2, None, None, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_carve_dev(h, d.ptr, -1, 3, None, None, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_carve_dev(h, None, 4, 3, None, None, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_carve_dev(h, d.ptr, 4, 3, ptr(R), None, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_carve_dev(h, d.ptr, 4, 3, None, ptr(t), None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_carve(h, None, 4, 3, None, None, None, None, None) == api.E_INVALID
    for bad in (dict(tail_den=0), dict(tail_den=-3), dict(end_margin=-1), dict(tail_num=-1), dict(max_ray_cells=0)):
        cp = api.vmap_default_carve_params(**bad)
        assert L.slam_vmap_carve_dev(h, d.ptr, 4, 3, None, None, None, C.byref(cp), None, None) == api.E_INVALID, bad
        assert L.slam_vmap_carve(h, ptr(pts), 4, 3, None, None, None, C.byref(cp), None) == api.E_INVALID, bad
    for o in ((np.nan, 0, 0), (0, 2.0 ** 22, 0), (0, 0, -(2.0 ** 20) * K.LEAF)):        # an origin without a cell
        o = np.array(o, np.float64)
        assert L.slam_vmap_carve_dev(h, d.ptr, 4, 3, None, None, ptr(o), None, None, None) == api.E_INVALID
        with pytest.raises(ValueError):
            p.om.carve(pts, origin=o)
    assert L.slam_vmap_carve_dev(h, d.ptr, 4, 3, ptr(R), ptr(np.array([0, 5e6, 0.0])), None, None, None, None) == api.E_INVALID   # moved out of range
    assert b"origin" in L.slam_last_error()
    assert L.slam_vmap_extract_carved_dev(h, None, None, 0, 1, 0, d.ptr, None, None, 1, C.byref(n), None) == api.E_INVALID
    assert L.slam_vmap_extract_carved_dev(h, None, None, 0, -1, 1, d.ptr, None, None, 1, C.byref(n), None) == api.E_INVALID
    assert L.slam_vmap_extract_carved_dev(h, None, None, 0, 1, 1, d.ptr, None, None, -1, C.byref(n), None) == api.E_INVALID
    assert L.slam_vmap_read_carved(h, None, None, 0, 1, -1, None, None, None, 0, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_read_carved(None, None, None, 0, 1, 1, None, None, None, 0, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_read_carve(h, None, None, None, -1, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_read_carve(h, None, None, None, 0, None) == api.E_INVALID
    assert L.slam_vmap_read_carve(None, None, None, None, 0, C.byref(n)) == api.E_INVALID
    assert n.value == -5
    # a capacity too small: the number needed, nothing else
    assert L.slam_vmap_read_carve(h, None, None, None, 1, C.byref(n)) == api.E_NOMEM and n.value == p.dm.info()["n_voxels"]
    # an empty cloud is no error and charges nothing
    res = api.VmapCarveResult()
    assert L.slam_vmap_carve_dev(h, None, 0, 3, None, None, None, None, C.byref(res), None) == api.SLAM_OK
    assert api.vmap_carve_result_dict(res) == dict.fromkeys(VC.COUNTERS, 0)
    assert all(np.array_equal(a, b) for a, b in zip(p.planes(), before))
    p.check()
    p.close()


def test_create_carve_destroy_cycles_keep_device_memory_flat():
    """As tests/test_gpu_vmap.py sizes it: a table of 2^20 slots (36 MB, and 12 MB of planes), so that free device memory,
    which moves in pieces of megabytes, shows one cycle's holding S; 40 cycles may cost at most S."""
    from test_gpu_lifetime import free_bytes, hip_runtime
    rt = hip_runtime()
    pts, (R, t) = KV.FOUR_CLOUDS[0]

    def cycle(alive=None):
        dm = api.VoxelMap(leaf=K.LEAF, initial_capacity=1 << 20)
        dm.integrate(BLOCK)
        dm.integrate(pts, R, t)
        r = dm.carve(pts, R, t, ORIGIN)
        out = dm.read(max_miss=(1, 1)) + dm.read_carve()[:2] + (np.array(sorted(r.items()), dtype=object),)
        if alive is not None:
            alive.append(free_bytes(rt))
        dm.close()
        return out

    def same(a, b):
        return KV.same_map(a[:5], b[:5]) and list(a[5][:, 1]) == list(b[5][:, 1])

    first = cycle()
    for _ in range(2):
        cycle()
    free_after_warmup = free_bytes(rt)
    alive = []
    assert same(cycle(alive), first)
    S = free_after_warmup - alive[0]
    for _ in range(40):
        assert same(cycle(), first)
    free_after = free_bytes(rt)
    print("vmap carve lifetime: S = %d bytes, drift over 40 cycles %d bytes" % (S, free_after_warmup - free_after))
    assert S > 0 and free_after >= free_after_warmup - S
