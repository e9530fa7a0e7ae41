"""The occupancy grid's distance field and costmap on the device (slam_gdist_*, slam_grid_distance_field, docs/GRID_DIST.md):
dist2 and cost EQUAL the restatement of tests/grid_dist_cases.py, bit for bit, on every case of its list; the cost rule at its
edge; handle reuse; the grid's own occupancy after a roll and in the in-order mode; the C++ adapter."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import grid_dist_cases as G
from slam_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def inflation(R):
    t = api.inflation_table(max_cells=R, **G.inflation_for(R))
    t.setflags(write=False)
    return t


def field_for(c, **kw):
    return api.DistanceField(c["sx"], c["sy"], max_cells=c["R"], unknown_is_obstacle=c["unk"], **kw)


@pytest.mark.parametrize("name", [c["name"] for c in G.cases()])
def test_dist2_and_cost_equal_the_restatement(name):
    c = G.case(name)
    df = field_for(c)
    df.compute(c["occ"])
    d, cost = df.read()
    assert cost is None and d.dtype == np.uint16 and np.array_equal(d, G.expected(name))
    df.set_table(inflation(c["R"]))
    df.compute(c["occ"])
    d, cost = df.read()
    assert np.array_equal(d, G.expected(name))
    assert cost.dtype == np.uint8 and np.array_equal(cost, G.cost_of(G.expected(name), c["occ"], inflation(c["R"]), c["R"], c["unk"]))
    if name in ("empty", "empty_unknown"):
        assert (d == G.FAR).all()
    if name.startswith("full"):
        assert (d == 0).all() and (cost == 254).all()
    df.close()


@pytest.mark.parametrize("name", G.RANDOM_CASES)
def test_cost_tables_and_the_unknown_rule(name):
    c = G.case(name)
    R, occ, want = c["R"], c["occ"], G.expected(name)
    # an arbitrary table: a random permutation of bytes
    T = G.random_table(R)
    df = field_for(c)
    df.set_table(T)
    df.compute(occ)
    assert np.array_equal(df.read()[1], G.cost_of(want, occ, T, R, c["unk"]))
    df.close()
    # the unknown rule at its edge: an unknown cell inside the inscribed radius (253) keeps its cost from 253, not from 254
    got = {}
    for keep in (253, 254):
        df = field_for(c, unknown_keep_from=keep, unknown_cost=77)
        df.set_table(inflation(R))
        df.compute(occ)
        got[keep] = df.read()[1]
        assert np.array_equal(got[keep], G.cost_of(want, occ, inflation(R), R, c["unk"], unknown_cost=77, unknown_keep_from=keep))
        df.close()
    unknown_inscribed = (occ == G.UNKNOWN) & (inflation(R)[np.minimum(want, R * R + 1)] == 253)
    if not c["unk"] and R >= 7 and "_d0_" not in name:
        assert unknown_inscribed.any()                               # the edge is reached
    if not c["unk"]:
        assert (got[253][unknown_inscribed] == 253).all() and (got[254][unknown_inscribed] == 77).all()


def test_table_removed_and_set_again():
    c = G.case("random_97x83_d1_R7_unk0")
    df = field_for(c)
    L = api.lib()
    short = np.zeros(7 * 7 + 1, np.uint8)
    for t in (short, np.zeros(7 * 7 + 3, np.uint8)):                 # a wrong length on a live handle
        assert L.slam_gdist_set_table(df.h, t.ctypes.data_as(C.c_void_p), len(t)) == api.E_INVALID
        assert b"slam_gdist_set_table" in L.slam_last_error()
    assert L.slam_gdist_set_table(df.h, None, 51) == api.E_INVALID
    with pytest.raises(api.SlamError) as e:                          # nothing computed yet
        df.read()
    assert e.value.code == api.E_INVALID
    df.set_table(inflation(7))
    df.compute(c["occ"])
    first = df.read()[1]
    assert np.array_equal(first, G.cost_of(G.expected(c["name"]), c["occ"], inflation(7), 7))
    df.set_table(None, 0)
    with pytest.raises(api.SlamError) as e:
        df.read(cost=True)
    assert e.value.code == api.E_INVALID and "table" in str(e.value)
    d, cost = df.read()
    assert cost is None and np.array_equal(d, G.expected(c["name"]))
    assert df.planes_dev()[0] and not df.planes_dev()[1]
    T = G.random_table(7, seed=9)
    df.set_table(T)
    with pytest.raises(api.SlamError):                               # the cost plane belongs to the table it was computed with
        df.read(cost=True)
    df.compute(c["occ"])
    assert np.array_equal(df.read()[1], G.cost_of(G.expected(c["name"]), c["occ"], T, 7))
    assert all(df.planes_dev())
    df.close()


def test_one_handle_two_planes():
    """the second plane is emptier than the first: stale row distances, flags or costs would show"""
    dense, sparse, empty = (G.case("random_97x83_d2_R7_unk0"), G.case("random_97x83_d0_R7_unk0"), G.plane(97, 83))
    df = field_for(dense)
    df.set_table(inflation(7))
    for occ, want in ((dense["occ"], G.expected(dense["name"])), (sparse["occ"], G.expected(sparse["name"])),
                      (empty, np.full(97 * 83, G.FAR, np.uint16)), (dense["occ"], G.expected(dense["name"]))):
        df.compute(occ)
        d, cost = df.read()
        assert np.array_equal(d, want) and np.array_equal(cost, G.cost_of(want, occ, inflation(7), 7))
    df.close()


def test_compute_dev_on_a_stream():
    c = G.case("70x700_R32_tile_edges")
    df = field_for(c)
    df.set_table(inflation(32))
    d_occ = api.DeviceArray.from_host(c["occ"], np.int8)
    st = api.Stream()
    df.compute_dev(d_occ, st)
    st.synchronize()
    d, cost = df.read()
    assert np.array_equal(d, G.expected(c["name"])) and np.array_equal(cost, G.cost_of(d, c["occ"], inflation(32), 32))
    p_d, p_c = df.planes_dev()
    raw = np.empty(c["sx"] * c["sy"], np.uint16)
    api.check(api.lib().slam_memcpy_d2h(raw.ctypes.data_as(C.c_void_p), p_d, raw.nbytes, None))
    assert np.array_equal(raw, d)
    df.close()
    d_occ.free()


# ------------------------------------------------------------------------------------------------ the grid's own occupancy
def scan_points(seed, n_obs=60, n_gnd=400):
    rs = np.random.RandomState(seed)
    obs = np.zeros((n_obs, 4), np.float32)
    gnd = np.zeros((n_gnd, 4), np.float32)
    obs[:, :2] = rs.uniform(-1, 1, (n_obs, 2)) * [4.5, 3.7]
    gnd[:, :2] = rs.uniform(-1, 1, (n_gnd, 2)) * [4.5, 3.7]
    return obs, gnd


def check_grid_field(grid, df, R):
    grid.distance_field(df)                                          # first: it may not lean on read_occupancy's own sync
    d, cost = df.read()
    occ = grid.read_occupancy()
    assert (occ == 100).sum() > 10 and (occ == 0).sum() > 10 and (occ == -1).sum() > 10
    want = G.brute(occ, grid.size_x, grid.size_y, R)
    assert np.array_equal(d, want) and np.array_equal(cost, G.cost_of(want, occ, inflation(R), R))
    df.compute(occ)
    d2, cost2 = df.read()
    assert np.array_equal(d2, d) and np.array_equal(cost2, cost)
    return occ


def test_grid_distance_field_after_a_roll():
    grid = api.Grid(96, 80, 0.1, rolling=1, min_cluster_points=0)
    df = api.DistanceField(96, 80, max_cells=32)
    df.set_table(inflation(32))
    grid.add_endpoints(*scan_points(1))
    grid.set_pose(0.7, -0.5)
    info = grid.info()
    assert grid.window_cell() == (7, -5) and info["origin_x"] != 0 and info["origin_y"] != 0
    grid.add_endpoints(*scan_points(2))
    grid.finalize()
    check_grid_field(grid, df, 32)
    grid.close()
    df.close()


def test_grid_distance_field_in_the_inorder_mode():
    grid = api.Grid(96, 80, 0.1, rolling=1, min_cluster_points=0)
    df = api.DistanceField(96, 80, max_cells=32)
    df.set_table(inflation(32))
    grid.add_scan_inorder(*scan_points(3))
    grid.set_pose(-0.3, 0.4)
    grid.add_scan_inorder(*scan_points(4))
    first = check_grid_field(grid, df, 32)                           # no finalize: the in-order mode's own state
    grid.add_scan_inorder(*scan_points(5, n_obs=200))
    again = check_grid_field(grid, df, 32)
    assert not np.array_equal(first, again)
    grid.close()
    df.close()


def test_grid_and_field_of_different_sizes():
    grid = api.Grid(96, 80, 0.1, rolling=1, min_cluster_points=0)
    for sx, sy in ((80, 96), (96, 81), (95, 80)):
        df = api.DistanceField(sx, sy)
        with pytest.raises(api.SlamError) as e:
            grid.distance_field(df)
        assert e.value.code == api.E_INVALID and "slam_grid_distance_field" in str(e.value)
        df.close()
    grid.close()


# ----------------------------------------------------------------------------------------------------------- the C++ adapter
def test_mls_adapter_costmap(tmp_path):
    exe = str(tmp_path / "mls_costmap_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mls_costmap_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    d = str(tmp_path)
    sx, sy, res, R = 96, 80, 0.1, 20
    inscribed, infl, scaling = 0.45, 1.5, 2.5
    scans = [scan_points(6), scan_points(7)]
    for k, (obs, gnd) in enumerate(scans):
        obs.tofile(os.path.join(d, "obs%d.f32" % k))
        gnd.tofile(os.path.join(d, "gnd%d.f32" % k))
    np.array([sx, sy, res, 0.7, -0.5, inscribed, infl, scaling, R], np.float64).tofile(os.path.join(d, "params.f64"))
    subprocess.check_call([exe, d], timeout=120)
    occ = np.fromfile(os.path.join(d, "occ_with.i8"), np.int8)
    dist2 = np.fromfile(os.path.join(d, "dist2.u16"), np.uint16)
    cost = np.fromfile(os.path.join(d, "cost.u8"), np.uint8)
    meta = np.fromfile(os.path.join(d, "meta.f64"), np.float64)
    assert tuple(meta[:5]) == tuple(meta[5:]) and tuple(meta[:3]) == (res, sx, sy)
    # the drivability bytes are what they were: the same clouds through the Python binding, and the map without a costmap
    grid = api.Grid(sx, sy, res, rolling=1, min_cluster_points=0)
    for (obs, gnd), pose in zip(scans, ((0.0, 0.0), (0.7, -0.5))):
        grid.set_pose(*pose)
        grid.add_scan_inorder(obs, gnd)
    assert np.array_equal(occ, grid.read_occupancy())
    assert np.array_equal(occ, np.fromfile(os.path.join(d, "occ_without.i8"), np.int8))
    grid.close()
    assert (occ == 100).sum() > 10 and (occ == -1).sum() > 10
    want = G.brute(occ, sx, sy, R)
    T = api.inflation_table(res, inscribed, infl, scaling, R)
    assert np.array_equal(dist2, want) and np.array_equal(cost, G.cost_of(want, occ, T, R))
