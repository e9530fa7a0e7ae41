"""The occupancy grid's navigation field and path on the device (slam_gnav_*, slam_grid_nav_field, docs/GRID_NAV.md): the
potential, every path with its length and status, and the state's flags EQUAL the restatement of tests/grid_nav_cases.py, bit for
bit, on every case of its list; too few rounds and a continued call; handle reuse, a caller's stream, a replayed graph; the grid's
own cost plane after a roll."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grid_nav_cases as N
from slam_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in N.cases()]


def field_for(c):
    nf = api.NavField(c["sx"], c["sy"], c["orth_w"], c["diag_w"])
    nf.set_table(c["S"])
    return nf


def check_state(nf, c, want):
    """the flags of the state; returns it"""
    st = nf.state()
    used, skipped = N.split_goals(c["cost"], c["sx"], c["sy"], c["S"], c["goals"])
    assert (st.converged, st.goals_used, st.goals_skipped) == (1, len(used), skipped), vars(st)
    assert st.rounds >= 1 and st.tiles_processed >= (1 if used else 0)
    return st


def check_paths(nf, c, want, starts):
    cells = c["sx"] * c["sy"]
    for start in starts:
        wp, ws = N.walk(c["cost"], c["sx"], c["sy"], c["S"], want, start, cells, c["orth_w"], c["diag_w"])
        path, status = nf.path(start)
        print(c["name"], start, "length", len(path), "status", status, "want", len(wp), ws)
        assert status == ws and path.dtype == np.int32 and np.array_equal(path, wp)
        st = nf.state()
        assert (st.last_path_len, st.last_path_status) == (len(wp), ws)
        if len(wp) > 1:                                              # one short: cut, the cells it has are valid
            cut, status = nf.path(start, len(wp) - 1)
            assert status == N.CUT and np.array_equal(cut, wp[:-1])
            assert nf.state().last_path_len == len(wp) - 1
            exact, status = nf.path(start, len(wp))
            assert status == N.REACHED and np.array_equal(exact, wp)


@pytest.mark.parametrize("name", NAMES)
def test_field_paths_and_state_equal_the_restatement(name):
    c, want = N.case(name), N.expected(name)
    nf = field_for(c)
    nf.compute(c["cost"], c["goals"])
    pot = nf.potential()
    print(name, "cells that differ:", int((pot != want).sum()), "rounds", nf.state().rounds, "tiles", nf.state().tiles_processed)
    assert pot.dtype == np.uint32 and np.array_equal(pot, want)
    check_state(nf, c, want)
    check_paths(nf, c, want, N.starts_of(name) + ((-1, 0), (0, c["sy"]), (c["sx"], 0)))
    for x, y in N.split_goals(c["cost"], c["sx"], c["sy"], c["S"], c["goals"])[0][:1]:   # a start on a goal: length 1
        path, status = nf.path((x, y))
        assert status == N.REACHED and path.tolist() == [[x, y]]
    nf.close()


def test_saturation_reads_far_and_never_a_wrapped_number():
    c = N.case("1x300_saturation")
    nf = field_for(c)
    nf.compute(c["cost"], c["goals"])
    pot = nf.potential()
    assert pot[299] == N.FAR and pot[298] == 16 * N.SATURATION_MOVE and pot[265] == N.FAR and pot[266] == 16 * N.SATURATION_MOVE
    assert nf.path((0, 299))[1] == N.NO_START and nf.path((0, 298))[1] == N.REACHED
    nf.close()


def test_the_params_install_the_table_they_describe():
    c = N.case("random_97x83_d2")
    by_params = api.NavField(c["sx"], c["sy"], c["orth_w"], c["diag_w"], params=api.gnav_default_params(neutral=7))
    by_table = api.NavField(c["sx"], c["sy"], c["orth_w"], c["diag_w"])
    by_table.compute(c["cost"], c["goals"])
    default = by_table.potential()
    by_table.set_table(api.step_table(neutral=7))
    pots = []
    for nf in (by_params, by_table):
        nf.compute(c["cost"], c["goals"])
        pots.append(nf.potential())
        nf.close()
    assert np.array_equal(pots[0], pots[1]) and not np.array_equal(pots[0], default)


def test_too_few_rounds_then_a_continued_call():
    c, want = N.case("130x70_maze"), N.expected("130x70_maze")
    nf = field_for(c)
    d_cost = api.DeviceArray.from_host(c["cost"], np.uint8)
    nf.compute_dev(d_cost, c["goals"], rounds=3)
    st = nf.state()
    assert (st.rounds, st.converged) == (3, 0) and 1 <= st.tiles_processed <= 3 * 6
    early = nf.potential()
    assert (early >= want).all() and (early != want).any() and early[0] == 0
    path, status = nf.path((129, 68))
    assert status == N.NOT_CONVERGED and len(path) == 0
    d_path, d_ls = api.DeviceArray((16, 2), np.int32), api.DeviceArray((2,), np.int32)
    nf.path_dev((0, 0), 16, d_path, d_ls)
    assert d_ls.download().tolist() == [0, N.NOT_CONVERGED]
    nf.compute_dev(d_cost, c["goals"], rounds=600, restart=False)    # continues: the goals are not read again
    st = nf.state()
    print("maze: rounds", st.rounds, "tiles processed", st.tiles_processed)
    assert (st.rounds, st.converged) == (603, 1)
    assert np.array_equal(nf.potential(), want)
    check_paths(nf, c, want, c["starts"])
    nf.close()
    d_cost.free()


def test_the_host_form_gives_up_at_max_rounds():
    c = N.case("130x70_maze")
    nf = field_for(c)
    with pytest.raises(api.SlamError) as e:
        nf.compute(c["cost"], c["goals"], max_rounds=1)
    assert e.value.code == api.E_TIMEOUT and "slam_gnav_compute" in str(e.value)
    st = nf.state()
    assert (st.rounds, st.converged) == (1, 0)
    assert nf.path((129, 68))[1] == N.NOT_CONVERGED
    nf.compute(c["cost"], c["goals"])                                # and to the end: max_rounds 0
    assert np.array_equal(nf.potential(), N.expected("130x70_maze"))
    nf.close()


def test_one_handle_three_planes():
    """each plane is emptier or fuller than the one before: stale potentials, flags, counts or tables would show"""
    names = ("random_97x83_d2", "random_97x83_d0", "random_97x83_unknown_400", "random_97x83_random_table", "random_97x83_d2")
    nf = api.NavField(97, 83)
    for name in names:
        c, want = N.case(name), N.expected(name)
        nf.set_table(c["S"])
        nf.compute(c["cost"], c["goals"])
        assert np.array_equal(nf.potential(), want), name
        check_state(nf, c, want)
        check_paths(nf, c, want, N.starts_of(name)[-3:])
    nf.close()


def test_compute_dev_and_path_dev_on_a_stream():
    c, want = N.case("130x70_five_goals"), N.expected("130x70_five_goals")
    nf = field_for(c)
    st = api.Stream()
    d_cost, d_goals = api.DeviceArray.from_host(c["cost"], np.uint8), api.DeviceArray.from_host(c["goals"], np.int32)
    d_path, d_ls = api.DeviceArray((400, 2), np.int32), api.DeviceArray((2,), np.int32)
    nf.compute_dev(d_cost, d_goals, rounds=24, stream=st)
    nf.path_dev((64, 30), 400, d_path, d_ls, stream=st)
    st.synchronize()
    assert np.array_equal(nf.potential(), want)
    check_state(nf, c, want)
    wp, ws = N.expected_path(c["name"], (64, 30))
    n, status = d_ls.download().tolist()
    assert (n, status) == (len(wp), ws) and np.array_equal(d_path.download()[:n], wp)
    raw = np.empty(c["sx"] * c["sy"], np.uint32)
    api.check(api.lib().slam_memcpy_d2h(raw.ctypes.data_as(C.c_void_p), nf.potential_dev(), raw.nbytes, None))
    assert np.array_equal(raw, want)
    nf.close()
    for d in (d_cost, d_goals, d_path, d_ls):
        d.free()


def test_a_graph_replayed_with_the_goal_buffer_rewritten():
    c = N.case("130x70_goal_0_0")
    sx, sy = c["sx"], c["sy"]
    nf = field_for(c)
    st = api.Stream()
    d_cost = api.DeviceArray.from_host(c["cost"], np.uint8)
    d_goals = api.DeviceArray.from_host(np.array([[0, 0], [-1, -1]], np.int32))
    d_path, d_ls = api.DeviceArray((400, 2), np.int32), api.DeviceArray((2,), np.int32)
    start, rounds = (129, 69), 25

    def sequence():
        nf.compute_dev(d_cost, d_goals, rounds=rounds, stream=st)
        nf.path_dev(start, 400, d_path, d_ls, stream=st)

    sequence()                                                       # warm-up
    st.synchronize()
    with api.Graph(st) as g:
        sequence()
    for goals in ([[0, 0], [-1, -1]], [[64, 64], [63, 63]], [[129, 0], [500, 500]], [[0, 0], [-1, -1]]):
        d_goals.upload(np.array(goals, np.int32))
        g.launch()
        st.synchronize()
        want = N.dijkstra(c["cost"], sx, sy, c["S"], goals)
        assert np.array_equal(nf.potential(), want), goals
        state = nf.state()
        used, skipped = N.split_goals(c["cost"], sx, sy, c["S"], goals)
        assert (state.rounds, state.converged, state.goals_used, state.goals_skipped) == (rounds, 1, len(used), skipped)
        wp, ws = N.walk(c["cost"], sx, sy, c["S"], want, start, 400)
        n, status = d_ls.download().tolist()
        assert (n, status) == (len(wp), ws) and np.array_equal(d_path.download()[:n], wp)
    nf.close()
    for d in (d_cost, d_goals, d_path, d_ls):
        d.free()


def test_refusals_on_a_live_handle():
    L, vp = api.lib(), C.c_void_p
    nf = api.NavField(10, 10)
    d = api.DeviceArray((100,), np.int32)
    for call in (lambda: L.slam_gnav_compute_dev(nf.h, d.ptr, d.ptr, 0, 1, 1, None), lambda: L.slam_gnav_compute_dev(nf.h, d.ptr, d.ptr, 1, -1, 1, None),
                 lambda: L.slam_gnav_compute_dev(nf.h, d.ptr, d.ptr, 1, 1, 0, None), lambda: L.slam_gnav_path_dev(nf.h, 0, 0, 0, d.ptr, d.ptr, None),
                 lambda: L.slam_gnav_path_dev(nf.h, 0, 0, 5, d.ptr, d.ptr, None)):
        assert call() == api.E_INVALID and b"slam_gnav_" in L.slam_last_error()
    with pytest.raises(api.SlamError):
        nf.potential()                                               # nothing has been computed
    with pytest.raises(api.SlamError):
        nf.set_table(np.zeros(255, np.uint32))
    t = api.step_table()
    t[0] = (1 << 20) + 1
    with pytest.raises(api.SlamError):
        nf.set_table(t)
    st = nf.state()
    assert (st.rounds, st.converged, st.goals_used) == (0, 0, 0)
    nf.close()
    d.free()


# ------------------------------------------------------------------------------------------------ the grid's own cost plane
SIZE_X, SIZE_Y, RES, R = 200, 160, 0.25, 8


def room_grid():
    """synth.py's room (40 x 30 m, four pillars) in a rolling grid of 50 x 40 m: the walls as obstacle points, then a roll of
    (+7, -5) cells, then a ground point at every cell centre inside the room; finalized"""
    g = api.Grid(SIZE_X, SIZE_Y, RES, rolling=1, min_cluster_points=0)
    m_ga, m_nga = synth.make_map(6000)
    g.add_endpoints(np.concatenate([m_ga, m_nga]).astype(np.float32), np.zeros((0, 2), np.float32))
    g.set_pose(7 * RES, -5 * RES)
    assert g.window_cell() == (7, -5)
    c = np.asarray(g.get_pose(), np.float64)
    xs = np.arange(-synth.ROOM_W / 2 + RES / 2, synth.ROOM_W / 2, RES)
    ys = np.arange(-synth.ROOM_H / 2 + RES / 2, synth.ROOM_H / 2, RES)
    gnd = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    g.add_endpoints(np.zeros((0, 2), np.float32), (gnd - c).astype(np.float32))
    g.finalize()
    return g


def test_grid_to_distance_field_to_nav_field_after_a_roll():
    g = room_grid()
    df = api.DistanceField(SIZE_X, SIZE_Y, max_cells=R)
    df.set_inflation(RES, 0.3, 1.5, 2.0)
    nf = api.NavField(SIZE_X, SIZE_Y)
    occ = g.read_occupancy()
    assert (occ == 100).sum() > 200 and (occ == 0).sum() > 5000 and (occ == -1).sum() > 5000
    free = np.flatnonzero(occ == 0)
    goals = np.array([[free[len(free) // 3] % SIZE_X, free[len(free) // 3] // SIZE_X], [-4, 2], [0, 0]], np.int32)   # (0, 0) is unknown: closed
    g.distance_field(df)
    g.nav_field(df, nf, goals, rounds=40)
    cost = df.read()[1]
    S = N.step_table()
    want = N.dijkstra(cost, SIZE_X, SIZE_Y, S, goals)
    pot = nf.potential()
    assert np.array_equal(pot, want)
    st = nf.state()
    assert (st.rounds, st.converged, st.goals_used, st.goals_skipped) == (40, 1, 1, 2)
    finite = np.flatnonzero(want != N.FAR)
    assert len(finite) > 5000 and (want[occ == -1] == N.FAR).all() and (want[occ == 100] == N.FAR).all()
    c = dict(name="room", sx=SIZE_X, sy=SIZE_Y, cost=cost, S=S, orth_w=N.ORTH_W, diag_w=N.DIAG_W)
    far_cell = finite[np.argmax(want[finite])]
    check_paths(nf, c, want, [(far_cell % SIZE_X, far_cell // SIZE_X), (finite[0] % SIZE_X, finite[0] // SIZE_X), (0, 0)])
    # handles of different sizes, and a distance field without a table
    for sx, sy in ((SIZE_X, SIZE_Y + 1), (SIZE_X - 1, SIZE_Y)):
        other = api.NavField(sx, sy)
        with pytest.raises(api.SlamError) as e:
            g.nav_field(df, other, goals)
        assert e.value.code == api.E_INVALID and "slam_grid_nav_field" in str(e.value)
        other.close()
        odf = api.DistanceField(sx, sy, max_cells=R)
        with pytest.raises(api.SlamError) as e:
            g.nav_field(odf, nf, goals)
        assert e.value.code == api.E_INVALID
        odf.close()
    bare = api.DistanceField(SIZE_X, SIZE_Y, max_cells=R)
    with pytest.raises(api.SlamError) as e:
        g.nav_field(bare, nf, goals)
    assert e.value.code == api.E_INVALID and "table" in str(e.value)
    for h in (bare, nf, df, g):
        h.close()


# ----------------------------------------------------------------------------------------------------------- the C++ adapter
def room_clouds(pose):
    """the room's walls as obstacle points and a ground point at every cell centre inside it, in the frame of a window at `pose`"""
    m_ga, m_nga = synth.make_map(6000)
    xs = np.arange(-synth.ROOM_W / 2 + RES / 2, synth.ROOM_W / 2, RES)
    ys = np.arange(-synth.ROOM_H / 2 + RES / 2, synth.ROOM_H / 2, RES)
    obs, gnd = np.concatenate([m_ga, m_nga]), np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    out = []
    for pts in (obs, gnd):
        a = np.zeros((len(pts), 4), np.float32)
        a[:, :2] = pts - np.asarray(pose)
        out.append(a)
    return out


def test_cpp_adapter_nav_field_and_plan_path(tmp_path):
    exe = str(tmp_path / "nav_field_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "nav_field_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    d = str(tmp_path)
    # the field alone: a case with its own table and weights
    c = N.case("random_97x83_unknown_400")
    start = N.starts_of(c["name"])[-3]
    c["cost"].tofile(os.path.join(d, "plane.u8"))
    c["goals"].tofile(os.path.join(d, "goals.i32"))
    np.array([c["sx"], c["sy"], c["orth_w"], c["diag_w"], N.NEUTRAL, N.LETHAL_FROM, 400, start[0], start[1]], np.float64).tofile(os.path.join(d, "plane.f64"))
    # the map: two clouds at two poses, the second one rolling the window by (+7, -5) cells
    pose1, inscribed, infl, scaling = (7 * RES, -5 * RES), 0.3, 1.5, 2.0
    frm, to = (-15.2, -10.1), (15.3, 10.4)
    clouds = [room_clouds((0.0, 0.0)), room_clouds(pose1)]
    for k, (obs, gnd) in enumerate(clouds):
        obs.tofile(os.path.join(d, "obs%d.f32" % k))
        gnd.tofile(os.path.join(d, "gnd%d.f32" % k))
    np.array([SIZE_X, SIZE_Y, RES, pose1[0], pose1[1], inscribed, infl, scaling, R, frm[0], frm[1], to[0], to[1]], np.float64).tofile(os.path.join(d, "params.f64"))
    subprocess.check_call([exe, d], timeout=120)

    def load(name, dt):
        return np.fromfile(os.path.join(d, name), dt)

    # ---- the field alone against the Python binding, bit for bit, and so against the restatement
    nf = field_for(c)
    nf.compute(c["cost"], c["goals"])
    path, status = nf.path(start)
    st = nf.state()
    assert np.array_equal(load("a_pot.u32", np.uint32), nf.potential()) and np.array_equal(nf.potential(), N.expected(c["name"]))
    assert np.array_equal(load("a_path.i32", np.int32).reshape(-1, 2), path) and status == N.REACHED and len(path) > 10
    a_state = load("a_state.i64", np.int64)
    assert a_state[1:4].tolist() == [st.converged, st.goals_used, st.goals_skipped] == [1, 2, 0]
    assert a_state[5:].tolist() == [len(path), N.REACHED, N.REACHED]
    nf.close()
    # ---- the map's planner against Grid -> DistanceField -> NavField fed the same clouds
    g = api.Grid(SIZE_X, SIZE_Y, RES, rolling=1, min_cluster_points=0)
    for (obs, gnd), pose in zip(clouds, ((0.0, 0.0), pose1)):
        g.set_pose(*pose)
        g.add_scan_inorder(obs, gnd)
    px, py = g.get_pose()
    df = api.DistanceField(SIZE_X, SIZE_Y, max_cells=R)
    df.set_inflation(RES, inscribed, infl, scaling)
    nf = api.NavField(SIZE_X, SIZE_Y)

    def cell(wx, wy):                                                # the grid's own binning of a float point in the window's frame
        return (int(float(np.float32(wx - px)) / RES + SIZE_X // 2), int(float(np.float32(wy - py)) / RES + SIZE_Y // 2))

    meta = load("b_meta.f64", np.float64)
    assert meta[1:5].tolist() == list(cell(*frm) + cell(*to))
    assert meta[5:].tolist() == [N.NO_START, 0, N.NO_START, 0]       # a start or a goal outside the window
    g.distance_field(df)
    g.nav_field(df, nf, np.array([cell(*to)], np.int32), rounds=40)
    cost = df.read()[1]
    assert np.array_equal(load("b_cost.u8", np.uint8), cost)
    pot = nf.potential()
    assert nf.state().converged == 1 and np.array_equal(load("b_pot.u32", np.uint32), pot)
    assert np.array_equal(pot, N.dijkstra(cost, SIZE_X, SIZE_Y, N.step_table(), [cell(*to)]))
    path, status = nf.path(cell(*frm))
    cells = load("b_cells.i32", np.int32).reshape(-1, 2)
    assert meta[0] == status == N.REACHED and len(path) > 100 and np.array_equal(cells, path)
    assert tuple(cells[0]) == cell(*frm) and tuple(cells[-1]) == cell(*to)
    points = load("b_points.f64", np.float64).reshape(-1, 2)
    want = np.stack([((path[:, 0] - SIZE_X // 2) + 0.5) * RES + px, ((path[:, 1] - SIZE_Y // 2) + 0.5) * RES + py], -1)
    assert np.array_equal(points, want)
    assert np.abs(points[0] - frm).max() <= RES and np.abs(points[-1] - to).max() <= RES
    for h in (nf, df, g):
        h.close()
