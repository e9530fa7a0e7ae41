"""The navigation field's restatement against itself, the step table and every refusal of the entry points -- no GPU
(docs/GRID_NAV.md section 4).  The device is held to the same restatement in tests/test_gpu_grid_nav.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_nav_cases as N
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in N.cases()]


@pytest.fixture(scope="module")
def L():
    return api.lib()


def test_the_case_list_is_what_the_kernels_need():
    assert N.TILE == 64 and len(set(NAMES)) == len(NAMES)
    src = open(os.path.join(ROOT, "slam_amd", "csrc", "grid_nav.hip")).read()
    assert re.search(r"constexpr int\s+kTile = %d;" % N.TILE, src)
    shapes = {(c["sx"], c["sy"]) for c in N.cases()}
    assert {(1, 1), (1, 300), (300, 1), (63, 5), (64, 64), (65, 67), (130, 70), (97, 83)} <= shapes


@pytest.mark.parametrize("name", NAMES)
def test_the_two_forms_agree(name):
    c = N.case(name)
    bf = N.bellman_ford(c["cost"], c["sx"], c["sy"], c["S"], c["goals"], c["orth_w"], c["diag_w"])
    want = N.expected(name)
    assert want.dtype == np.uint32 and np.array_equal(bf, want)
    step = c["S"][c["cost"]]
    assert (want[step == 0] == N.FAR).all()                          # closed cells are FAR
    used, skipped = N.expected_goal_counts(name)
    assert used + skipped == len(c["goals"])
    for x, y in N.split_goals(c["cost"], c["sx"], c["sy"], c["S"], c["goals"])[0]:
        assert want[x + c["sx"] * y] == 0
    assert ((want == 0).sum() == len(set(N.split_goals(c["cost"], c["sx"], c["sy"], c["S"], c["goals"])[0])))
    if used == 0:
        assert (want == N.FAR).all()


@pytest.mark.parametrize("name", NAMES)
def test_every_path_is_a_shortest_path(name):
    c = N.case(name)
    want = N.expected(name)
    assert c["starts"]
    for start in N.starts_of(name):
        path, status = N.expected_path(name, start)
        i = start[0] + c["sx"] * start[1]
        if c["S"][c["cost"][i]] == 0 or want[i] == N.FAR:
            assert status == N.NO_START and len(path) == 0
            continue
        assert status == N.REACHED and tuple(path[0]) == tuple(start)
        N.check_path(c["cost"], c["sx"], c["sy"], c["S"], want, path, c["goals"], c["orth_w"], c["diag_w"])
        if len(path) > 1:                                            # one short: cut, and the cells it has are the same
            cut, status = N.expected_path(name, start, len(path) - 1)
            assert status == N.CUT and np.array_equal(cut, path[:-1])
    assert N.walk(c["cost"], c["sx"], c["sy"], c["S"], want, (-1, 0), 10)[1] == N.NO_START
    assert N.walk(c["cost"], c["sx"], c["sy"], c["S"], want, c["starts"][0], 10, converged=False)[1] == N.NOT_CONVERGED


def test_what_the_cases_are_there_for():
    far = N.FAR
    # saturation: the far end is FAR, the cell before it holds its true value; 16 moves fit, 17 do not
    p = N.expected("1x300_saturation")
    m = N.SATURATION_MOVE
    assert 16 * m < far <= 17 * m
    assert p[299] == far and p[298] == 16 * m and p[266] == 16 * m and p[265] == far and p[282] == 0
    # a goal on a lethal cell and goals outside the plane are skipped and counted
    assert N.expected_goal_counts("130x70_goal_on_lethal") == (2, 4)
    assert N.expected_goal_counts("130x70_only_invalid_goals") == (0, 4) and (N.expected("130x70_only_invalid_goals") == far).all()
    # the closed wall and the closed room
    p = N.expected("130x70_wall_closed").reshape(70, 130)
    assert (p[:, 63:] == far).all() and (p[:, :63] != far).all()
    p = N.expected("130x70_room").reshape(70, 130)
    assert (p[20:41, 70:91] == far).all() and (p != far).sum() == 130 * 70 - 21 * 21
    # the corner: open, the diagonal across the four tiles is taken; with one side lethal, the way round through the other
    s = 50
    open_, closed = N.expected("130x70_corner_open").reshape(70, 130), N.expected("130x70_corner_side_lethal").reshape(70, 130)
    assert open_[64, 64] == open_[63, 63] + 17 * (s + s)
    assert closed[63, 63] == open_[63, 63] and closed[64, 64] == closed[63, 63] + 12 * (s + 250) + 12 * (250 + s) and closed[63, 64] == far
    assert N.expected_path("130x70_corner_open", (64, 64))[0][1].tolist() == [63, 63]
    assert N.expected_path("130x70_corner_side_lethal", (64, 64))[0][1].tolist() == [63, 64]
    # the maze's shortest path runs every corridor: far more cells than the plane is long, and it re-enters the tiles
    path, status = N.expected_path("130x70_maze", (129, 68))
    assert status == N.REACHED and len(path) > 30 * 130
    # ties on the open plane go to the lowest direction: from (0, 0) towards (32, 33) the diagonal d = 1 before d = 2
    path, _ = N.expected_path("65x67_open_ties", (0, 0))
    assert path[1].tolist() == [1, 1] and path[-1].tolist() == [32, 33] and len(path) == 34
    path, _ = N.expected_path("65x67_open_ties", (64, 40))
    assert path[1].tolist() == [63, 40] and len(path) == 33          # d = 4 (-1, 0) and d = 5 (-1, -1) both continue: d = 4 is taken
    # a border cell that falls late by exactly 65 536: through X in the first round, through the detour ten crossings later
    b, t = 63 + 130 * 10, N.late_table()
    through_x = N.dijkstra(N.late_drop_130x70(detour_open=False), 130, 70, t, [(0, 10)], 1, 1)[b]
    detour = N.dijkstra(N.late_drop_130x70(x_open=False), 130, 70, t, [(0, 10)], 1, 1)[b]
    assert int(through_x) - int(detour) == 65536 and N.expected("130x70_late_drop")[b] == detour == 394
    # a corner cell that falls late while the diagonal's side cells stay: (64, 64) is reached through the corner alone
    p = N.expected("130x70_late_corner").reshape(70, 130)
    side = N.LATE_SIDE_STEP
    assert p[63, 63] == 288 and p[64, 64] == 290 and p[63, 64] == 232 + 1 + side and p[64, 63] == 248 + 1 + side
    assert p[63, 64] < p[63, 63] + 1 + side and p[64, 63] < p[63, 63] + 1 + side       # the side cells owe (63, 63) nothing
    assert N.expected_path("130x70_late_corner", (100, 64))[0][37].tolist() == [63, 63]
    # the unknown cells: closed at step 0, open at 400
    a, b = N.expected("random_97x83_unknown_closed"), N.expected("random_97x83_unknown_400")
    unknown = N.case("random_97x83_unknown_closed")["cost"] == N.UNKNOWN
    assert unknown.sum() > 2000 and (a[unknown] == far).all() and (b[unknown] != far).sum() > 2000 and (b <= a).all()


# ------------------------------------------------------------------------------------------------------------ the step table
def test_the_table_maker_against_its_formula(L):
    d = api.gnav_default_params()
    assert [f for f, _ in d._fields_] == ["orth_w", "diag_w", "neutral", "lethal_from", "unknown_step"]
    assert (d.orth_w, d.diag_w, d.neutral, d.lethal_from, d.unknown_step) == (12, 17, 50, 253, 0)
    assert (api.GNAV_REACHED, api.GNAV_NO_START, api.GNAV_CUT, api.GNAV_NOT_CONVERGED) == (0, 1, 2, 3)
    assert [f for f, _ in api.GnavState._fields_] == ["rounds", "converged", "goals_used", "goals_skipped", "tiles_processed", "last_path_len",
                                                      "last_path_status"]
    assert (N.ORTH_W, N.DIAG_W, N.NEUTRAL, N.LETHAL_FROM, N.UNKNOWN_STEP) == (12, 17, 50, 253, 0)
    assert api.GNAV_FAR == N.FAR == 0xFFFFFFFF
    t = api.step_table()
    assert t.dtype == np.uint32 and np.array_equal(t, N.step_table())
    assert t[0] == 50 and t[252] == 302 and t[253] == t[254] == t[255] == 0
    for neutral in (1, 50, 1 << 19):
        for lethal_from in (1, 100, 253, 256):
            for unknown_step in (0, 400, 1 << 20):
                t = api.step_table(neutral, lethal_from, unknown_step)
                assert np.array_equal(t, N.step_table(neutral, lethal_from, unknown_step))
                c = np.arange(255)
                assert np.array_equal(t[:255], np.where(c < lethal_from, neutral + c, 0)) and t[255] == unknown_step
                assert t.max() <= 1 << 20


def test_the_table_maker_refuses(L):
    vp = C.c_void_p
    for args in ((0, 253, 0), (-1, 253, 0), ((1 << 19) + 1, 253, 0), (50, 0, 0), (50, 257, 0), (50, -3, 0), (50, 253, -1),
                 (50, 253, (1 << 20) + 1)):
        t = np.full(256, 7, np.uint32)
        assert L.slam_grid_step_table(*args, t.ctypes.data_as(vp), 256) == api.E_INVALID
        assert b"slam_grid_step_table" in L.slam_last_error() and (t == 7).all()
        with pytest.raises(api.SlamError):
            api.step_table(*args)
    for n in (255, 257, 0, -1):
        t = np.full(257, 7, np.uint32)
        assert L.slam_grid_step_table(50, 253, 0, t.ctypes.data_as(vp), n) == api.E_INVALID and (t == 7).all()
    assert L.slam_grid_step_table(50, 253, 0, None, 256) == api.E_INVALID


def test_table_header_alone_under_the_sanitizers(tmp_path):
    src = open(os.path.join(ROOT, "slam_amd", "csrc", "grid_nav_table.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["cstdint"]                 # no HIP, no library
    exe = str(tmp_path / "grid_nav_table_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "grid_nav_table_check.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok"


def test_the_scalar_cpp_form_agrees(tmp_path):
    """tests/cpp/grid_nav_oracle.cpp, the form tools/grid_nav_time.py times beside the device, on the cases that bend a rule"""
    exe = str(tmp_path / "grid_nav_oracle")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "grid_nav_oracle.cpp"), "-o", exe])
    for name in ("1x1", "130x70_goal_on_lethal", "130x70_only_invalid_goals", "130x70_corner_open", "130x70_corner_side_lethal", "130x70_maze_costs",
                 "1x300_saturation", "random_97x83_d2", "random_97x83_unknown_400", "random_97x83_random_table"):
        c = N.case(name)
        files = [str(tmp_path / f) for f in ("cost.u8", "table.u32", "goals.i32", "pot.u32")]
        for a, f in zip((c["cost"], c["S"], c["goals"]), files):
            a.tofile(f)
        subprocess.check_call([exe, files[0], str(c["sx"]), str(c["sy"]), files[1], str(c["orth_w"]), str(c["diag_w"]), files[2], files[3]],
                              stdout=subprocess.DEVNULL, timeout=120)
        assert np.array_equal(np.fromfile(files[3], np.uint32), N.expected(name)), name


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_every_entry_point_refuses_before_a_device_is_touched(L):
    """SLAM_E_INVALID with the function's name in the message, on a machine with or without a GPU.  `fake` stands for a live
    handle where the refusal is of another argument: zeroed memory that the call must not get as far as using."""
    vp, inv = C.c_void_p, api.E_INVALID
    fake = C.create_string_buffer(4096)
    buf = np.zeros(1024, np.int32)
    p = buf.ctypes.data_as(vp)
    h = vp()

    def refused(name, *args):
        assert getattr(L, name)(*args) == inv, name
        assert name.encode() in L.slam_last_error(), (name, L.slam_last_error())

    for sx, sy in ((0, 5), (5, 0), (-1, 5), (5, -1), (32768, 5), (5, 32768)):
        for params in (None, C.byref(api.gnav_default_params())):    # null params are the defaults
            h.value = 5
            refused("slam_gnav_create", sx, sy, params, C.byref(h))
            assert not h.value                                       # the out pointer is nulled
    for ow, dw in ((0, 17), (12, 0), (256, 17), (12, 256), (-1, 17), (12, -5)):
        refused("slam_gnav_create", 10, 10, C.byref(api.gnav_default_params(orth_w=ow, diag_w=dw)), C.byref(h))
    # the table's parameters, by the bounds of slam_grid_step_table (test_the_table_maker_refuses)
    for neutral, lethal_from, unknown_step in ((0, 253, 0), (-1, 253, 0), ((1 << 19) + 1, 253, 0), (50, 0, 0), (50, 257, 0), (50, -3, 0),
                                               (50, 253, -1), (50, 253, (1 << 20) + 1)):
        h.value = 5
        refused("slam_gnav_create", 10, 10, C.byref(api.gnav_default_params(neutral=neutral, lethal_from=lethal_from, unknown_step=unknown_step)),
                C.byref(h))
        assert not h.value
    refused("slam_gnav_create", 10, 10, C.byref(api.gnav_default_params()), None)
    refused("slam_gnav_create", 10, 10, None, None)
    L.slam_gnav_destroy(None)                                        # a null handle is nothing to free
    good = api.step_table()
    refused("slam_gnav_set_table", None, good.ctypes.data_as(vp), 256)
    refused("slam_gnav_set_table", fake, None, 256)
    for n in (255, 257, 0):
        refused("slam_gnav_set_table", fake, good.ctypes.data_as(vp), n)
    high = good.copy()
    high[9] = (1 << 20) + 1
    refused("slam_gnav_set_table", fake, high.ctypes.data_as(vp), 256)
    # the device form
    refused("slam_gnav_compute_dev", None, p, p, 1, 1, 1, None)
    refused("slam_gnav_compute_dev", fake, None, p, 1, 1, 1, None)
    refused("slam_gnav_compute_dev", fake, p, None, 1, 1, 1, None)
    refused("slam_gnav_compute_dev", fake, p, p, 0, 1, 1, None)
    refused("slam_gnav_compute_dev", fake, p, p, -4, 1, 1, None)
    refused("slam_gnav_compute_dev", fake, p, p, 1, -1, 1, None)
    refused("slam_gnav_compute_dev", fake, p, p, 1, 1, 0, None)      # nothing to continue: no restart yet
    # the host form
    refused("slam_gnav_compute", None, p, p, 1, 0)
    refused("slam_gnav_compute", fake, None, p, 1, 0)
    refused("slam_gnav_compute", fake, p, None, 1, 0)
    refused("slam_gnav_compute", fake, p, p, 0, 0)
    refused("slam_gnav_compute", fake, p, p, 1, -1)
    # read-back
    refused("slam_gnav_read", None, p)
    refused("slam_gnav_read", fake, None)
    refused("slam_gnav_read", fake, p)                               # nothing has been computed
    refused("slam_gnav_potential_dev", None, C.byref(h))
    refused("slam_gnav_potential_dev", fake, None)
    refused("slam_gnav_read_state", None, C.byref(api.GnavState()))
    refused("slam_gnav_read_state", fake, None)
    # the path
    n, st = C.c_int(), C.c_int()
    refused("slam_gnav_path_dev", None, 0, 0, 10, p, p, None)
    refused("slam_gnav_path_dev", fake, 0, 0, 10, None, p, None)
    refused("slam_gnav_path_dev", fake, 0, 0, 10, p, None, None)
    refused("slam_gnav_path_dev", fake, 0, 0, 0, p, p, None)
    refused("slam_gnav_path_dev", fake, 0, 0, -3, p, p, None)
    refused("slam_gnav_path_dev", fake, 0, 0, 10, p, p, None)        # nothing has been computed
    refused("slam_gnav_path", None, 0, 0, 10, p, C.byref(n), C.byref(st))
    refused("slam_gnav_path", fake, 0, 0, 10, None, C.byref(n), C.byref(st))
    refused("slam_gnav_path", fake, 0, 0, 10, p, None, C.byref(st))
    refused("slam_gnav_path", fake, 0, 0, 10, p, C.byref(n), None)
    refused("slam_gnav_path", fake, 0, 0, 0, p, C.byref(n), C.byref(st))
    # the grid's own
    refused("slam_grid_nav_field", None, fake, fake, p, 1, 0, None)
    refused("slam_grid_nav_field", fake, None, fake, p, 1, 0, None)
    refused("slam_grid_nav_field", fake, fake, None, p, 1, 0, None)
    refused("slam_grid_nav_field", fake, fake, fake, None, 1, 0, None)
    refused("slam_grid_nav_field", fake, fake, fake, p, 0, 0, None)
    refused("slam_grid_nav_field", fake, fake, fake, p, 1, -1, None)
    L.slam_gnav_default_params(None)                                 # a null pointer: nothing to fill
    assert issubclass(api.NavField, api._Handle) and api.NavField._destroy in api.EXPORTS
    assert "close" not in vars(api.NavField) and "__del__" not in vars(api.NavField)
