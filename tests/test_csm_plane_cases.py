"""The matcher over a byte plane (docs/GRID_MATCH.md) without a GPU: the two numpy forms of the score volume agree on every case
of tests/csm_plane_cases.py, the host's likelihood table (slam_grid_likelihood_table, which needs no device) is the formula,
argument errors answer before any device question, the table header alone survives its extreme arguments under the host
sanitizers, header, exports and ctypes mirror agree, and the two rehearsals of the accuracy condition hold on the restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import csm_oracle
import csm_plane_cases as P
from slam_amd import api, synth
from slam_amd.api import GridMatcher, likelihood_table  # noqa: F401  (what this file is about: without them nothing here holds)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["slam_grid_likelihood_table", "slam_csm_create_from_plane", "slam_csm_create_from_plane_dev", "slam_csm_set_plane_dev",
       "slam_csm_score_poses_dev", "slam_csm_score_poses"]


@pytest.fixture(scope="module")
def L():
    return api.lib()


# ------------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("name", [c["name"] for c in P.cases()])
def test_the_two_volume_forms_agree(name):
    c = P.case(name)
    vol, cnt = P.expected(name)
    vol2, cnt2 = P.volume_direct((c["ox"], c["oy"], c["plane"]), c["pts"], P.case_angles(c), c["t0"], c["res"], c["half_x"], c["half_y"])
    assert np.array_equal(vol, vol2) and np.array_equal(cnt, cnt2)
    assert (cnt == len(c["pts"])).all()                                        # a point outside the window is counted
    if name.endswith("_outside"):
        assert not vol.any()
    elif name != "1x1_half":
        assert vol.any()


def test_the_case_list_reaches_what_it_names():
    vol, cnt = P.expected("tie")
    assert (vol == 9 * 50).all()                                               # an exact tie of every candidate
    c = P.case("tie")
    _, t, r = P.match(vol, cnt, 50, P.case_angles(c), c["t0"], c["res"], c["half_x"], c["half_y"])
    assert (r["k"], r["b"], r["a"]) == (0, 0, 0) and t.tolist() == [-5 * P.RES, -5 * P.RES]
    _, t, r = P.match(*P.expected("four_points"), 4, None, (1.0, 2.0), P.RES, 6, 5)
    assert r["score"] == -1 and t.tolist() == [1.0, 2.0]
    # W: the slide reaches D - 1 cells towards smaller indices and no further
    T, W = P.tables(np.array([[0, 0, 0], [0, 7, 0], [0, 0, 3]], np.uint8), 2)
    assert W.tolist() == [[0, 0, 0, 0], [0, 7, 7, 0], [0, 7, 7, 3], [0, 0, 3, 3]]
    T, W = P.tables(np.array([[5]], np.uint8), 1)
    assert W.tolist() == [[5]]
    # the scorer counts a point outside the table with score 0, and nothing at a non-finite pose
    tab = (0, 0, np.full((4, 4), 2, np.uint8))
    pts = np.array([[0.0, 0.0], [0.25, 0.25], [100.0, 0.0]])
    s, n = P.score_poses((tab, tab), pts, 1, [[1, 0, 0, 0], [1, 0, np.nan, 0], [np.inf, 0, 0, 0], [1, 0, 0, -1e300]], P.RES)
    assert s.tolist() == [4, 0, 0, 0] and n.tolist() == [3, 0, 0, 0]
    s, n = P.score_poses((tab, None), pts, 1, [[1, 0, 0, 0]], P.RES)           # a class without a table is not counted
    assert s.tolist() == [2] and n.tolist() == [1]


# ------------------------------------------------------------------------------------------------------ the likelihood table
def test_likelihood_table_by_hand(L):
    t = api.likelihood_table(0.1, 0.2, 6)
    assert t.dtype == np.uint8 and len(t) == 38
    assert t[0] == 255 and t[1] == 225 and t[36] == 3 and t[37] == 0


@pytest.mark.parametrize("res,sigma,R", [(0.1, 0.2, 6), (0.5, 0.5, 3), (0.05, 0.2, 12), (0.1, 0.2, 1), (0.05, 1.0, 254), (0.125, 0.3, 64),
                                         (1.0, 1e-3, 5), (1e-3, 1.0, 9)])
def test_likelihood_table_is_the_formula(L, res, sigma, R):
    t = api.likelihood_table(res, sigma, R)
    want, real = P.likelihood_table_np(res, sigma, R)
    assert len(t) == R * R + 2 and t[R * R + 1] == 0 and t[0] == 255
    assert (np.diff(t[:R * R + 1].astype(int)) <= 0).all()
    inner = np.arange(R * R + 2) <= R * R
    clear = inner & (np.abs(real - np.floor(real) - 0.5) > 1e-9)             # libm and numpy may differ in the last ulp: only there
    assert np.array_equal(t[clear], want[clear])
    assert (np.abs(t.astype(int) - want.astype(int)) <= 1).all()
    # entry i * i + j * j is the matcher's stamp entry (i, j): the expression of docs/CSM.md section 2, here by numpy
    i, j = 2, min(3, R - 1) if R > 2 else 0
    if i <= R and j <= R and i * i + j * j <= R * R:
        d2 = float(i * i + j * j)
        stamp = 255.0 * np.exp(-(d2 * (res * res)) / (2.0 * (sigma * sigma)))
        assert abs(int(t[i * i + j * j]) - stamp) <= 0.5 + 1e-9


def test_likelihood_table_refusals(L):
    n = 6 * 6 + 2
    bad = [((0.1, 0.2, 6, n - 1), "entries"), ((0.1, 0.2, 6, n + 1), "entries"), ((float("nan"), 0.2, 6, n), "non-finite"),
           ((0.1, float("nan"), 6, n), "non-finite"), ((float("inf"), 0.2, 6, n), "non-finite"), ((0.1, float("inf"), 6, n), "non-finite"),
           ((-0.1, 0.2, 6, n), "resolution"), ((0.0, 0.2, 6, n), "resolution"), ((0.1, -0.2, 6, n), "sigma"), ((0.1, 0.0, 6, n), "sigma"),
           ((0.1, 0.2, 0, 2), "max_cells"), ((0.1, 0.2, 255, 255 * 255 + 2), "max_cells"), ((0.1, 0.2, -1, 3), "max_cells"),
           ((5e-324, 0.2, 6, n), "range of a double"), ((0.1, 1.7e308, 6, n), "range of a double")]
    for args, word in bad:
        t = np.full(max(args[3], 1) + 8, 0xAB, np.uint8)
        rc = L.slam_grid_likelihood_table(*args[:3], t.ctypes.data_as(C.c_void_p), args[3])
        msg = L.slam_last_error().decode()
        assert rc == api.E_INVALID and "slam_grid_likelihood_table" in msg and word in msg, (args, msg)
        assert (t == 0xAB).all()                                               # nothing written
    assert L.slam_grid_likelihood_table(0.1, 0.2, 6, None, n) == api.E_INVALID
    with pytest.raises(api.SlamError) as e:
        api.likelihood_table(0.1, 0.2, 255)
    assert e.value.code == api.E_INVALID
    assert len(api.likelihood_table(0.1, 0.2, 1)) == 3 and len(api.likelihood_table(0.1, 0.2, 254)) == 254 * 254 + 2


# ---------------------------------------------------------------------------------------------- argument errors need no device
CREATES = ("slam_csm_create_from_plane", "slam_csm_create_from_plane_dev")


@pytest.mark.parametrize("fn", CREATES)
def test_every_refusal_of_the_create_calls_needs_no_device(L, fn):
    sentinel = 0x5A5A5A5A
    plane = np.zeros(128, np.uint8)                # never read: every call below is refused before the plane or the device is touched
    for w, h, ox, oy, kw, word in P.BAD_PLANES:
        p = csm_oracle.default_params(**kw)
        out = C.c_void_p(sentinel)
        rc = getattr(L, fn)(plane.ctypes.data_as(C.c_void_p), w, h, ox, oy, C.byref(p), C.byref(out))
        msg = L.slam_last_error().decode()
        assert rc == api.E_INVALID and (fn + ":") in msg and word in msg, (w, h, ox, oy, kw, msg)
        assert not out.value                                                   # the out pointer is cleared, nothing is made
    p = csm_oracle.default_params()
    assert getattr(L, fn)(plane.ctypes.data_as(C.c_void_p), 8, 8, 0, 0, C.byref(p), None) == api.E_INVALID
    assert "null out pointer" in L.slam_last_error().decode()
    out = C.c_void_p(sentinel)
    assert getattr(L, fn)(None, 8, 8, 0, 0, C.byref(p), C.byref(out)) == api.E_INVALID and (fn + ": null plane") in L.slam_last_error().decode()
    # the edge itself is allowed as far as the arguments go: the next question is the device
    # (the host form alone: the device form would be handed a host pointer)
    for ox in ((1 << 30) - 9, -(1 << 30) + 7) if fn == "slam_csm_create_from_plane" else ():
        out = C.c_void_p(sentinel)
        rc = getattr(L, fn)(plane.ctypes.data_as(C.c_void_p), 10, 10, ox, ox, C.byref(p), C.byref(out))
        assert rc in (api.SLAM_OK, api.E_NO_DEVICE), (ox, L.slam_last_error())
        if rc == api.SLAM_OK:
            L.slam_csm_destroy(out)


def test_calls_without_a_handle_are_refused(L):
    one = np.zeros(8)
    i32 = np.zeros(2, np.int32)
    assert L.slam_csm_set_plane_dev(None, one.ctypes.data_as(C.c_void_p), 0, 0, None) == api.E_INVALID
    assert "slam_csm_set_plane_dev" in L.slam_last_error().decode()
    args = (one.ctypes.data_as(C.c_void_p), 1, 0, one.ctypes.data_as(C.c_void_p), 1, i32.ctypes.data_as(C.c_void_p), i32.ctypes.data_as(C.c_void_p))
    assert L.slam_csm_score_poses_dev(None, *args, None) == api.E_INVALID and "slam_csm_score_poses_dev" in L.slam_last_error().decode()
    assert L.slam_csm_score_poses(None, *args) == api.E_INVALID and "slam_csm_score_poses" in L.slam_last_error().decode()


@pytest.mark.skipif(api.device_count() != 0, reason="a GPU is present")
def test_well_formed_create_answers_no_device(L):
    with pytest.raises(api.SlamError) as e:
        api.CorrelativeMatcher.from_plane(np.zeros((4, 4), np.uint8), 0, 0)
    assert e.value.code == api.E_NO_DEVICE


# ------------------------------------------------------------------------------------------------ header, exports, mirror
def test_new_symbols_are_declared_exported_and_bound(L):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slam_mi355x.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", txt))
    for n in NEW:
        assert n in names and n in api.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None, n
    for m in ("from_plane", "set_plane_dev", "score_poses", "score_poses_dev", "poses"):
        assert callable(getattr(api.CorrelativeMatcher, m))
    for m in ("update", "match", "match_post", "match_batch", "score_poses", "relocalize", "close"):
        assert callable(getattr(api.GridMatcher, m))
    assert callable(api.likelihood_table)


# --------------------------------------------------------------------------- the table header alone, under the host sanitizers
def test_likelihood_table_header_alone_under_the_sanitizers(tmp_path):
    src = open(os.path.join(ROOT, "slam_amd", "csrc", "grid_cost_table.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["cmath", "cstdint"]                    # no HIP, no library
    exe = str(tmp_path / "grid_likelihood_table_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "grid_likelihood_table_check.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    rows = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    assert rows["failures"] == ["0"] and "BROKEN" not in r.stdout
    assert rows["R1"][0] == "ok" and rows["R254"][0] == "ok" and rows["n_one_short"][0] == "invalid" and rows["nan_sigma"][0] == "invalid"
    assert rows["tiny_sigma"][0] == "invalid" and rows["huge_both"][0] == "invalid" and rows["sqrt_huge"][:5] == ["ok", "255", "0", "0", "0"]
    assert rows["R6"][:5] == ["ok", "255", "225", "3", "0"]
    # ... and it is the table the library hands out
    t = api.likelihood_table(0.05, 0.5, 254)
    assert rows["R254"][1:] == [str(int(v)) for v in (t[0], t[1], t[254 * 254], t[254 * 254 + 1], t.astype(np.int64).sum())]


# --------------------------------------------------------------- the rehearsals: the accuracy condition, pinned on the restatement
def room_plane(size, res, sigma, R):
    """the likelihood plane of the synthetic room: obstacles are the grid cells of make_map()'s points, everything else unknown"""
    m_ga, m_nga = csm_oracle.synth_map()
    x, y = P.grid_cells(np.concatenate([m_ga, m_nga]), size, size, res)
    occ = np.full(size * size, -1, np.int8)
    occ[x + size * y] = 100
    return P.likelihood_plane(occ, size, size, res, sigma, R)


def rehearse(plane, size, res, k, start, half_xy, half_theta, step):
    t_ga, t_nga, pose = synth.make_scan(k, 256)
    pts = np.concatenate([t_ga, t_nga])
    cs = P.angle_pairs(start[2], half_theta, step)
    vol, cnt = P.volume_slices((-(size // 2), -(size // 2), plane), pts, cs, start[:2], res, half_xy, half_xy)
    _, t, r = P.match(vol, cnt, len(pts), cs, start[:2], res, half_xy, half_xy)
    theta = start[2] + (r["k"] - half_theta) * step
    dth = (theta - pose[2] + np.pi) % (2 * np.pi) - np.pi
    return abs(t[0] - pose[0]), abs(t[1] - pose[1]), abs(dth)


@pytest.fixture(scope="module")
def warm_plane():
    return room_plane(500, 0.1, 0.2, 6)


@pytest.fixture(scope="module")
def cold_plane():
    return room_plane(128, 0.5, 0.5, 3)


@pytest.mark.parametrize("k", csm_oracle.BASIN_KS)
def test_warm_start_lands_within_a_cell_and_a_step(warm_plane, k):
    """500 x 500 at 0.1 m, sigma 0.2 m, R 6; (0.73, -0.58, 0.153) off the truth; +-1 m, +-0.2 rad at 0.01 rad"""
    pose = synth.make_scan(k, 256)[2]
    ex, ey, eth = rehearse(warm_plane, 500, 0.1, k, (pose[0] + 0.73, pose[1] - 0.58, pose[2] + 0.153), 10, 20, 0.01)
    print("warm k=%d: %.3f m %.3f m %.4f rad" % (k, ex, ey, eth))
    assert ex <= 0.1 and ey <= 0.1 and eth <= 0.01


@pytest.mark.parametrize("k", csm_oracle.BASIN_KS)
def test_cold_start_lands_within_a_cell_and_a_step(cold_plane, k):
    """128 x 128 at 0.5 m, sigma 0.5 m, R 3; from (0, 0, 0); +-20 m, 127 angles at 0.05 rad"""
    ex, ey, eth = rehearse(cold_plane, 128, 0.5, k, (0.0, 0.0, 0.0), 40, 63, 0.05)
    print("cold k=%d: %.3f m %.3f m %.4f rad" % (k, ex, ey, eth))
    assert ex <= 0.5 and ey <= 0.5 and eth <= 0.05
