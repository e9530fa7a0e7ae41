"""The distance field and costmap of the occupancy grid (docs/GRID_DIST.md) without a GPU: the two numpy restatements agree on
every case of tests/grid_dist_cases.py, the host's inflation table (slam_grid_inflation_table, which needs no device) is the
formula, argument errors answer before any device question, the table header alone survives its extreme arguments under the host
sanitizers, and header, exports and ctypes mirror agree."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_dist_cases as G
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["slam_gdist_default_params", "slam_grid_inflation_table", "slam_gdist_create", "slam_gdist_destroy", "slam_gdist_set_table",
       "slam_gdist_compute_dev", "slam_gdist_compute", "slam_gdist_read", "slam_gdist_planes_dev", "slam_grid_distance_field"]


@pytest.fixture(scope="module")
def L():
    return api.lib()


# ------------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("name", [c["name"] for c in G.cases()])
def test_brute_force_and_two_pass_agree(name):
    c = G.case(name)
    assert np.array_equal(G.expected(name), G.two_pass(c["occ"], c["sx"], c["sy"], c["R"], c["unk"]))


def test_the_case_list_reaches_what_it_names():
    def at(name, x, y):
        return int(G.expected(name)[x + G.case(name)["sx"] * y])
    # d^2 = 25 = R^2 is in, 26 is FAR; the same at R = 1 and R = 254
    assert at("single_R5", 6 + 3, 6 + 4) == 25 and at("single_R5", 6 + 5, 6) == 25 and at("single_R5", 6 - 3, 6 - 4) == 25
    assert at("single_R5", 6 + 1, 6 + 5) == G.FAR and at("single_R5", 6, 6) == 0
    assert at("single_R1", 3, 2) == 1 and at("single_R1", 2, 1) == 1 and at("single_R1", 3, 3) == G.FAR
    assert at("single_R254", 300 + 254, 2) == 254 * 254 and at("single_R254", 300 - 254, 2) == 254 * 254
    assert at("single_R254", 300 + 254, 3) == G.FAR and at("single_R254", 300 + 255, 2) == G.FAR
    # nothing wraps: beyond R cells of the only obstacle column (row) everything is FAR, up to the far edge
    d = G.expected("column_x0").reshape(5, 200)
    assert (d[:, 101:] == G.FAR).all() and (d[:, 100] == 100 * 100).all() and (d[:, 199] == G.FAR).all()
    d = G.expected("row_y0").reshape(200, 5)
    assert (d[101:] == G.FAR).all() and (d[100] == 100 * 100).all()
    assert (G.expected("empty") == G.FAR).all() and (G.expected("empty_unknown") == G.FAR).all()
    assert (G.expected("full") == 0).all() and (G.expected("full_unknown_is_obstacle") == 0).all()
    # across a word boundary from both sides: the cell right of an obstacle at x = 63 and left of one at x = 64
    d = G.expected("130x70_word_edges_R3").reshape(70, 130)
    assert d[15, 64] == 1 and d[15, 66] == 9 and d[15, 67] == G.FAR and d[25, 63] == 1 and d[25, 61] == 9
    assert d[35, 128] == 1 and d[45, 127] == 1 and d[55, 126] == 9 and d[5, 3] == 9
    # the tall planes have an interior tile with both halos inside, and a ragged last tile
    for sy in (700, G.TILE_H + 2 * 254 + 3):
        assert any(t * G.TILE_H - 254 >= 0 and (t + 1) * G.TILE_H + 254 <= sy for t in range(sy // G.TILE_H)) and sy % G.TILE_H
    third = np.mean(G.case("random_97x83_d1_R7_unk0")["occ"] == G.UNKNOWN)
    assert 0.25 < third < 0.4


def test_cost_rule_restated():
    occ = np.array([100, 0, -1, -1, -1, 0], np.int8)
    d2 = np.array([0, 1, 1, 4, G.FAR, G.FAR], np.uint16)
    T = np.array([254, 253, 200, 150, 100, 0], np.uint8)                      # R = 2: six entries, T[5] answers FAR
    assert G.cost_of(d2, occ, T, 2).tolist() == [254, 253, 253, 255, 255, 0]
    assert G.cost_of(d2, occ, T, 2, unknown_keep_from=254).tolist() == [254, 253, 255, 255, 255, 0]
    assert G.cost_of(d2, occ, T, 2, unknown_cost=7, unknown_keep_from=100).tolist() == [254, 253, 253, 100, 7, 0]
    assert G.cost_of(d2, occ, T, 2, unknown_is_obstacle=1).tolist() == [254, 253, 253, 100, 0, 0]


def test_the_scalar_cpp_restatement_agrees(tmp_path):
    """tests/cpp/grid_dist_oracle.cpp, which tools/grid_dist_time.py times beside the device and holds the large planes to"""
    exe = str(tmp_path / "grid_dist_oracle")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "grid_dist_oracle.cpp"), "-o", exe])
    for name in ("1x1_obstacle_unk0", "65x67_R7", "130x70_word_edges_R254", "70x700_R254", "single_R5", "empty", "column_x0", "row_y0",
                 "random_97x83_d1_R32_unk0", "random_97x83_d2_R254_unk1", "random_97x83_d0_R1_unk1"):
        c = G.case(name)
        c["occ"].tofile(str(tmp_path / "occ.i8"))
        subprocess.check_call([exe, str(tmp_path / "occ.i8"), str(c["sx"]), str(c["sy"]), str(c["R"]), str(c["unk"]), str(tmp_path / "d.u16")],
                              stdout=subprocess.DEVNULL)
        assert np.array_equal(np.fromfile(str(tmp_path / "d.u16"), np.uint16), G.expected(name)), name


# ------------------------------------------------------------------------------------------------------ the inflation table
@pytest.mark.parametrize("R,res,inscribed,inflation,scaling", [
    (32, 0.05, 0.3, 1.2, 3.0), (32, 0.05, 0.725, 1.6, 10.0), (1, 0.2, 0.1, 0.2, 3.0), (254, 0.05, 0.725, 12.7, 0.5),
    (254, 0.01, 0.0, 2.54, 3.0), (100, 0.1, 2.0, 2.0, 3.0), (64, 0.05, 0.0, 0.0, 0.0), (7, 0.05, 0.05, 0.35, 0.0)])
def test_inflation_table_is_the_formula(L, R, res, inscribed, inflation, scaling):
    t = api.inflation_table(res, inscribed, inflation, scaling, R)
    assert t.dtype == np.uint8 and len(t) == R * R + 2
    want, real, exact = G.inflation_table_np(res, inscribed, inflation, scaling, R)
    k = np.arange(R * R + 2)
    d = np.sqrt(k.astype(np.float64)) * res
    assert t[0] == 254 and t[R * R + 1] == 0
    inner = (k >= 1) & (k <= R * R)
    assert (t[inner & (d <= inscribed)] == 253).all()
    assert (t[inner & (d > inflation)] == 0).all()
    assert (np.diff(t.astype(int)) <= 0).all()                                # non-increasing in k
    assert np.array_equal(t[exact], want[exact])
    clear = ~exact & (np.abs(real - np.round(real)) > 1e-9)                   # libm and numpy may differ in the last ulp: only there
    assert np.array_equal(t[clear], want[clear])
    assert (np.abs(t[~exact].astype(int) - want[~exact].astype(int)) <= 1).all()
    assert (t[~exact] <= 252).all()


def test_inflation_table_refusals(L):
    n = 32 * 32 + 2
    bad = [((0.05, 0.3, 1.2, 3.0, 32, n - 1), "entries"), ((0.05, 0.3, 1.2, 3.0, 32, n + 1), "entries"),
           ((float("nan"), 0.3, 1.2, 3.0, 32, n), "non-finite"), ((0.05, float("inf"), 1.2, 3.0, 32, n), "non-finite"),
           ((0.05, 0.3, float("inf"), 3.0, 32, n), "non-finite"), ((0.05, 0.3, 1.2, float("nan"), 32, n), "non-finite"),
           ((-0.05, 0.3, 1.2, 3.0, 32, n), "resolution"), ((0.05, -0.3, 1.2, 3.0, 32, n), "negative"),
           ((0.05, 0.3, -1.2, 3.0, 32, n), "negative"), ((0.05, 0.3, 1.2, -3.0, 32, n), "negative"),
           ((0.05, 1.3, 1.2, 3.0, 32, n), "inscribed_radius exceeds"), ((0.05, 0.3, 1.61, 3.0, 32, n), "cut the inflation short"),
           ((0.05, 0.3, 1.2, 3.0, 0, 2), "max_cells"), ((0.05, 0.3, 1.2, 3.0, 255, 255 * 255 + 2), "max_cells")]
    for args, word in bad:
        t = np.full(max(args[5], 1) + 8, 0xAB, np.uint8)
        rc = L.slam_grid_inflation_table(*args[:5], t.ctypes.data_as(C.c_void_p), args[5])
        msg = L.slam_last_error().decode()
        assert rc == api.E_INVALID and "slam_grid_inflation_table" in msg and word in msg, (args, msg)
        assert (t == 0xAB).all()                                               # nothing written
    assert L.slam_grid_inflation_table(0.05, 0.3, 1.2, 3.0, 32, None, n) == api.E_INVALID
    with pytest.raises(api.SlamError) as e:
        api.inflation_table(0.05, 0.3, 1.61, 3.0, 32)
    assert e.value.code == api.E_INVALID
    assert api.inflation_table(0.05, 0.3, 1.6, 3.0, 32)[32 * 32] == int(252.0 * np.exp(-3.0 * (1.6 - 0.3)))   # the cap itself is allowed


# ---------------------------------------------------------------------------------------------- argument errors need no device
def test_argument_errors_do_not_need_a_device(L):
    sentinel = 0x5A5A5A5A
    for sx, sy, R in ((10, 10, 0), (10, 10, 255), (0, 10, 32), (10, 0, 32), (-1, 10, 32), (40000, 10, 32)):
        h = C.c_void_p(sentinel)
        p = api.gdist_default_params(max_cells=R)
        assert L.slam_gdist_create(sx, sy, C.byref(p), C.byref(h)) == api.E_INVALID, (sx, sy, R)
        assert b"slam_gdist_create" in L.slam_last_error() and h.value == sentinel
    for kw in (dict(unknown_cost=256), dict(unknown_keep_from=-1)):
        h = C.c_void_p(sentinel)
        p = api.gdist_default_params(**kw)
        assert L.slam_gdist_create(10, 10, C.byref(p), C.byref(h)) == api.E_INVALID and h.value == sentinel
    p = api.gdist_default_params()
    assert L.slam_gdist_create(10, 10, C.byref(p), None) == api.E_INVALID and b"null out pointer" in L.slam_last_error()
    # without a handle every call is refused, whatever else it is given (a wrong table length on a live handle: the GPU suite)
    t = np.zeros(7, np.uint8)
    assert L.slam_gdist_set_table(None, t.ctypes.data_as(C.c_void_p), 7) == api.E_INVALID and b"slam_gdist_set_table" in L.slam_last_error()
    assert L.slam_gdist_compute_dev(None, None, None) == api.E_INVALID
    assert L.slam_gdist_compute(None, None) == api.E_INVALID
    assert L.slam_gdist_read(None, None, None) == api.E_INVALID
    assert L.slam_gdist_planes_dev(None, None, None) == api.E_INVALID
    assert L.slam_grid_distance_field(None, None, None) == api.E_INVALID and b"slam_grid_distance_field" in L.slam_last_error()
    L.slam_gdist_destroy(None)


@pytest.mark.skipif(api.device_count() != 0, reason="a GPU is present")
def test_well_formed_create_answers_no_device(L):
    h = C.c_void_p(7)
    assert L.slam_gdist_create(10, 10, None, C.byref(h)) == api.E_NO_DEVICE and not h.value
    with pytest.raises(api.SlamError) as e:
        api.DistanceField(10, 10)
    assert e.value.code == api.E_NO_DEVICE


# ------------------------------------------------------------------------------------------------ header, exports, mirror
def header_text():
    txt = open(os.path.join(ROOT, "include", "slam_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_new_symbols_are_declared_exported_and_bound(L):
    names = set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", header_text()))
    for n in NEW:
        assert n in names and n in api.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None, n
    assert re.search(r"#define\s+SLAM_GDIST_FAR\s+0xFFFFu", header_text()) and api.GDIST_FAR == G.FAR == 0xFFFF
    for name in ("DistanceField", "GdistParams", "gdist_default_params", "inflation_table"):
        assert hasattr(api, name)
    for m in ("set_table", "set_inflation", "compute", "compute_dev", "read", "planes_dev", "close"):
        assert callable(getattr(api.DistanceField, m))
    assert callable(api.Grid.distance_field)


def test_defaults(L):
    p = api.gdist_default_params()
    assert (p.max_cells, p.unknown_is_obstacle, p.unknown_cost, p.unknown_keep_from) == (32, 0, 255, 253)
    assert api.gdist_default_params(max_cells=7).max_cells == 7


def test_gdist_params_mirror_the_header(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "slam_mi355x.h"', "int main(void) {",
             'printf("%zu", sizeof(slam_gdist_params));']
    for f, _ in api.GdistParams._fields_:
        lines.append('printf(" %s=%%zu", offsetof(slam_gdist_params, %s));' % (f, f))
    lines += ['printf("\\n");', "return 0;", "}"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    parts = subprocess.check_output([str(exe)], text=True).split()
    assert int(parts[0]) == C.sizeof(api.GdistParams)
    assert len(parts) - 1 == len(api.GdistParams._fields_) == 4
    for p in parts[1:]:
        f, off = p.split("=")
        assert getattr(api.GdistParams, f).offset == int(off), (f, off)


# --------------------------------------------------------------------------- the table header alone, under the host sanitizers
def test_cost_table_header_alone_under_the_sanitizers(tmp_path):
    src = open(os.path.join(ROOT, "slam_amd", "csrc", "grid_cost_table.hpp")).read()
    assert [i for i in re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)] == ["cmath", "cstdint"]      # no HIP, no library
    exe = str(tmp_path / "grid_cost_table_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "grid_cost_table_check.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    rows = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    assert rows["failures"] == ["0"] and "BROKEN" not in r.stdout
    assert rows["R1"][0] == "ok" and rows["R254"][0] == "ok" and rows["n_one_short"][0] == "invalid" and rows["nan_scaling"][0] == "invalid"
    # ... and it is the table the library hands out
    t = api.inflation_table(0.05, 0.3, 12.7, 3.0, 254)
    assert rows["R254"][1:] == [str(int(v)) for v in (t[0], t[1], t[254 * 254], t[254 * 254 + 1], t.astype(np.int64).sum())]
