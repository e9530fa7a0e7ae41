"""slam_amd::MapLocalizer::search / relocalize (tests/cpp/map_relocalize_test.cpp) against slam_amd.api.MapLocalizer on the scene of
docs/VOXEL_MAP.md section 11.4, bit for bit: the hits, every (level, hit) that ran and the verdict, on two calls."""
import os
import subprocess

import numpy as np
import pytest

import map_localizer_cases as ML
import vmap_search_cases as SC
from slam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_SECONDS = 120
LEVELS = 2


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "map_relocalize_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_relocalize_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_relocalize_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def hexes(words):
    return [float.fromhex(w) for w in words]


@pytest.mark.gpu
def test_cpp_twin_returns_the_python_twins_bits(tmp_path):
    d = str(tmp_path)
    exe = compile_test(d)
    parts, scan, truth = ML.scene()
    fine = api.VoxelMap(leaf=ML.LEAF)
    fine.enable_distributions()
    for c, T in parts:
        assert fine.integrate(c, T[:3, :3], T[:3, 3]) == 0
    loc = api.MapLocalizer(levels=LEVELS)
    loc.set_map(fine)
    x, y, _ = [np.asarray(v) for v in SC.V.cells_of(loc.level(1).read_sums()[2])]
    cx, cy = np.float32((x.min() + x.max() + 1) * 2.0 / 2), np.float32((y.min() + y.max() + 1) * 2.0 / 2)
    radius = float(max(x.max() - x.min(), y.max() - y.min()) + 2)             # metres: half the box in 2 m cells, and one more cell
    out = loc.relocalize(scan, cx, cy, 0.0, radius)
    assert out["found"] and len(out["hits"]) == 4
    fine.save(os.path.join(d, "map.vmap"))
    np.ascontiguousarray(scan[:, :3], np.float32).tofile(os.path.join(d, "scan.f32"))
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(LEVELS), float(cx).hex(), float(cy).hex(), float(0.0).hex(), radius.hex()], timeout=RUN_SECONDS,
                       capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    rounds = [i for i, ln in enumerate(lines) if ln[0] == "round"]
    assert len(rounds) == 2 and lines[rounds[0] + 1:rounds[1]] == lines[rounds[1] + 1:-1]     # the same bits on two calls
    lines = lines[rounds[0] + 1:rounds[1]]
    hits = [ln for ln in lines if ln[0] == "hit"]
    assert len(hits) == len(out["hits"])
    for ln, h in zip(hits, out["hits"]):
        assert [int(v) for v in ln[2:8]] == [h["score"], h["k"], h["dx"], h["dy"], h["dz"], h["n_with_cell"]]
        assert bits(np.array(hexes(ln[8:24]), np.float32)) == bits(h["init"])
    results = {(int(ln[1]), int(ln[2])): ln for ln in lines if ln[0] == "result"}
    assert set(results) == {(k, i) for k in range(LEVELS) for i in range(len(hits)) if out["last"][k][i] is not None}
    for (k, i), ln in results.items():
        p = out["last"][k][i]
        assert [int(v) for v in ln[3:8]] == [p["iterations"], p["state"], p["converged"], p["pairs"], p["fitness_pairs"]], (k, i)
        assert float.fromhex(ln[8]) == p["fitness"], (k, i)
        assert bits(np.array(hexes(ln[9:25]), np.float32)) == bits(p["transform"]) and bits(np.array(hexes(ln[25:41]))) == bits(p["transform64"]), (k, i)
    v = [ln for ln in lines if ln[0] == "verdict"][0]
    assert [int(w) for w in v[1:4]] == [int(out["found"]), out["index"], out["n_source"]]
    assert hexes(v[4:7]) == [out["x"], out["y"], out["theta"]]
    assert bits(np.array(hexes(v[7:23]), np.float32)) == bits(out["transform"]) and bits(np.array(hexes(v[23:39]))) == bits(out["transform64"])
    loc.close()
    fine.close()
