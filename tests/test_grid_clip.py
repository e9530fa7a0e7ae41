"""The tiled raycast's clip of one beam to one tile (slam_amd/csrc/grid_clip.hpp) beside the plain Bresenham walk, on the host --
no GPU: every beam of a 24 x 24 window against 5 x 5-cell tiles, and the longest beams a 32767-cell grid admits against its
128-cell tiles, with the reciprocals one float off either way (tests/cpp/grid_clip_check.cpp says what is required).  The device
runs the same function: tests/test_gpu_grid_raycast_edges.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_header_alone(tmp_path):
    src = open(os.path.join(ROOT, "slam_amd", "csrc", "grid_clip.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == []                          # no HIP, no library
    exe = str(tmp_path / "grid_clip_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "grid_clip_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)                # (one thread)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", (r.stdout[-2000:], r.stderr[-2000:])
