"""The occupancy grid's row ranges (slam_amd/csrc/grid_rows.hpp) walked through every transition on the host -- no GPU.  The
device is held to the same rules in tests/test_gpu_grid_rows.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_ranges_header_alone(tmp_path):
    src = open(os.path.join(ROOT, "slam_amd", "csrc", "grid_rows.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["cstddef"]                 # no HIP, no library
    exe = str(tmp_path / "grid_rows_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "grid_rows_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-2000:], r.stderr[-2000:])
