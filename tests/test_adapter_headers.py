"""The public headers under include/slam_amd/: each one compiles in a translation unit of its own and all of them in one,
with warnings as errors and no library; Pose has one definition and no macro guards a second one."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "slam_amd", "*.hpp")))


def syntax_only(tmp_path, names):
    tu = tmp_path / "tu.cpp"
    tu.write_text("".join('#include "slam_amd/%s"\n' % n for n in names) + "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(tu)])


def test_the_eleven_headers_are_there():
    assert HEADERS == ["buffer.hpp", "ccicp.hpp", "correlative.hpp", "global_match.hpp", "graph_edges.hpp", "icp.hpp",
                       "map_builder.hpp", "mls.hpp", "mls_map.hpp", "pose.hpp", "pose_graph.hpp"]


@pytest.mark.parametrize("name", HEADERS)
def test_header_stands_alone(tmp_path, name):
    syntax_only(tmp_path, [name])


def test_headers_stand_together(tmp_path):
    syntax_only(tmp_path, HEADERS)
    syntax_only(tmp_path, HEADERS[::-1])


def test_pose_is_defined_once_and_unguarded():
    text = {n: open(os.path.join(INCLUDE, "slam_amd", n)).read() for n in HEADERS}
    assert [n for n, t in text.items() if "SLAM_AMD_POSE_DEFINED" in t] == []
    assert [n for n, t in text.items() if re.search(r"\bstruct\s+Pose\s*\{", t)] == ["pose.hpp"]


def test_pose_header_is_pure_math():
    """pose.hpp includes neither the C-ABI nor HIP; buffer.hpp sits over the C-ABI and not over HIP."""
    pose = open(os.path.join(INCLUDE, "slam_amd", "pose.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', pose) == ["cmath"]
    buf = open(os.path.join(INCLUDE, "slam_amd", "buffer.hpp")).read()
    assert not [i for i in re.findall(r'#include\s+[<"]([^>"]+)[>"]', buf) if "hip" in i]


def test_only_buffer_hpp_allocates():
    """slam_malloc / slam_free / slam_host_alloc / slam_host_free are called from buffer.hpp and nowhere else in the adapters
    (comments may name slam_host_alloc as the caller's way to get pinned memory)."""
    call = re.compile(r"\bslam_(malloc|free|host_alloc|host_free)\s*\(")
    hits = []
    for n in HEADERS:
        for line in open(os.path.join(INCLUDE, "slam_amd", n)):
            if call.search(line.split("//")[0]):
                hits.append(n)
    assert set(hits) == {"buffer.hpp"}
