"""A buffer that grows in the middle of a sequence changes nothing an adapter reports: tests/cpp/adapter_growth_test.cpp
runs slam_amd::MLS, MLSMap, CCICP and GlobalMapBuilder over a small cloud and then one eight times as large, once with an
object whose blocks grow between the two and once with an object that was sized beforehand by a still larger cloud and
emptied again.  What the two objects report must be equal byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from slam_amd import build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTERS = ("mls", "mls_map", "ccicp", "builder")


def compile_growth_test(tmp):
    build.build()
    exe = os.path.join(tmp, "adapter_growth_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "adapter_growth_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_growth_between_two_clouds_changes_nothing(tmp_path):
    exe = compile_growth_test(str(tmp_path))
    d = str(tmp_path)
    # one pose of the loop at four samplings: about 500, 4 000 and 16 000 points, and the 4 000 of another seed the
    # matcher's target and the builder's map start from
    shapes = {"small": (16, 32, 9000), "big": (16, 256, 9000), "huge": (32, 512, 9000), "base": (16, 256, 9100)}
    sizes = {}
    for name, (rings, n_az, seed) in shapes.items():
        xyz, _ = synth.make_cloud3d(3, n_loop=50, rings=rings, n_az=n_az, seed_base=seed)
        xyz.tofile(os.path.join(d, name + ".f32"))
        sizes[name] = len(xyz)
    print(sizes)
    assert sizes["big"] > 1.5 * sizes["small"] and sizes["huge"] > sizes["big"] + sizes["small"]   # every block grows in A, none in B
    out = os.path.join(d, "out")
    print(subprocess.check_output([exe, d, out]).decode())
    for name in ADAPTERS:
        a, b = (open("%s.%s.%s" % (out, name, ab), "rb").read() for ab in "AB")
        assert len(a) > 0 and a == b, "%s: %d bytes against %d, first difference at %s" % (
            name, len(a), len(b), next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None))
