"""slam_amd::MLSMap (include/slam_amd/mls_map.hpp) run the way graph_slam runs its global map: tests/cpp/mls_map_test.cpp
(the first keyframe with setMinClusterPoints(5) / (10), regenerateGlobalMap, getSegmentedClouds into CCICP(SCAN_TO_MAP),
offsetMap), compiled with g++ against the library.  The map's outputs against the restatement
(tests/cpp/mls_map_oracle.cpp), the pose against CCICP on the restatement's clouds and against the oracle chain."""
import os
import subprocess

import numpy as np
import pytest

import mls_map_oracle as MO
import oracle_lib as O
from ccicp_chain import oracle_scan_match, quat_rpy
from slam_amd import api, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYFRAMES = [0, 2, 4, 6]
SCENE = 5


def compile_test(tmp):
    build.build()
    exe = os.path.join(tmp, "mls_map_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mls_map_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_mls_map_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter headers are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def quat_matrix(q):
    """tf::poseMsgToEigen's rotation as slam_amd::MLSMap computes it (the same operations in the same order)"""
    qx, qy, qz, qw = q
    d = qx * qx + qy * qy + qz * qz + qw * qw
    s2 = 2.0 / d if d > 0 else 0.0
    xs, ys, zs = qx * s2, qy * s2, qz * s2
    wx, wy, wz = qw * xs, qw * ys, qw * zs
    xx, xy, xz, yy, yz, zz = qx * xs, qx * ys, qx * zs, qy * ys, qy * zs, qz * zs
    return np.array([[1.0 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1.0 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1.0 - (xx + yy)]])


def f32(path, cols=3):
    return np.fromfile(path, np.float32).reshape(-1, cols)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_regenerate_global_map_into_ccicp(tmp_path):
    exe = compile_test(str(tmp_path))
    d = str(tmp_path)
    poses, world = [], []
    for i, k in enumerate(KEYFRAMES):
        xyz, (x, y, th) = synth.make_cloud3d(k, n_loop=50)
        pose = [x, y, 0.0] + quat_rpy(0.0, 0.0, th)
        poses.append(pose)
        np.ascontiguousarray(np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], 1)).tofile(os.path.join(d, "kf%d.f32" % i))
        world.append(MO.transform(xyz, quat_matrix(pose[3:]), np.array(pose[:3])))   # graph_slam.cpp:271-275
    np.array(poses).tofile(os.path.join(d, "poses.f64"))

    # the restatement: the same calls
    ora = MO.OracleMls(1000, 1000, 0.5, api.mls_default_params())
    ora.set_params(min_cluster_points=5)
    ora.add_cloud(world[0], poses[0][:2])
    ora.set_params(min_cluster_points=10)
    first = ora.segmented_clouds()
    ora.clear()
    for w, p in zip(world, poses):
        ora.add_cloud(w, p[:2])
    obs, gnd = ora.segmented_clouds()
    drv = ora.read_drivability()
    obs.tofile(os.path.join(d, "oracle_obstacle.f32"))
    gnd.tofile(os.path.join(d, "oracle_ground.f32"))

    scene, (sx, sy, sth) = synth.make_cloud3d(SCENE, n_loop=50)
    init = [sx + 0.15, sy - 0.1, 0.0] + quat_rpy(0.0, 0.0, sth + 0.03)
    scene.tofile(os.path.join(d, "scene.f32"))
    np.array(init).tofile(os.path.join(d, "init.f64"))
    out = os.path.join(d, "out")
    subprocess.check_call([exe, d, out, str(len(KEYFRAMES))])   # exit 5: CCICP on the map's clouds != on the restatement's

    assert same(f32(out + ".first_obstacle"), first[0]) and same(f32(out + ".first_ground"), first[1])
    assert same(f32(out + ".obstacle"), obs) and same(f32(out + ".ground"), gnd)
    assert len(obs) > 300 and len(gnd) > 1000
    assert np.array_equal(np.fromfile(out + ".drivability", np.int8), drv)

    # filterPointCloud(0.1, 0.1) on the device, the host fallback's filter on the same cloud, and the oracle's pcl::VoxelGrid
    gc, gc_host = f32(out + ".global"), f32(out + ".global_host")
    allw = np.concatenate(world)
    vox, n_vox = O.voxel_downsample(np.concatenate([allw, np.zeros((len(allw), 1), np.float32)], 1), (0.1, 0.1, 0.1))
    assert 0 < len(gc) < len(allw) and len(gc) == len(gc_host) == n_vox
    assert np.abs(gc - gc_host).max() < 1e-4 and np.abs(gc - vox[:, :3]).max() < 1e-4

    # the pose: CCICP on the map's clouds equals CCICP on the restatement's (the program checked it bit for bit);
    # against the oracle chain with the tolerances of the CCICP facade test
    got = np.fromfile(out + ".pose", np.float64)
    e = oracle_scan_match(obs, gnd, scene, init)
    assert abs(got[0] - e["t"][0]) < 1e-4 and abs(got[1] - e["t"][1]) < 1e-4
    assert np.abs(got[3:7] - e["q"]).max() < 1e-5
    assert abs(got[7] - e["n_corr"]) <= 2
    # the height (icpTools.cpp:301-381) takes each wheel point's nearest ground point; here the ground target is a 0.5 m
    # lattice of cluster means, where those nearest points are near-ties between the chain's pose and the device's
    # (1.7 mm apart on this scene); z itself is held bit for bit by the program's comparison above
    z, _, _ = O.ccicp_height(gnd, [got[0], got[1], init[2]] + list(got[3:7]))
    assert abs(got[2] - z) < 1e-2
    assert abs(got[0] - sx) < 0.5 and abs(got[1] - sy) < 0.5 and abs(e["yaw"] - sth) < 0.05

    # offsetMap(z = 0.25): the clusters' mean z on the device, the global cloud's z + (float)0.25
    ora.offset_z(0.25)
    assert same(f32(out + ".offset_obstacle"), ora.segmented_clouds()[0])
    gc_off = f32(out + ".offset_global")
    want = gc.copy()
    want[:, 2] = want[:, 2] + np.float32(0.25)
    assert same(gc_off, want)
