"""The scalar restatement of graph_slam's keyframe edge (tests/cpp/kf_edge_oracle.cpp) against hand-worked cases, one per
branch, its gated search against brute force, its LUM sums against a straight numpy evaluation, and the new C structs
against their ctypes mirrors.  No GPU needed.  The rules are those of docs/KF_EDGE.md section 2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kf_edge_oracle as K
import oracle_lib as O
from kf_edge_cases import AXES, SOLVE_TOL, T_of, lattice_cloud, rot90   # shared with the branch tests
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("axis,turns", [(0, 1), (1, 1), (2, 1), (0, 2), (1, 3), (2, 2)])
def test_exact_rigid_copy_is_recovered_in_one_step(axis, turns):
    R, t = rot90(axis, turns), np.array([0.5, -1.25, 2.0])
    src = lattice_cloud()
    tgt = (src.astype(np.float64) @ R.T + t).astype(np.float32)
    assert np.array_equal(tgt.astype(np.float64), src.astype(np.float64) @ R.T + t)      # an exact copy
    Rs, ts, rank = K.solve(src, tgt)
    assert rank == 3 and np.abs(Rs - R).max() < SOLVE_TOL and np.abs(ts - t).max() < SOLVE_TOL
    # through the ICP: started a quarter of a metre off, every pair inside the gate and the right one
    init = T_of(R, t + np.array([0.25, -0.125, 0.25])).astype(np.float32)
    kf = K.OracleKeyframe(tgt)
    one = K.register_edge(kf, src, init, params=K.default_params(max_iterations=1))
    assert (one["iterations"], one["state"], one["pairs"]) == (1, api.KF_ITERATIONS, len(src))
    assert np.abs(one["transform64"] - T_of(R, t)).max() < SOLVE_TOL
    assert abs(one["mse"] - (0.25 ** 2 + 0.125 ** 2 + 0.25 ** 2)) < SOLVE_TOL
    # ... and the second step is the identity: TRANSFORM
    two = K.register_edge(kf, src, init)
    assert (two["iterations"], two["state"], two["converged"]) == (2, api.KF_TRANSFORM, 1)
    assert np.abs(two["transform64"] - T_of(R, t)).max() < SOLVE_TOL and two["mse"] < 1e-24
    # LUM on an exact match: ss = 0, the identity fallback (:203-208)
    assert two["num_corr"] == len(src) and two["singular"] == 1 and np.array_equal(two["information"], np.eye(6))


def test_reflected_pairs_take_the_determinant_fix():
    """H = diag(16, 4, -1) / 3 and diag(-16, 4, 1) / 3: det H < 0, the smallest singular value's sign flips"""
    for mirror, want in ((np.diag([1.0, 1, -1]), np.eye(3)), (np.diag([-1.0, 1, 1]), np.diag([-1.0, 1, -1]))):
        q = (AXES @ mirror).astype(np.float32)
        for use_float in (False, True):
            R, t, rank = K.solve(AXES, q, use_float)
            assert rank == 3 and abs(np.linalg.det(R) - 1) < 1e-6
            assert np.abs(R - want).max() < (1e-6 if use_float else SOLVE_TOL) and np.abs(t).max() < 1e-6


def test_planar_pairs_take_the_rank_two_branch():
    g = np.stack(np.meshgrid(np.arange(4.0), np.arange(3.0) * 2), -1).reshape(-1, 2)
    p = np.column_stack([g, np.zeros(len(g))]).astype(np.float32)
    Rz = rot90(2, 1)
    R, t, rank = K.solve(p, (p @ Rz.T + [1, 2, 3]).astype(np.float32))
    assert rank == 2 and np.abs(R - Rz).max() < SOLVE_TOL and np.abs(t - [1, 2, 3]).max() < SOLVE_TOL
    # a mirrored planar set: the proper rotation that does it turns the plane over (180 degrees about x)
    R, t, rank = K.solve(p, (p * [1, -1, 1]).astype(np.float32))
    assert rank == 2 and np.abs(R - np.diag([1.0, -1, -1])).max() < SOLVE_TOL and abs(np.linalg.det(R) - 1) < SOLVE_TOL
    # collinear and coincident pairs: still a proper rotation
    line = np.column_stack([np.arange(5.0), np.zeros(5), np.zeros(5)]).astype(np.float32)
    for q in (line + np.float32(1), np.zeros_like(line)):
        R, t, rank = K.solve(line, q)
        assert rank <= 1 and np.abs(R @ R.T - np.eye(3)).max() < SOLVE_TOL and abs(np.linalg.det(R) - 1) < SOLVE_TOL


def test_two_pairs_are_no_correspondences():
    tgt = np.array([[0, 0, 0], [5, 0, 0], [50, 50, 50]], np.float32)
    src = np.array([[0.1, 0, 0], [5.1, 0, 0], [20, 20, 20]], np.float32)
    r = K.register_edge(K.OracleKeyframe(tgt), src, np.eye(4))
    assert (r["state"], r["converged"], r["iterations"], r["pairs"]) == (api.KF_NO_CORRESPONDENCES, 0, 0, 2)
    assert np.array_equal(r["transform64"], np.eye(4)) and r["pairs_trace"][0] == 2 and r["pairs_trace"][1] == -1


def test_a_pair_at_the_gate_is_kept_by_icp_and_dropped_by_lum():
    tgt = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10]], np.float32)
    src = tgt + np.float32([0.75, 0, 0])          # 0.75 and 0.5625 are exact in f32 and f64
    kf = K.OracleKeyframe(tgt)
    i_icp, d_icp = kf.nearest(src, strict=False)
    i_lum, _ = kf.nearest(src, strict=True)
    assert i_icp.tolist() == [0, 1, 2, 3] and (d_icp == np.float32(0.5625)).all() and (i_lum == -1).all()
    r = K.register_edge(kf, src, np.eye(4), params=K.default_params(max_iterations=1))
    assert r["pairs"] == 4 and r["mse"] == 0.5625
    assert np.abs(r["transform64"] - T_of(np.eye(3), [-0.75, 0, 0])).max() < SOLVE_TOL
    assert K.lum_only(kf, src, np.eye(4))["num_corr"] == 0
    # one ulp inside the gate LUM takes it too: three of the four (10 + 0.74999994 rounds to 10.75 in f32, at the gate again)
    inside = tgt + np.float32([np.nextafter(np.float32(0.75), np.float32(0)), 0, 0])
    assert inside[1, 0] == np.float32(10.75) and K.lum_only(kf, inside, np.eye(4))["num_corr"] == 3


def filtered_keyframes():
    out = []
    for k in K.EDGE_KS:
        xyz, pose = K.cloud(k)
        f = O.voxel_downsample(np.hstack([xyz, np.zeros((len(xyz), 1), np.float32)]), leaf=(0.5, 0.5, 0.5))[0]
        out.append((np.ascontiguousarray(f[:, :3]), pose))
    return out


@pytest.fixture(scope="module")
def keyframes():
    return filtered_keyframes()


def test_every_stop_state_is_reached(keyframes):
    src = lattice_cloud()
    tgt = src + np.float32([0.25, 0, 0])
    kf = K.OracleKeyframe(tgt)
    # ITERATIONS: the cap comes first
    assert K.register_edge(kf, src, np.eye(4), params=K.default_params(max_iterations=1))["state"] == api.KF_ITERATIONS
    # TRANSFORM: the second step of an exact copy is the identity
    r = K.register_edge(kf, src, np.eye(4))
    assert (r["state"], r["iterations"]) == (api.KF_TRANSFORM, 2)
    # ABS_MSE: with the transform test off, mse goes 0.0625, 0, 0: the third difference is below 1e-12
    r = K.register_edge(kf, src, np.eye(4), params=K.default_params(transformation_epsilon=-1.0))
    assert (r["state"], r["iterations"], r["converged"]) == (api.KF_ABS_MSE, 3, 1)
    # REL_MSE: a noisy edge whose mse moves by a few per cent per iteration, against a fitness epsilon of 0.5
    (f0, p0), (f1, p1) = keyframes[0], keyframes[1]
    r = K.register_edge(K.OracleKeyframe(f0), f1, K.relative_init(p0, p1),
                        params=K.default_params(transformation_epsilon=-1.0, fitness_epsilon=0.5))
    assert (r["state"], r["iterations"], r["converged"]) == (api.KF_REL_MSE, 2, 1)
    # NO_CORRESPONDENCES: nothing within the gate
    r = K.register_edge(kf, src + np.float32(100), np.eye(4))
    assert (r["state"], r["converged"], r["pairs"]) == (api.KF_NO_CORRESPONDENCES, 0, 0)


def test_gated_search_equals_brute_force(keyframes):
    """on the make_cloud3d keyframes: the queries ICP actually makes (the source under the initial transform) and random ones"""
    rs = np.random.RandomState(2)
    f0, p0 = keyframes[0]
    kf = K.OracleKeyframe(f0)
    cells, max_cell = kf.stats()
    assert 2000 <= cells <= 2600 and max_cell <= 8 and 4300 <= len(f0) <= 5900
    kept = 0
    for f, p in keyframes[1:]:
        T = K.relative_init(p0, p).astype(np.float64)
        q = np.concatenate([(f.astype(np.float64) @ T[:3, :3].T + T[:3, 3]), f0 + rs.normal(0, 0.4, f0.shape)]).astype(np.float32)
        for strict in (False, True):
            oi, od = kf.nearest(q, strict=strict)
            bi, bd = K.brute_force(f0, q, 0.75, strict)
            assert np.array_equal(oi, bi) and np.array_equal(od.view(np.uint32), bd.view(np.uint32))
        kept += int((bi >= 0).sum())
    assert kept > 20000


def test_lum_sums_against_numpy(keyframes):
    """MM and MZ of :153-176 from the restatement's own pairs, the f32 products summed by numpy in f64: equal to the
    reassociation bound n 2^-53 sum|term| per entry; the 6 x 6 inverse against numpy's; ss against its f64 value."""
    (f0, p0), (f1, p1) = keyframes[0], keyframes[2]
    kf = K.OracleKeyframe(f0)
    r = K.register_edge(kf, f1, K.relative_init(p0, p1), lum_detail=True)
    a, d, n = r["aver"], r["diff"], r["num_corr"]
    assert n > 4000 and a.dtype == np.float32 and len(a) == n

    def s64(x):
        assert x.dtype == np.float32
        return x.astype(np.float64).sum(), np.abs(x.astype(np.float64)).sum()
    want = {(0, 4): s64(-a[:, 1]), (0, 5): s64(a[:, 2]), (1, 3): s64(-a[:, 2]), (1, 4): s64(a[:, 0]), (2, 3): s64(a[:, 1]),
            (2, 5): s64(-a[:, 0]), (3, 4): s64(-(a[:, 0] * a[:, 2])), (3, 5): s64(-(a[:, 0] * a[:, 1])), (4, 5): s64(-(a[:, 1] * a[:, 2])),
            (3, 3): s64(a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]), (4, 4): s64(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]),
            (5, 5): s64(a[:, 0] * a[:, 0] + a[:, 2] * a[:, 2])}
    for (i, j), (v, mag) in want.items():
        bound = n * 2.0 ** -53 * mag
        assert abs(r["MM"][i, j] - v) <= bound and r["MM"][j, i] == r["MM"][i, j], (i, j, r["MM"][i, j] - v, bound)
    assert r["MM"][0, 0] == r["MM"][1, 1] == r["MM"][2, 2] == float(n)
    mz = [s64(d[:, 0]), s64(d[:, 1]), s64(d[:, 2]), s64(a[:, 1] * d[:, 2] - a[:, 2] * d[:, 1]),
          s64(a[:, 0] * d[:, 1] - a[:, 1] * d[:, 0]), s64(a[:, 2] * d[:, 0] - a[:, 0] * d[:, 2])]
    for i, (v, mag) in enumerate(mz):
        assert abs(r["MZ"][i] - v) <= n * 2.0 ** -53 * mag, i
    inv = K.inverse6(r["MM"])
    assert np.abs(inv @ r["MM"] - np.eye(6)).max() < 1e-9
    D = inv @ r["MZ"]
    a64, d64 = a.astype(np.float64), d.astype(np.float64)
    e = np.stack([d64[:, 0] - (D[0] + a64[:, 2] * D[5] - a64[:, 1] * D[4]), d64[:, 1] - (D[1] + a64[:, 0] * D[4] - a64[:, 2] * D[3]),
                  d64[:, 2] - (D[2] + a64[:, 1] * D[3] - a64[:, 0] * D[5])], 1)
    ss = (e * e).sum()
    assert abs(float(r["ss"]) - ss) <= n * 2.0 ** -24 * ss and r["singular"] == 0
    assert np.array_equal(r["information"], r["MM"] * float(np.float32(1.0) / r["ss"]))
    # a singular MM (no pair at all): non-finite entries or zeros end in the identity fallback
    far = K.lum_only(kf, f1 + np.float32(1000), np.eye(4))
    assert far["num_corr"] == 0 and far["singular"] == 1 and np.array_equal(far["information"], np.eye(6))


def test_float_mode_stays_close_to_the_contract(keyframes):
    """mode 1 follows PCL's float order of operations; docs/KF_EDGE.md records the difference printed here"""
    f0, p0 = keyframes[0]
    kf = K.OracleKeyframe(f0)
    for (f, p), k in zip(keyframes[1:], K.EDGE_KS[1:]):
        init = K.relative_init(p0, p)
        a, b = K.register_edge(kf, f, init, mode=0), K.register_edge(kf, f, init, mode=1)
        dpos, dang = K.pose_error(a["transform64"], b["transform64"])
        tpos, tang = K.pose_error(a["transform64"], K.true_relative(p0, p))
        print("edge 0-%d: double %d iterations (state %d, margin %.3g), float %d (state %d); float - double %.3g m %.3g rad; "
              "double - truth %.3g m %.3g rad" % (k, a["iterations"], a["state"], a["margin"], b["iterations"], b["state"], dpos, dang, tpos, tang))
        assert a["state"] == api.KF_TRANSFORM and a["margin"] > 1e-3 and tpos < 0.05 and tang < 0.01
        assert b["converged"] == 1 and dpos < 0.05 and dang < 0.01     # no further from it than the ICP is from the truth


def test_new_structs_mirror_the_header(tmp_path):
    structs = {"slam_kf_params": api.KfParams, "slam_kf_edge_req": api.KfEdgeReq, "slam_kf_edge_result": api.KfEdgeResult}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "slam_mi355x.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (f, name, f.rstrip("_")))
        lines.append('printf("\\n");')
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    seen = 0
    for line in out.strip().splitlines():
        parts = line.split()
        cls = structs[parts[0]]
        assert int(parts[1]) == C.sizeof(cls), (parts[0], parts[1], C.sizeof(cls))
        for p in parts[2:]:
            f, off = p.split("=")
            assert getattr(cls, f).offset == int(off), (parts[0], f, off)
            seen += 1
    assert seen == sum(len(c._fields_) for c in structs.values())
    assert (api.KF_ITERATIONS, api.KF_TRANSFORM, api.KF_ABS_MSE, api.KF_REL_MSE, api.KF_NO_CORRESPONDENCES) == (1, 2, 3, 4, 5)


def test_store_refuses_without_a_device_or_bad_parameters():
    L = api.lib()
    h = C.c_void_p()
    bad = api.KfParams(0.5, 0.75, 0.5, 200, 1e-6, 1e-6, 1)      # a lattice finer than the gate would miss neighbours
    assert L.slam_kf_create(C.byref(bad), C.byref(h)) == api.E_INVALID and b"cell_size" in L.slam_last_error()
    assert L.slam_kf_create(None, None) == api.E_INVALID
    p = api.kf_default_params()
    assert (p.leaf_size, p.gate, p.cell_size, p.max_iterations, p.transformation_epsilon, p.fitness_epsilon, p.target_in_lds) == \
        (0.5, 0.75, 0.0, 200, 1e-6, 1e-6, 1)                   # graphSlamTools.cpp:27-39, 281
    if api.device_count() == 0:
        with pytest.raises(api.SlamError) as e:
            api.KeyframeStore()
        assert e.value.code == api.E_NO_DEVICE


def test_small_cpp_program_compiles_against_the_library(tmp_path):
    """the adapter header in a translation unit of its own, linked against the shipped library"""
    src = tmp_path / "use.cpp"
    src.write_text('#include "slam_amd/graph_edges.hpp"\n#include "slam_amd/mls_map.hpp"\n'
                   "int main() { slam_amd::KeyframeGraph g; slam_amd::GraphEdge e; float p[9] = {0};\n"
                   "  if (!g.ok()) return 0;\n  g.addNode(p, 3, 3, slam_amd::Pose());\n  return g.calcEdgeIcp(0, 0, e) ? 0 : 1; }\n")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    assert os.path.exists(api.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use"),
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
